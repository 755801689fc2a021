// Evidence of one data set under a grid of (prior scale alpha, noise scale tau) settings (blr_logpdf_grid_*).
// With the base prior precision L0, the base noise S0 and the setting Lw = alpha L0, Sy = tau S0
// (reference src/bayesian_linear_regression.jl:55-58 on BayesianLinearRegressor(mw, alpha L0)(x, tau S0)):
//   G0 = X S0^-1 X'    b0 = X S0^-1 (y - X'mw)    q0 = (y - X'mw)' S0^-1 (y - X'mw)    l0 = logdet S0
//   A = alpha L0 + G0 / tau      T = chol(A).U      u = T^-T b0 / tau      mw' = mw + T^-1 u
//   logpdf = -1/2 [N log 2 pi + N log tau + l0 + q0 / tau + logdet A - D log alpha - logdet L0 - |u|^2]
// D <= 128, four kinds of launch whatever B and G are:
//   grid_prior_kernel   one workgroup per regressor: SPD check and logdet of the base prior (dense: one Cholesky, not one per setting)
//   grid_stats_kernel   one workgroup per (regressor, column block): phase_gram of blr_fused_small.hpp with no prior -- X is read
//                       exactly once -- G0 (packed lower triangle, padded to 16 NB), b0, q0, l0 to the handle's statistics buffer;
//                       grid_reduce_kernel adds the column blocks of a regressor in a fixed order when there is more than one
//   grid_eval_kernel    one workgroup per (regressor, setting): A and b0 / tau in the LDS layout of phase_chol, the factorisation with
//                       the forward substitution, the evidence.  Launched once more over the B winning settings (refit) with the back
//                       substitution and the factor store when mw_best / T_best are asked for
//   grid_argmax_kernel  best[b]: the smallest g among the settings with the largest finite evidence, -1 when there is none
// The column blocks follow from N alone (grid_splits), so the bits of a regressor do not depend on B, and those of a setting not on G.
// phase_chol / phase_backsolve are instantiated with TAG = 1: copies of their own, the existing kernels' code stays as it is.
#pragma once
#include "blr_common.hpp"
#include "blr_fused_small.hpp"

namespace blr {

template <typename T>
struct GridArgs {
  const T* X; int64_t ldx, strideX;
  const T* y; int64_t stridey;
  const T* s; int64_t strides;
  const T* mw; int64_t stridemw;
  const T* Lw; int64_t ldl, strideLw;
  const T* alpha; int64_t stride_alpha;  // NULL: all ones
  const T* tau; int64_t stride_tau;
  double* logpdf; int64_t stride_lp;
  int32_t* info; int64_t stride_info;
  int64_t* best;      // [B], workspace
  int64_t* best_out;  // [B], the caller's (may be NULL)
  T* mw_best; int64_t stride_mwbest;
  T* T_best; int64_t ldt, strideT;
  // statistics buffer: per (regressor, column block) PACKED + DP elements, {q0, l0}, first bad observation; per regressor the prior's
  T* stats; double* scal; int32_t* bad; double* prior_logdet; int32_t* prior_info;
  int layout, noise_kind, prior_kind;
  int D, N, B, G;
  int S, chunk;  // column blocks per regressor, columns per block (grid_splits)
  int refit;     // grid_eval_kernel: one workgroup per regressor on setting best[b], writes mw_best / T_best instead of the evidence
};

constexpr int kGridNoBad = 0x7fffffff;
constexpr int kGridPriorNone = 3;  // phase_gram: neither a precision nor a factor -- the accumulators start from zero

// Column blocks of the statistics pass: one workgroup streaming all of X is a latency floor when B is small, so N is cut into
// blocks of about 1024 columns (at most 8, whole stages of 64).  A function of N alone.
inline void grid_splits(int64_t N, int* S, int* chunk) {
  int64_t s = std::max<int64_t>(1, std::min<int64_t>(8, N / 1024));
  int64_t c = (N + s - 1) / s;
  c = (c + 63) / 64 * 64;
  *S = (int)s;
  *chunk = (int)std::max<int64_t>(c, 64);
}

template <typename T, int NB>
constexpr int grid_stat_elems() { return SmallCfg<T, NB>::PACKED + SmallCfg<T, NB>::DP; }

#define BLR_GRID_BOUNDS(T, NB) __launch_bounds__(kThreads, ((NB) <= 4 ? 4 : (sizeof(T) == 4 ? BLR_F32_WAVES_PER_SIMD : 2)))

// ---- base prior: status (reference :78) and logdet L0, once per regressor ---------------------------------------------------------
template <typename T, int NB>
__global__ BLR_GRID_BOUNDS(T, NB) void grid_prior_kernel(GridArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = SmallCfg<T, NB>;
  T* const P = reinterpret_cast<T*>(smem);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  int* const iscr = reinterpret_cast<int*>(smem + C::OFF_SCR + 64);
  const int tid = threadIdx.x;
  const int D = a.D;
  const int64_t reg = blockIdx.x;
  const T* Lw = a.Lw + reg * a.strideLw;
  int info = 0;
  double logdet = 0.0;
  if (a.prior_kind == PRIOR_DENSE) {
    // upper triangle of the caller's matrix (LAPACK 'U'), as glue_prior reads it
    for (int i = tid >> 6; i < D; i += kWaves)
      for (int k = tid & 63; k <= i; k += kWave) P[pidx(i, k)] = Lw[(int64_t)i * a.ldl + k];
    for (int idx = D * (D + 1) / 2 + tid; idx < C::PACKED; idx += kThreads) P[idx] = T(0);
    __syncthreads();
    info = phase_chol<T, NB, 1>(smem, D, 0);
    const double v = (info == 0 && tid < D) ? log((double)P[pidx(tid, tid)]) : 0.0;
    logdet = 2.0 * block_allreduce(v, scr, tid);
  } else {
    double v = 0.0;
    int bad = kGridNoBad;
    if (tid < D) {
      const T dv = Lw[tid];
      if (dv > T(0)) v = log((double)dv);
      else bad = tid + 1;
    }
    bad = block_min_int(bad, iscr, tid);
    if (bad != kGridNoBad) info = bad;
    logdet = block_allreduce(v, scr, tid);
  }
  if (tid == 0) { a.prior_info[reg] = info; a.prior_logdet[reg] = logdet; }
}

// ---- statistics of one column block: the streaming Gram phase without a prior ----------------------------------------------------
template <typename T, int NB, int MODE>
__global__ BLR_GRID_BOUNDS(T, NB) void grid_stats_kernel(GridArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = SmallCfg<T, NB>;
  T* const P = reinterpret_cast<T*>(smem);
  T* const bvec = reinterpret_cast<T*>(smem + C::OFF_B);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  int* const iscr = reinterpret_cast<int*>(smem + C::OFF_SCR + 64);
  RegCtx<T>* ctx = reinterpret_cast<RegCtx<T>*>(smem + C::OFF_CTX);
  const int tid = threadIdx.x;
  const int64_t wg = blockIdx.x;
  const int64_t reg = wg / a.S;
  const int sp = (int)(wg - reg * a.S);
  const int n0 = sp * a.chunk;
  const int n = max(0, min(a.chunk, a.N - n0));
  const bool diag = a.noise_kind == NOISE_DIAGONAL;
  if (tid == 0) {
    ctx->X = a.X + reg * a.strideX + (a.layout == LAYOUT_COLVECS ? (int64_t)n0 * a.ldx : (int64_t)n0);
    ctx->y = a.y + reg * a.stridey + n0;
    ctx->s = a.s + reg * a.strides + (diag ? n0 : 0);
    ctx->mw = a.mw + reg * a.stridemw;
    ctx->Lw = ctx->mw;  // (a valid address: phase_gram loads one word of it and drops the value)
    ctx->ldx = a.ldx;
    ctx->ldl = 0;
    ctx->D = a.D;
    ctx->N = n;
    ctx->noise_kind = a.noise_kind;
    ctx->prior_kind = kGridPriorNone;
  }
  __syncthreads();
  phase_gram<T, NB, MODE>(smem);
  constexpr int SZ = grid_stat_elems<T, NB>();
  T* const out = a.stats + wg * SZ;
  for (int idx = tid; idx < C::PACKED; idx += kThreads) out[idx] = P[idx];
  if (tid < C::DP) out[C::PACKED + tid] = bvec[tid];
  if (tid == 0) {
    a.scal[2 * wg] = scr[4];
    a.scal[2 * wg + 1] = scr[5];
    const int bad = iscr[6];
    a.bad[wg] = (bad == kGridNoBad || !diag) ? bad : bad + n0;  // (isotropic: observation 1 whichever block sees it)
  }
}

// ---- column blocks 1 .. S-1 of a regressor added to block 0, in that order ---------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void grid_reduce_kernel(GridArgs<T> a, int SZ) {
  const int64_t reg = blockIdx.x;  // (the regressor on grid.x: grid.y ends at 65535)
  T* const st = a.stats + reg * a.S * (int64_t)SZ;
  for (int idx = blockIdx.y * kThreads + threadIdx.x; idx < SZ; idx += gridDim.y * kThreads) {
    double acc = (double)st[idx];
    for (int sp = 1; sp < a.S; ++sp) acc += (double)st[(int64_t)sp * SZ + idx];
    st[idx] = (T)acc;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    double q = a.scal[2 * reg * a.S], l = a.scal[2 * reg * a.S + 1];
    int bad = a.bad[reg * a.S];
    for (int sp = 1; sp < a.S; ++sp) {
      q += a.scal[2 * (reg * a.S + sp)];
      l += a.scal[2 * (reg * a.S + sp) + 1];
      bad = min(bad, a.bad[reg * a.S + sp]);
    }
    a.scal[2 * reg * a.S] = q;
    a.scal[2 * reg * a.S + 1] = l;
    a.bad[reg * a.S] = bad;
  }
}

// ---- one setting: A = alpha L0 + G0 / tau, its factor, the evidence (or, refit, the posterior) -------------------------------------
template <typename T, int NB>
__global__ BLR_GRID_BOUNDS(T, NB) void grid_eval_kernel(GridArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = SmallCfg<T, NB>;
  static_assert(2 * C::LDS_BYTES <= 160 * 1024, "two workgroups per CU: twice the dynamic LDS of a launch must fit 160 KB");
  constexpr int SZ = grid_stat_elems<T, NB>();
  T* const P = reinterpret_cast<T*>(smem);
  T* const bvec = reinterpret_cast<T*>(smem + C::OFF_B);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  const int tid = threadIdx.x;
  const int D = a.D;
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  int64_t reg;
  int g;
  if (a.refit) {
    reg = blockIdx.x;
    const int64_t bg = a.best[reg];
    if (bg < 0) return;  // nothing succeeded: mw_best / T_best stay as they are
    g = (int)bg;
  } else {
    reg = blockIdx.x / a.G;
    g = (int)(blockIdx.x - reg * a.G);
  }
  const T alpha = a.alpha ? a.alpha[reg * a.stride_alpha + g] : T(1);
  const T tau = a.tau ? a.tau[reg * a.stride_tau + g] : T(1);
  const int64_t slot = reg * a.S;
  // status in the reference's order: prior (:78), noise (:79); block-uniform
  int info = 0;
  if (!(alpha > T(0)) || !isfinite((double)alpha)) info = 1;
  else if (a.prior_info[reg] != 0) info = a.prior_info[reg];
  else if (!(tau > T(0)) || !isfinite((double)tau)) info = 1;
  else if (a.bad[slot] != kGridNoBad) info = a.bad[slot];
  int32_t* const info_out = a.info + reg * a.stride_info + g;
  double* const lp_out = a.logpdf + reg * a.stride_lp + g;
  if (info != 0) {
    if (!a.refit && tid == 0) { *info_out = info; *lp_out = kNaN; }
    return;
  }
  const T rt = T(1) / tau;
  const T* const st = a.stats + slot * SZ;
  for (int idx = tid; idx < C::PACKED; idx += kThreads) P[idx] = st[idx] * rt;
  if (tid < C::DP) bvec[tid] = st[C::PACKED + tid] * rt;
  __syncthreads();
  const T* Lw = a.Lw + reg * a.strideLw;
  if (a.prior_kind == PRIOR_DENSE) {
    for (int i = tid >> 6; i < D; i += kWaves)
      for (int k = tid & 63; k <= i; k += kWave) P[pidx(i, k)] += alpha * Lw[(int64_t)i * a.ldl + k];
  } else if (tid < D) {
    P[pidx(tid, tid)] += alpha * Lw[tid];
  }
  __syncthreads();
  info = phase_chol<T, NB, 1>(smem, D, 1);  // :86, with u = T^-T b riding along
  if (info != 0) {
    if (!a.refit && tid == 0) { *info_out = info; *lp_out = kNaN; }
    return;
  }
  if (a.refit) {
    phase_backsolve<T, NB, 1>(smem, D, a.T_best ? a.T_best + reg * a.strideT : (T*)nullptr, a.ldt);
    if (a.mw_best && tid < D) a.mw_best[reg * a.stride_mwbest + tid] = (a.mw + reg * a.stridemw)[tid] + bvec[tid];  // :68
    return;
  }
  double uu = 0.0, ld = 0.0;
  if (tid < D) {
    const double u = (double)bvec[tid];
    uu = u * u;
    ld = log((double)P[pidx(tid, tid)]);
  }
  uu = block_allreduce(uu, scr, tid);
  ld = 2.0 * block_allreduce(ld, scr, tid);  // logdet A
  if (tid == 0) {
    const double LOG2PI = 1.8378770664093454835606594728112;
    const double t = (double)tau, N = (double)a.N;
    *info_out = 0;
    *lp_out = -0.5 * (N * LOG2PI + N * log(t) + a.scal[2 * slot + 1] + a.scal[2 * slot] / t + ld - (double)D * log((double)alpha) -
                      a.prior_logdet[reg] - uu);
  }
}

// ---- best[b]: first of the settings with the largest finite evidence ---------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grid_argmax_kernel(const double* __restrict__ logpdf, int64_t stride_lp, int G, int B,
                                                               int64_t* __restrict__ best, int64_t* __restrict__ best_out) {
  const int64_t reg = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (reg >= B) return;
  int64_t arg = -1;
  double top = 0.0;
  for (int g = 0; g < G; ++g) {
    const double v = logpdf[reg * stride_lp + g];
    if (isfinite(v) && (arg < 0 || v > top)) { arg = g; top = v; }
  }
  best[reg] = arg;
  if (best_out) best_out[reg] = arg;
}

// ---- D > 128: the operands of one setting, s' = tau s and Lw' = alpha Lw, for the existing pipeline --------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void grid_scale_kernel(GridArgs<T> a, int64_t reg0, int g, T* __restrict__ s_out, int64_t s_one,
                                                              T* __restrict__ Lw_out, int64_t lw_one) {
  const int64_t r = blockIdx.y, reg = reg0 + r;
  const T alpha = a.alpha ? a.alpha[reg * a.stride_alpha + g] : T(1);
  const T tau = a.tau ? a.tau[reg * a.stride_tau + g] : T(1);
  const T* s = a.s + reg * a.strides;
  const T* Lw = a.Lw + reg * a.strideLw;
  const int64_t i0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  for (int64_t i = i0; i < s_one; i += step) s_out[r * s_one + i] = tau * s[i];
  if (a.prior_kind == PRIOR_DENSE) {
    const int64_t D = a.D;
    for (int64_t e = i0; e < D * D; e += step) {
      const int64_t c = e / D, row = e - c * D;
      Lw_out[r * lw_one + e] = alpha * Lw[c * a.ldl + row];
    }
  } else {
    for (int64_t i = i0; i < a.D; i += step) Lw_out[r * lw_one + i] = alpha * Lw[i];
  }
}

// one evidence / status per regressor of a setting -> the caller's [B][G] arrays (NaN where the setting failed)
__global__ __launch_bounds__(kThreads) void grid_scatter_kernel(const double* __restrict__ lp, const int32_t* __restrict__ inf, int B, int g,
                                                                double* __restrict__ logpdf, int64_t stride_lp, int32_t* __restrict__ info,
                                                                int64_t stride_info) {
  const int64_t reg = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (reg >= B) return;
  info[reg * stride_info + g] = inf[reg];
  logpdf[reg * stride_lp + g] = inf[reg] == 0 ? lp[reg] : __longlong_as_double(0x7ff8000000000000LL);
}

}  // namespace blr
