// Evidence grid for a batch whose regressors have UNEQUAL observation counts (blr_logpdf_grid_ragged_*).
//
// Replaces reference src/bayesian_linear_regression.jl:55-58 on BayesianLinearRegressor(mw, alpha L0)(x, tau S0), per setting, under a
// map over fxs of different lengths.  The observations are packed as in blr_posterior_ragged_*; regressor b owns columns
// [offsets[b], offsets[b+1]).  The algebra and the launches are those of blr_grid.hpp (K13):
//   grid_prior_kernel               as it is: already one workgroup per regressor (launched by blr_abi.hip)
//   ragged_evidence_stats_kernel    one workgroup per ITEM of the host plan (blr_grid_ragged_plan.hpp): one column block of one
//                                   regressor, longest block first; phase_gram without a prior on the block, the statistics to the
//                                   item's slot
//   ragged_evidence_reduce_kernel   blocks 1 .. S_b - 1 of a regressor added to its block 0 in that order, in double
//   ragged_evidence_eval_kernel     one workgroup per (regressor, setting), then one per regressor on the winner (refit): the
//                                   statistics at slot0[reg], the regressor's own N in the evidence
//   grid_argmax_kernel              as it is
// The column blocks of a regressor are those blr_logpdf_grid_* cuts at N = N_b, every sum runs in the same order and the phases are
// the same code on the same data: the bits of regressor b are those of blr_logpdf_grid_* with B = 1 on its slice.  No atomics.
//
// The kernels here are copies of the bodies of grid_stats_kernel / grid_reduce_kernel / grid_eval_kernel with the slice, the slot
// and N taken from the plan's tables; blr_grid.hpp and the code objects of its kernels stay exactly as they are.  They are
// instantiated in a unit of their own (blr_grid_ragged.hip), phase_chol / phase_backsolve with TAG = 3.  This header does not include
// blr_grid.hpp (that one defines kernels that are not templates: one translation unit only); blr_abi.hip, which sees both, asserts
// that the constants repeated here agree.
#pragma once
#include "blr_common.hpp"
#include "blr_fused_small.hpp"
#include "blr_grid_ragged_plan.hpp"

namespace blr {

template <typename T>
struct RaggedEvidenceArgs {
  const T* X; int64_t ldx;      // the packed arrays' bases
  const T* y;
  const T* s; int64_t strides;  // diagonal: packed like y; isotropic: s[reg * strides]
  const T* mw; int64_t stridemw;
  const T* Lw; int64_t ldl, strideLw;
  const T* alpha; int64_t stride_alpha;  // NULL: all ones
  const T* tau; int64_t stride_tau;
  double* logpdf; int64_t stride_lp;
  int32_t* info; int64_t stride_info;
  const int64_t* best;  // [B], workspace (grid_argmax_kernel)
  T* mw_best; int64_t stride_mwbest;
  T* T_best; int64_t ldt, strideT;
  // statistics buffer: per slot PACKED + DP elements, {q0, l0}, first bad observation; per regressor the prior's (grid_prior_kernel)
  T* stats; double* scal; int32_t* bad; const double* prior_logdet; const int32_t* prior_info;
  const int64_t* offsets;       // [B + 1], device
  const int32_t* slot0;         // [B + 1], device
  const GridRaggedItem* items;  // [slot0[B]], device, longest block first
  int layout, noise_kind, prior_kind;
  int D, B, G;
  int refit;  // ragged_evidence_eval_kernel: one workgroup per regressor on setting best[b], writes mw_best / T_best
};

constexpr int kEvidenceNoBad = 0x7fffffff;  // = kGridNoBad
constexpr int kEvidencePriorNone = 3;       // = kGridPriorNone
constexpr int kEvidenceTag = 3;             // phase_chol / phase_backsolve: copies of this unit's own

template <typename T, int NB>
constexpr int evidence_stat_elems() { return SmallCfg<T, NB>::PACKED + SmallCfg<T, NB>::DP; }  // = grid_stat_elems

#ifndef BLR_GRID_BOUNDS
#define BLR_GRID_BOUNDS(T, NB) __launch_bounds__(kThreads, ((NB) <= 4 ? 4 : (sizeof(T) == 4 ? BLR_F32_WAVES_PER_SIMD : 2)))
#endif

// ---- statistics of one item: the streaming Gram phase without a prior on one column block of one regressor ------------------------
template <typename T, int NB, int MODE>
__global__ BLR_GRID_BOUNDS(T, NB) void ragged_evidence_stats_kernel(RaggedEvidenceArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = SmallCfg<T, NB>;
  T* const P = reinterpret_cast<T*>(smem);
  T* const bvec = reinterpret_cast<T*>(smem + C::OFF_B);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  int* const iscr = reinterpret_cast<int*>(smem + C::OFF_SCR + 64);
  RegCtx<T>* ctx = reinterpret_cast<RegCtx<T>*>(smem + C::OFF_CTX);
  const int tid = threadIdx.x;
  const GridRaggedItem it = a.items[blockIdx.x];
  const int64_t reg = it.reg, wg = it.slot;
  const int n0 = it.n0;
  const bool diag = a.noise_kind == NOISE_DIAGONAL;
  if (tid == 0) {
    const int64_t o = a.offsets[reg] + n0;
    ctx->X = a.X + (a.layout == LAYOUT_COLVECS ? o * a.ldx : o);
    ctx->y = a.y + o;
    ctx->s = diag ? a.s + o : a.s + reg * a.strides;
    ctx->mw = a.mw + reg * a.stridemw;
    ctx->Lw = ctx->mw;  // (a valid address: phase_gram loads one word of it and drops the value)
    ctx->ldx = a.ldx;
    ctx->ldl = 0;
    ctx->D = a.D;
    ctx->N = it.n;
    ctx->noise_kind = a.noise_kind;
    ctx->prior_kind = kEvidencePriorNone;
  }
  __syncthreads();
  phase_gram<T, NB, MODE>(smem);
  constexpr int SZ = evidence_stat_elems<T, NB>();
  T* const out = a.stats + wg * SZ;
  for (int idx = tid; idx < C::PACKED; idx += kThreads) out[idx] = P[idx];
  if (tid < C::DP) out[C::PACKED + tid] = bvec[tid];
  if (tid == 0) {
    a.scal[2 * wg] = scr[4];
    a.scal[2 * wg + 1] = scr[5];
    const int bad = iscr[6];
    a.bad[wg] = (bad == kEvidenceNoBad || !diag) ? bad : bad + n0;  // (1-based within the regressor's own slice)
  }
}

// ---- column blocks 1 .. S_b - 1 of a regressor added to block 0, in that order -------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void ragged_evidence_reduce_kernel(RaggedEvidenceArgs<T> a, int SZ) {
  const int64_t reg = blockIdx.x;  // (the regressor on grid.x: grid.y ends at 65535)
  const int64_t slot = a.slot0[reg];
  const int S = (int)(a.slot0[reg + 1] - slot);
  if (S <= 1) return;
  T* const st = a.stats + slot * (int64_t)SZ;
  for (int idx = blockIdx.y * kThreads + threadIdx.x; idx < SZ; idx += gridDim.y * kThreads) {
    double acc = (double)st[idx];
    for (int sp = 1; sp < S; ++sp) acc += (double)st[(int64_t)sp * SZ + idx];
    st[idx] = (T)acc;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    double q = a.scal[2 * slot], l = a.scal[2 * slot + 1];
    int bad = a.bad[slot];
    for (int sp = 1; sp < S; ++sp) {
      q += a.scal[2 * (slot + sp)];
      l += a.scal[2 * (slot + sp) + 1];
      bad = min(bad, a.bad[slot + sp]);
    }
    a.scal[2 * slot] = q;
    a.scal[2 * slot + 1] = l;
    a.bad[slot] = bad;
  }
}

// ---- one setting: A = alpha L0 + G0 / tau, its factor, the evidence (or, refit, the posterior) -------------------------------------
template <typename T, int NB>
__global__ BLR_GRID_BOUNDS(T, NB) void ragged_evidence_eval_kernel(RaggedEvidenceArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = SmallCfg<T, NB>;
  static_assert(2 * C::LDS_BYTES <= 160 * 1024, "two workgroups per CU: twice the dynamic LDS of a launch must fit 160 KB");
  constexpr int SZ = evidence_stat_elems<T, NB>();
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
  const int64_t slot = a.slot0[reg];
  // status in the reference's order: prior (:78), noise (:79); block-uniform
  int info = 0;
  if (!(alpha > T(0)) || !isfinite((double)alpha)) info = 1;
  else if (a.prior_info[reg] != 0) info = a.prior_info[reg];
  else if (!(tau > T(0)) || !isfinite((double)tau)) info = 1;
  else if (a.bad[slot] != kEvidenceNoBad) info = a.bad[slot];
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
  info = phase_chol<T, NB, kEvidenceTag>(smem, D, 1);  // :86, with u = T^-T b riding along
  if (info != 0) {
    if (!a.refit && tid == 0) { *info_out = info; *lp_out = kNaN; }
    return;
  }
  if (a.refit) {
    phase_backsolve<T, NB, kEvidenceTag>(smem, D, a.T_best ? a.T_best + reg * a.strideT : (T*)nullptr, a.ldt);
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
    const double t = (double)tau, N = (double)(int)(a.offsets[reg + 1] - a.offsets[reg]);
    *info_out = 0;
    *lp_out = -0.5 * (N * LOG2PI + N * log(t) + a.scal[2 * slot + 1] + a.scal[2 * slot] / t + ld - (double)D * log((double)alpha) -
                      a.prior_logdet[reg] - uu);
  }
}

// ---- host side of the instantiations (blr_grid_ragged.hip), used by blr_abi.hip ------------------------------------------------------
// mode: 0, 1 or 4; NB: 1 .. 8.  The *_ptr functions give what hipFuncSetAttribute wants (NULL: not in this build, BLR_DEV_FAST)
const void* ragged_evidence_stats_ptr_f64(int NB, int mode);
const void* ragged_evidence_stats_ptr_f32(int NB, int mode);
const void* ragged_evidence_eval_ptr_f64(int NB);
const void* ragged_evidence_eval_ptr_f32(int NB);
size_t ragged_evidence_lds_f64(int NB);
size_t ragged_evidence_lds_f32(int NB);
int ragged_evidence_stat_elems_f64(int NB);
int ragged_evidence_stat_elems_f32(int NB);
void ragged_evidence_stats_launch_f64(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<double>& a);
void ragged_evidence_stats_launch_f32(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<float>& a);
void ragged_evidence_reduce_launch_f64(int NB, unsigned B, hipStream_t stream, const RaggedEvidenceArgs<double>& a);
void ragged_evidence_reduce_launch_f32(int NB, unsigned B, hipStream_t stream, const RaggedEvidenceArgs<float>& a);
void ragged_evidence_eval_launch_f64(int NB, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<double>& a);
void ragged_evidence_eval_launch_f32(int NB, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<float>& a);

}  // namespace blr
