// Exact leave-one-out predictives of a batched MULTI-OUTPUT state (blr_loo_multi_batched_*): S target columns share
// one factor per regressor, so the leverage of an input is computed once and only the residual depends on the column.
//
// Replaces reference src/bayesian_linear_regression.jl:55-58 per held-out point and column (the repeated conditioning its test
// :49-70 runs).  With A = T'T, M the D x S mean block and s_n the noise variance:
//   sigma2_n = |T^-T x_n|^2,  1 - h_n = (s_n - sigma2_n) / s_n,  loo_var_n = s_n / (1 - h_n)      once per input
//   m_nc = x_n'M[:, c],  r_nc = Y[n, c] - m_nc,  loo_mean_nc = Y[n, c] - r_nc / (1 - h_n),
//   loo_logpdf_nc = -1/2 [log 2 pi + log s_n - log(1 - h_n) + r_nc^2 / (s_n (1 - h_n))]            per input and column
// The epilogue is loo_predictive (blr_loo.hpp), the one place the formula lives.
//
// loo_cols_kernel: grid (tile groups, regressors), 256 threads.  The tile layout, the staging through registers, the image of
// L^-T in LDS (marg_image_kernel, blr_marginals.hpp) and the prefetch of the next tile are those of marginals_cols_kernel
// (blr_marg_multi.hpp).  The leverage is needed by every column and workgroups of one launch cannot hand it to each other, so a
// workgroup KEEPS its tile and loops over the column passes instead of putting the passes on the grid.  Per tile:
//   once       z' = (L^-T)'x on the matrix cores; every lane of a wave then holds sigma2 of its input: loo_var is stored and the
//              degenerate inputs are counted (once per input, whatever S is);
//   per pass   the A fragments of kLooColsPerPass columns of M (from the L2-resident block; with a single pass they are loaded once
//              per workgroup), mean' = M'X_tile' as in marginals_cols_kernel, then for the lane's four (n, c) pairs Y[n, c], the
//              epilogue in double and the stores, coalesced along n.
// X is read from HBM once whatever S is; nothing N-long but the outputs reaches memory.  Every sum has a fixed order, nothing
// floating-point is atomic, and an output row of an MFMA depends on its own A row only: the bits of a column do not depend on S, on
// its pass or slot or on the other columns; those of loo_var not on S or on which other outputs are wanted.
// loo_cols_total_kernel: the fixed-order block sum once per (column, regressor).
// D > 128: loo_cols_finish_kernel over the large-D variance route and the projected means in handle workspace (correct, not fast).
#pragma once
#include "blr_loo.hpp"
#include "blr_marg_multi.hpp"

namespace blr {

constexpr int kLooColsPerPass = kMargColsPerPass;  // columns of M per pass (mirrored as _abi.LOO_COLS_PER_PASS)

template <typename T>
struct LooColsArgs {
  const T* X; int64_t ldx, strideX;
  const T* Y; int64_t ldY, strideY;          // N x S targets per regressor
  const T* s; int64_t strides;
  const T* M; int64_t ldm, strideM;          // D x S mean columns per regressor
  const T* img;                              // images of L^-T, IMG_ELEMS apart, the launch's first regressor first
  const int32_t* info;                       // [B] status of loo_check_kernel: a regressor with info != 0 is skipped
  T* lm; int64_t ld_lm, stride_lm;           // LOO means, N x S (may be NULL)
  T* lv; int64_t stride_lv;                  // LOO variances, N (may be NULL)
  double* ll; int64_t ld_ll, stride_ll;      // LOO log densities, N x S (may be NULL)
  unsigned long long* degenerate;            // inputs with 1 - h_n <= 0 or not finite (blr_get_stat "loo_degenerate")
  int noise_kind, D, N, S;
  int ngroups;                               // tile groups per regressor (= gridDim.x)
  int reg0;                                  // first regressor of this launch (grid.y <= 65535)
};

// dynamic LDS of a launch: the "with image" footprint of marginals_cols_kernel (its 1 / d slot stays unused)
inline size_t loo_cols_lds_bytes(size_t elem, int D) { return marg_cols_lds_bytes(elem, D, true); }

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void loo_cols_kernel(LooColsArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Mf = Mfma<T>;
  using G = MargGemmCfg<T>;
  using acc4 = typename Mf::acc4;
  constexpr int W = kLooColsPerPass, TN = kMargTile, VEC = Mf::VEC;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  if (a.info[reg] != 0) return;  // (block-uniform) the state failed the check: outputs untouched
  const int grp = blockIdx.x;
  const int D = a.D, N = a.N;
  const int NB = (D + 15) / 16, DP = 16 * NB, NK = DP / 4, LDX = marg_cols_ldx<T>(DP);
  const bool do_cols = a.lm != nullptr || a.ll != nullptr;
  const int npasses = do_cols ? (a.S + W - 1) / W : 0;

  T* const Xs = reinterpret_cast<T*>(smem);        // [TN][LDX]
  T* const img = Xs + TN * LDX + kMargMaxD;        // [2 NB (NB + 1)][64]

  const BLR_GLOBAL T* const Xg = as_global(a.X + reg * a.strideX);
  const BLR_GLOBAL T* const sg = as_global(a.s + reg * a.strides);
  const BLR_GLOBAL T* const Yg = as_global(a.Y + reg * a.strideY);
  const BLR_GLOBAL T* const Mg = as_global(a.M + reg * a.strideM);
  const int ntiles = (N + TN - 1) / TN;

  // ---- the tile through registers, as marginals_cols_kernel stages it ----
  const int xcnt = DP / 4;
  T xreg[32];
  auto prefetch = [&](int tile) {
    const int n0 = tile * TN;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      if (i < xcnt) {
        const int e = tid + kThreads * i;
        int d, n;
        if (LAYOUT == LAYOUT_COLVECS) { d = (tid & 15) + 16 * (i >> 2); n = (tid >> 4) + 16 * (i & 3); } else { n = e % TN; d = e / TN; }
        const bool ok = d < D && n0 + n < N;
        const int64_t at = LAYOUT == LAYOUT_COLVECS ? (int64_t)d + (int64_t)(n0 + n) * a.ldx : (int64_t)(n0 + n) + (int64_t)d * a.ldx;
        xreg[i] = ok ? Xg[at] : T(0);
      }
    }
  };
  if (grp < ntiles) prefetch(grp);

  // A fragments of M' for one pass: mf[ks] = M[4 ks + g, c0 + li]
  T mf[32];
  auto load_fragments = [&](int c0) {
    const bool cok = c0 + li < a.S;
    const BLR_GLOBAL T* const Mc = Mg + (int64_t)(cok ? c0 + li : 0) * a.ldm;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
      mf[ks] = T(0);
      if (ks < NK) {
        const int d = 4 * ks + g;
        if (cok && d < D) mf[ks] = Mc[d];
      }
    }
  };
  if (npasses == 1) load_fragments(0);  // a single pass: once per workgroup
  {
    const BLR_GLOBAL vecT* const src = reinterpret_cast<const BLR_GLOBAL vecT*>(as_global(a.img + (int64_t)blockIdx.y * G::IMG_ELEMS));
    vecT* const dst = reinterpret_cast<vecT*>(img);
    const int nvec = G::frag0(NB) * 64 / VEC;
    for (int e = tid; e < nvec; e += kThreads) dst[e] = src[e];
  }
  const T s_iso = (a.noise_kind == NOISE_ISOTROPIC && N > 0) ? sg[0] : T(1);

  int ndeg = 0;
  const int row = 16 * wave + li;  // this lane's input of the tile (the same in its four lane groups)
  for (int tile = grp; tile < ntiles; tile += a.ngroups) {
    const int n0 = tile * TN;
    __syncthreads();  // the previous tile's readers of Xs are done (first tile: nothing pending)
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      if (i < xcnt) {
        const int e = tid + kThreads * i;
        int d, n;
        if (LAYOUT == LAYOUT_COLVECS) { d = (tid & 15) + 16 * (i >> 2); n = (tid >> 4) + 16 * (i & 3); } else { n = e % TN; d = e / TN; }
        Xs[n * LDX + d] = xreg[i];
      }
    }
    __syncthreads();  // (also: the image in place)
    if (tile + a.ngroups < ntiles) prefetch(tile + a.ngroups);  // in flight during this tile's products
    const int n = n0 + row;
    const bool nok = n < N;
    const T sv = a.noise_kind == NOISE_DIAGONAL ? (nok ? sg[n] : T(1)) : s_iso;
    const T* const xr = Xs + row * LDX;

    // sigma2_n = |L^-1 x_n|^2: after the butterfly every lane group holds it for its input
    T sq = T(0);
#pragma unroll 1
    for (int J = 0; J < NB; ++J) {
      acc4 acc = {T(0), T(0), T(0), T(0)};
      const T* const fb = img + G::frag0(J) * 64 + lane;
#pragma unroll 4
      for (int m = 0; m < 4 * (J + 1); ++m) acc = Mf::mma(fb[m * 64], xr[G::d_of(m, g)], acc);
#pragma unroll
      for (int v = 0; v < 4; ++v) sq += acc[v] * acc[v];
    }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    const double sig2 = (double)sq, sd = (double)sv;
    __builtin_amdgcn_sched_barrier(0);
    {  // once per input: the variance and the count (y = m = 0: the same expression whatever the columns are)
      LooOut o;
      const bool ok = loo_predictive(0.0, 0.0, sig2, sd, o);
      if (g == 0 && nok) {
        if (a.lv) a.lv[reg * a.stride_lv + n] = (T)o.var;
        if (!ok) ++ndeg;
      }
    }
    __builtin_amdgcn_sched_barrier(0);

    for (int pass = 0; pass < npasses; ++pass) {
      const int c0 = pass * W;
      if (npasses > 1) load_fragments(c0);
      // mean' = M'X_tile': acc[v] = column c0 + crow(lane, v) at input n
      acc4 acc = {T(0), T(0), T(0), T(0)};
#pragma unroll
      for (int ks = 0; ks < 32; ++ks)
        if (ks < NK) acc = Mf::mma(mf[ks], xr[4 * ks + g], acc);
      __builtin_amdgcn_sched_barrier(0);  // the double-precision epilogue stays out of the products (it spilled there, K12)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int c = c0 + Mf::crow(lane, v);
        if (nok && c < a.S) {
          const double y = (double)Yg[(int64_t)c * a.ldY + n];
          LooOut o;
          loo_predictive(y, (double)acc[v], sig2, sd, o);
          if (a.lm) a.lm[reg * a.stride_lm + (int64_t)c * a.ld_lm + n] = (T)o.mean;
          if (a.ll) a.ll[reg * a.stride_ll + (int64_t)c * a.ld_ll + n] = o.logpdf;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  loo_count(ndeg, a.degenerate);  // (all 64 lanes)
}

// ---- D > 128: the epilogue over the latent variance (var, ldw apart per regressor of the chunk) and the projected means
// (mean, N x S with leading dimension ldmn, stridemn apart) in handle workspace ---------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void loo_cols_finish_kernel(LooColsArgs<T> a, const T* __restrict__ mean, int64_t ldmn, int64_t stridemn,
                                                                   const T* __restrict__ var, int64_t ldw) {
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  if (a.info[reg] != 0) return;
  const T* const s = a.s + reg * a.strides;
  const T* const Y = a.Y + reg * a.strideY;
  const T* const m = mean + (int64_t)blockIdx.y * stridemn;
  const T* const v = var + (int64_t)blockIdx.y * ldw;
  const bool diag = a.noise_kind == NOISE_DIAGONAL;
  int ndeg = 0;
  for (int n = blockIdx.x * kThreads + threadIdx.x; n < a.N; n += gridDim.x * kThreads) {
    const double sig2 = (double)v[n], sd = (double)(diag ? s[n] : s[0]);
    LooOut o;
    if (!loo_predictive(0.0, 0.0, sig2, sd, o)) ++ndeg;
    if (a.lv) a.lv[reg * a.stride_lv + n] = (T)o.var;
    if (a.lm || a.ll) {
      for (int c = 0; c < a.S; ++c) {
        loo_predictive((double)Y[(int64_t)c * a.ldY + n], (double)m[(int64_t)c * ldmn + n], sig2, sd, o);
        if (a.lm) a.lm[reg * a.stride_lm + (int64_t)c * a.ld_lm + n] = (T)o.mean;
        if (a.ll) a.ll[reg * a.stride_ll + (int64_t)c * a.ld_ll + n] = o.logpdf;
      }
    }
  }
  loo_count(ndeg, a.degenerate);
}

// ---- loo_total[reg][c] = sum_n logpdf[n, c] in a fixed order: one workgroup per (column, regressor) (defined in blr_loo_multi.hip) ------
__global__ __launch_bounds__(kThreads) void loo_cols_total_kernel(const double* __restrict__ ll, int64_t ld_ll, int64_t stride_ll, int N, double* __restrict__ total,
                                      int64_t stride_lt, const int32_t* __restrict__ info, int reg0);

// the instantiations the library uses, defined in blr_loo_multi.hip
extern template __global__ void loo_cols_kernel<double, LAYOUT_COLVECS>(LooColsArgs<double>);
extern template __global__ void loo_cols_kernel<double, LAYOUT_ROWVECS>(LooColsArgs<double>);
extern template __global__ void loo_cols_kernel<float, LAYOUT_COLVECS>(LooColsArgs<float>);
extern template __global__ void loo_cols_kernel<float, LAYOUT_ROWVECS>(LooColsArgs<float>);
extern template __global__ void loo_cols_finish_kernel<double>(LooColsArgs<double>, const double*, int64_t, int64_t, const double*, int64_t);
extern template __global__ void loo_cols_finish_kernel<float>(LooColsArgs<float>, const float*, int64_t, int64_t, const float*, int64_t);

}  // namespace blr
