// Marginals of a batched multi-output posterior (blr_marginals_multi_batched_*): S mean columns and one variance per
// input and regressor, from ONE read of X per column pass.
//
// Replaces reference src/bayesian_linear_regression.jl:33 (mean), :40-43 (var) and :47 (mean_and_var) under a map over fxs whose
// regressors come from matrix targets: the S column posteriors of a regressor share the factor, so var_n = |U^-T x_n|^2 + Sy_nn is
// computed once per input, and the S means are one N x D x S product.
//
// marginals_cols_kernel: grid (column passes x tile groups, regressors), 256 threads.  A pass takes kMargColsPerPass columns of M; a
// workgroup walks a strided set of 64-input tiles of its regressor.  Per workgroup:
//   once     the pass's columns of M go from global memory straight into REGISTERS as the A fragments of the transposed product
//            mean' = M'X_tile (lane (i, g) of k-step ks: M[4 ks + g, column i]; 2 x 32 registers in fp64) -- no LDS for M, so the
//            pass width is what the register file holds beside the staged tile, not what is left of the LDS;
//            pass 0 with a factor: the regressor's triangular inverse L^-T in MFMA fragment order (marg_image_kernel,
//            blr_marginals.hpp: formed once per regressor by the launch before this one) goes into LDS; with a diagonal prior 1 / d.
//   per tile the inputs become the ROWS of an LDS block through registers (one code path for both layouts: the loads run along the
//            contiguous index, the next tile's are in flight during this tile's products); wave w owns rows 16 w .. 16 w + 15:
//            mean'  = M'X_tile' on v_mfma_f64_16x16x4 / v_mfma_f32_16x16x4, k = d ascending; the accumulator holds 16 consecutive
//                     inputs per column: stores coalesced along n;
//            z'     = (L^-T)'x (pass 0 only), column block by column block as marginals_gemm_kernel does; var_n = |z_n|^2 + s_n.
// Every sum has a fixed order, nothing is atomic, and an output row of an MFMA depends on its own A row only: the bits of a column
// do not depend on S, on its pass or slot or on the other columns; those of var not on S or on whether the means are wanted.
#pragma once
#include "blr_common.hpp"
#include "blr_marg_image.hpp"

namespace blr {

constexpr int kMargColsPerPass = 16;  // columns of M per pass: one 16-row A operand, resident in registers
constexpr int kMargTile = 64;         // inputs per tile: one 16-input MFMA tile per wave
constexpr int kMargMaxD = kPB;        // the image of L^-T (MargGemmCfg, written by marg_image_kernel) covers one 128-block

template <typename T>
struct MargColsArgs {
  const T* X; int64_t ldx, strideX;
  const T* s; int64_t strides;
  const T* M; int64_t ldm, strideM;    // D x S weight columns per regressor
  const T* dprior; int64_t stridedp;   // PRIOR_DIAGONAL: the diagonal of the precision
  const T* img;                        // PRIOR_UPPER_FACTOR: images of L^-T, IMG_ELEMS apart, the launch's first regressor first
  const int32_t* info;                 // [B] status of a dense prior's factorisation (may be NULL)
  T* mean; int64_t ldmean, stridemean;
  T* var; int64_t stridevar;
  int noise_kind, prior_kind, D, N, S;
  int ngroups;                         // tile groups per (regressor, pass): blockIdx.x = pass * ngroups + group
  int reg0;                            // first regressor of this launch (grid.y <= 65535)
};

// row stride of the tile: 16 bytes over the padded width.  The B operand of the mean product (lane (i, g) reads row i, column
// 4 ks + g) then falls into distinct banks for each lane group of an LDS access (fp64: rows 2 banks x (DP + 2) apart, 32 lanes; fp32:
// DP + 4, 64 lanes); the image product reads columns VEC g apart and pays a 2-way (fp64) / 4-way (fp32) conflict on that one read
// per MFMA.
template <typename T>
__host__ __device__ constexpr int marg_cols_ldx(int DP) { return DP + 16 / (int)sizeof(T); }

// dynamic LDS of a launch: the tile, 1 / d of a diagonal prior, and the image's column blocks in use when any pass needs them
inline size_t marg_cols_lds_bytes(size_t elem, int D, bool with_image) {
  const int NB = (D + 15) / 16, DP = 16 * NB;
  const size_t tile = (size_t)kMargTile * (size_t)(DP + 16 / (int)elem) * elem;
  return tile + (size_t)kMargMaxD * elem + (with_image ? (size_t)2 * NB * (NB + 1) * 64 * elem : 0);
}

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void marginals_cols_kernel(MargColsArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Mf = Mfma<T>;
  using G = MargGemmCfg<T>;
  using acc4 = typename Mf::acc4;
  constexpr int W = kMargColsPerPass, TN = kMargTile, VEC = Mf::VEC;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  if (a.info && a.info[reg] != 0) return;  // (block-uniform) the prior is not positive definite: outputs untouched
  const int pass = blockIdx.x / a.ngroups, grp = blockIdx.x % a.ngroups;
  const int D = a.D, N = a.N;
  const int NB = (D + 15) / 16, DP = 16 * NB, NK = DP / 4, LDX = marg_cols_ldx<T>(DP);
  const int c0 = pass * W;
  const int ncols = min(W, a.S - c0);
  const bool do_mean = a.mean != nullptr && ncols > 0;
  const bool do_var = a.var != nullptr && pass == 0;
  const bool use_img = do_var && a.prior_kind == PRIOR_UPPER_FACTOR;
  const bool use_diag = do_var && a.prior_kind == PRIOR_DIAGONAL;
  if (!do_mean && !do_var) return;

  T* const Xs = reinterpret_cast<T*>(smem);  // [TN][LDX]
  T* const dinv = Xs + TN * LDX;            // [128]
  T* const img = dinv + kMargMaxD;           // [2 NB (NB + 1)][64]

  const BLR_GLOBAL T* const Xg = as_global(a.X + reg * a.strideX);
  const BLR_GLOBAL T* const sg = a.s ? as_global(a.s + reg * a.strides) : nullptr;
  const int ntiles = (N + TN - 1) / TN;

  // ---- the tile through registers: DP / 4 elements per thread, loads along the contiguous index of the layout (ColVecs: sixteen
  // consecutive d of four inputs per 16-feature block; RowVecs: the 64 inputs of a feature) ----
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

  // ---- once per workgroup ----
  T mf[32];  // A fragments of M' for this pass: mf[ks] = M[4 ks + g, c0 + li]
  {
    const BLR_GLOBAL T* const Mg = do_mean ? as_global(a.M + reg * a.strideM + (int64_t)(c0 + li) * a.ldm) : nullptr;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
      mf[ks] = T(0);
      if (ks < NK) {
        const int d = 4 * ks + g;
        if (do_mean && li < ncols && d < D) mf[ks] = Mg[d];
      }
    }
  }
  if (use_img) {
    const BLR_GLOBAL vecT* const src = reinterpret_cast<const BLR_GLOBAL vecT*>(as_global(a.img + (int64_t)blockIdx.y * G::IMG_ELEMS));
    vecT* const dst = reinterpret_cast<vecT*>(img);
    const int nvec = G::frag0(NB) * 64 / VEC;
    for (int e = tid; e < nvec; e += kThreads) dst[e] = src[e];
  }
  if (use_diag && tid < kMargMaxD) dinv[tid] = tid < D ? T(1) / as_global(a.dprior + reg * a.stridedp)[tid] : T(0);
  const T s_iso = (do_var && a.noise_kind == NOISE_ISOTROPIC) ? sg[0] : T(0);

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
    __syncthreads();  // (also: image and 1 / d in place)
    if (tile + a.ngroups < ntiles) prefetch(tile + a.ngroups);  // in flight during this tile's products
    const int n = n0 + row;
    const bool nok = n < N;
    T sv = s_iso;
    if (do_var && a.noise_kind == NOISE_DIAGONAL) sv = nok ? sg[n] : T(0);
    const T* const xr = Xs + row * LDX;

    // mean' = M'X_tile' (:33 per column): acc[v] = column c0 + crow(lane, v) at input n
    if (do_mean) {
      acc4 acc = {T(0), T(0), T(0), T(0)};
#pragma unroll
      for (int ks = 0; ks < 32; ++ks)
        if (ks < NK) acc = Mf::mma(mf[ks], xr[4 * ks + g], acc);
      T* const out = a.mean + reg * a.stridemean + n;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int c = Mf::crow(lane, v);
        if (nok && c < ncols) out[(int64_t)(c0 + c) * a.ldmean] = acc[v];
      }
    }
    // var_n = |L^-1 x_n|^2 + s_n (:40-43)
    if (use_img) {
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
      if (g == 0 && nok) a.var[reg * a.stridevar + n] = sq + sv;
    } else if (use_diag) {  // diagonal precision: var_n = sum_d x_dn^2 / d_d; the four lane groups take d = g (mod 4)
      T sq = T(0);
      for (int d = g; d < DP; d += 4) sq += xr[d] * xr[d] * dinv[d];
      sq += __shfl_xor(sq, 16, 64);
      sq += __shfl_xor(sq, 32, 64);
      if (g == 0 && nok) a.var[reg * a.stridevar + n] = sq + sv;
    }
  }
}

// the instantiations the library uses, defined in blr_marg_multi.hip
extern template __global__ void marginals_cols_kernel<double, LAYOUT_COLVECS>(MargColsArgs<double>);
extern template __global__ void marginals_cols_kernel<double, LAYOUT_ROWVECS>(MargColsArgs<double>);
extern template __global__ void marginals_cols_kernel<float, LAYOUT_COLVECS>(MargColsArgs<float>);
extern template __global__ void marginals_cols_kernel<float, LAYOUT_ROWVECS>(MargColsArgs<float>);

}  // namespace blr
