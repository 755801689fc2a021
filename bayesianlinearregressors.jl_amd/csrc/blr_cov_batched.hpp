// Joint predictive covariance of a batch of regressors (blr_mean_and_cov_batched_*, DESIGN.md K21, D <= 128):
//   mean_b = X_b' mw_b                                  (reference src/bayesian_linear_regression.jl:33)
//   C_b    = X_b' Lw_b^-1 X_b + Sigma_y = Z_b Z_b' + Sigma_y,  z_n = U_b^-T x_n   (:35-38, :45)
// Replaces a loop of blr_mean_and_cov_* calls (one launch chain, one drain and one set of temporaries per regressor) by two launches
// per chunk of regressors, after the status and the triangular inverses (marg_image_kernel) of the chunk:
//
// cov_whiten_kernel: grid (tile groups, regressors), 256 threads.  The tile walk of marginals_cols_kernel (blr_marg_multi.hpp): 64
//   inputs through registers into the rows of an LDS block, one code path for both layouts, the next tile's loads in flight.  Per tile
//     z'     = (L^-T)' x, column block by column block from the image in LDS (a diagonal prior: x_d / sqrt(d_d)); where the marginals
//              throw z away after |z|^2, here it is STORED: one row of DP = 16 ceil(D / 16) contiguous elements per input, the rows of
//              a regressor one after the other (the padding rows and columns are zeros: the tile is zero there);
//     mean_n = x_n' mw from the same LDS rows (the four lane groups take d = g mod 4, then a fixed two-step butterfly).
//   X is read once and Z is formed once per input.
// cov_tiles_kernel: grid (tile pairs i <= j, regressors), 256 threads.  The 64 x 64 block Z_i Z_j' on v_mfma_f64_16x16x4 /
//   v_mfma_f32_16x16x4, k = d ascending: Z_j (64 contiguous rows of the workspace) goes into LDS with 16-byte loads and is the B operand
//   of all four waves; wave w keeps the A fragments of its rows 16 w .. 16 w + 15 of Z_i in REGISTERS, loaded straight from the Z rows
//   (as mf[] in marginals_cols_kernel).  One tile in LDS, not two: 66.5 KB in fp64 at D = 128, two workgroups per CU.  The noise term is
//   added at the store, and block (i, j) and its transpose (j, i) are stored from the same accumulators; of a diagonal tile only the
//   entries r <= c are used, each stored to (r, c) and (c, r): C is symmetric bit for bit whatever the matrix core's rounding.
// Every sum has a fixed order, nothing is atomic, and an accumulator entry depends on its own two Z rows only: the bits of a regressor
// depend neither on B, on its position, on the chunking nor on whether the mean is wanted.
#pragma once
#include "blr_common.hpp"
#include "blr_marg_image.hpp"

namespace blr {

constexpr int kCovTile = 64;   // inputs per tile: one 16-input MFMA tile per wave
constexpr int kCovMaxD = kPB;  // the image of L^-T (MargGemmCfg, written by marg_image_kernel) covers one 128-block

template <typename T>
struct CovArgs {
  const T* X; int64_t ldx, strideX;
  const T* s; int64_t lds, strides;    // one variance, s[N], or the upper triangle of an N x N Sigma_y (lds >= N)
  const T* mw; int64_t stridemw;
  const T* dprior; int64_t stridedp;   // PRIOR_DIAGONAL: the diagonal of the precision
  const T* img;                        // PRIOR_UPPER_FACTOR: images of L^-T, IMG_ELEMS apart, the launch's first regressor first
  const int32_t* info;                 // [B] status, written by the launch before: a regressor with info != 0 is skipped
  T* mean; int64_t stridemean;         // may be NULL
  T* C; int64_t ldc, strideC;
  T* Z;                                // workspace: 64 ntiles rows of DP elements per regressor, the launch's first regressor first
  int noise_kind, prior_kind, D, N;
  int ngroups;                         // tile groups per regressor (cov_whiten_kernel)
  int reg0;                            // first regressor of this launch (grid.y <= 65535)
};

// row stride of an LDS tile: 16 bytes over the padded width (blr_marg_multi.hpp: the B operand of lane (i, g) -- row i, column
// 4 ks + g -- then falls into distinct banks for each lane group of an LDS access)
template <typename T>
__host__ __device__ constexpr int cov_ldz(int DP) { return DP + 16 / (int)sizeof(T); }

// elements of Z per regressor
inline size_t cov_z_elems(int D, int N) {
  const size_t DP = (size_t)16 * (((size_t)D + 15) / 16), ntiles = ((size_t)N + kCovTile - 1) / kCovTile;
  return ntiles * kCovTile * DP;
}

// dynamic LDS of cov_whiten_kernel: the tile, mw, 1 / sqrt(d) of a diagonal prior, and the image's column blocks in use
inline size_t cov_whiten_lds_bytes(size_t elem, int D, bool with_image) {
  const int NB = (D + 15) / 16, DP = 16 * NB;
  const size_t tile = (size_t)kCovTile * (size_t)(DP + 16 / (int)elem) * elem;
  return tile + (size_t)2 * kCovMaxD * elem + (with_image ? (size_t)2 * NB * (NB + 1) * 64 * elem : 0);
}
// of cov_tiles_kernel: the tile Z_j
inline size_t cov_tiles_lds_bytes(size_t elem, int D) {
  const int DP = 16 * ((D + 15) / 16);
  return (size_t)kCovTile * (size_t)(DP + 16 / (int)elem) * elem;
}

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void cov_whiten_kernel(CovArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Mf = Mfma<T>;
  using G = MargGemmCfg<T>;
  using acc4 = typename Mf::acc4;
  constexpr int TN = kCovTile, VEC = Mf::VEC;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  if (a.info[reg] != 0) return;  // (block-uniform) the prior is not positive definite: outputs untouched
  const int grp = blockIdx.x;
  const int D = a.D, N = a.N;
  const int NB = (D + 15) / 16, DP = 16 * NB, LDX = cov_ldz<T>(DP);
  const bool do_mean = a.mean != nullptr;
  const bool do_z = a.Z != nullptr;
  const bool use_img = do_z && a.prior_kind == PRIOR_UPPER_FACTOR;
  const bool use_diag = do_z && a.prior_kind == PRIOR_DIAGONAL;

  T* const Xs = reinterpret_cast<T*>(smem);  // [TN][LDX]
  T* const mws = Xs + TN * LDX;              // [128]
  T* const dsc = mws + kCovMaxD;             // [128]
  T* const img = dsc + kCovMaxD;             // [2 NB (NB + 1)][64]

  const BLR_GLOBAL T* const Xg = as_global(a.X + reg * a.strideX);
  const int ntiles = (N + TN - 1) / TN;
  BLR_GLOBAL T* const Zg = do_z ? as_global(a.Z + (int64_t)blockIdx.y * ntiles * TN * DP) : nullptr;

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
  if (use_img) {
    const BLR_GLOBAL vecT* const src = reinterpret_cast<const BLR_GLOBAL vecT*>(as_global(a.img + (int64_t)blockIdx.y * G::IMG_ELEMS));
    vecT* const dst = reinterpret_cast<vecT*>(img);
    const int nvec = G::frag0(NB) * 64 / VEC;
    for (int e = tid; e < nvec; e += kThreads) dst[e] = src[e];
  }
  if (tid < kCovMaxD) {
    mws[tid] = (do_mean && tid < D) ? as_global(a.mw + reg * a.stridemw)[tid] : T(0);
    dsc[tid] = (use_diag && tid < D) ? T(1) / sqrt(as_global(a.dprior + reg * a.stridedp)[tid]) : T(0);
  }

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
    __syncthreads();  // (also: image, mw and 1 / sqrt(d) in place)
    if (tile + a.ngroups < ntiles) prefetch(tile + a.ngroups);  // in flight during this tile's products
    const int n = n0 + row;
    const T* const xr = Xs + row * LDX;

    // mean_n = x_n' mw (:33)
    if (do_mean) {
      T m = T(0);
      for (int d = g; d < DP; d += 4) m = fused_madd(xr[d], mws[d], m);
      m += __shfl_xor(m, 16, 64);
      m += __shfl_xor(m, 32, 64);
      if (g == 0 && n < N) a.mean[reg * a.stridemean + n] = m;
    }
    // z_n = L^-1 x_n (:36 alpha = Uw' \ X), kept: row n0 + row of the regressor's Z (rows n >= N are zeros, as the tile is)
    if (use_img) {
      BLR_GLOBAL T* const zr = Zg + (int64_t)(n0 + row) * DP;
#pragma unroll 1
      for (int J = 0; J < NB; ++J) {
        acc4 acc = {T(0), T(0), T(0), T(0)};
        const T* const fb = img + G::frag0(J) * 64 + lane;
#pragma unroll 4
        for (int m = 0; m < 4 * (J + 1); ++m) acc = Mf::mma(fb[m * 64], xr[G::d_of(m, g)], acc);
#pragma unroll
        for (int v = 0; v < 4; ++v) zr[16 * J + Mf::crow(lane, v)] = acc[v];
      }
    } else if (use_diag) {  // diagonal precision: z_dn = x_dn / sqrt(d_d); stores along the rows of Z
      BLR_GLOBAL T* const zt = Zg + (int64_t)n0 * DP;
      for (int e = tid; e < TN * DP; e += kThreads) {
        const int r = e / DP, d = e - r * DP;
        zt[e] = Xs[r * LDX + d] * dsc[d];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads, 2) void cov_tiles_kernel(CovArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Mf = Mfma<T>;
  using acc4 = typename Mf::acc4;
  constexpr int TN = kCovTile, VEC = Mf::VEC;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  if (a.info[reg] != 0) return;  // (block-uniform) outputs untouched
  const int tj = tile_I((int)blockIdx.x), ti = (int)blockIdx.x - tj * (tj + 1) / 2;  // ti <= tj
  const int N = a.N;
  const int NB = (a.D + 15) / 16, DP = 16 * NB, NK = DP / 4, LDZ = cov_ldz<T>(DP);
  const int ntiles = (N + TN - 1) / TN;
  const BLR_GLOBAL T* const Zg = as_global(a.Z + (int64_t)blockIdx.y * ntiles * TN * DP);
  T* const Zs = reinterpret_cast<T*>(smem);  // [TN][LDZ]: tile tj

  // tile tj: 64 contiguous rows of the workspace into LDS rows
  {
    const BLR_GLOBAL vecT* const src = reinterpret_cast<const BLR_GLOBAL vecT*>(Zg + (int64_t)tj * TN * DP);
    const int nv = DP / VEC;
    for (int e = tid; e < TN * nv; e += kThreads) {
      const int r = e / nv, c = e - r * nv;
      *reinterpret_cast<vecT*>(Zs + r * LDZ + c * VEC) = src[e];
    }
  }
  // A fragments of this wave's rows of tile ti: zf[ks] = Z[64 ti + 16 wave + li, 4 ks + g]
  T zf[32];
  {
    const BLR_GLOBAL T* const zr = Zg + ((int64_t)ti * TN + 16 * wave + li) * DP + g;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) zf[ks] = ks < NK ? zr[4 * ks] : T(0);
  }
  __syncthreads();

  acc4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = acc4{T(0), T(0), T(0), T(0)};
  const T* const zb = Zs + li * LDZ + g;
#pragma unroll
  for (int ks = 0; ks < 32; ++ks) {
    if (ks < NK) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = Mf::mma(zf[ks], zb[16 * c * LDZ + 4 * ks], acc[c]);
    }
  }

  // acc[c][v] = (Z_i Z_j')[16 wave + crow(lane, v), 16 c + li]: + Sigma_y, then to (r, c) and (c, r)
  const BLR_GLOBAL T* const sg = as_global(a.s + reg * a.strides);
  BLR_GLOBAL T* const Cg = as_global(a.C + reg * a.strideC);
  const T s_iso = a.noise_kind == NOISE_ISOTROPIC ? sg[0] : T(0);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = TN * tj + 16 * c + li;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = TN * ti + 16 * wave + Mf::crow(lane, v);
      if (r > col || col >= N) continue;  // (r <= col < N; a diagonal tile's lower half is the mirror of its upper half)
      T val = acc[c][v];
      if (a.noise_kind == NOISE_DENSE) val += sg[(int64_t)r + (int64_t)col * a.lds];
      else if (r == col) val += a.noise_kind == NOISE_DIAGONAL ? sg[r] : s_iso;
      Cg[(int64_t)r + (int64_t)col * a.ldc] = val;
      if (r != col) Cg[(int64_t)col + (int64_t)r * a.ldc] = val;
    }
  }
}

// the instantiations the library uses, defined in blr_cov_batched.hip
extern template __global__ void cov_whiten_kernel<double, LAYOUT_COLVECS>(CovArgs<double>);
extern template __global__ void cov_whiten_kernel<double, LAYOUT_ROWVECS>(CovArgs<double>);
extern template __global__ void cov_whiten_kernel<float, LAYOUT_COLVECS>(CovArgs<float>);
extern template __global__ void cov_whiten_kernel<float, LAYOUT_ROWVECS>(CovArgs<float>);
extern template __global__ void cov_tiles_kernel<double>(CovArgs<double>);
extern template __global__ void cov_tiles_kernel<float>(CovArgs<float>);

}  // namespace blr
