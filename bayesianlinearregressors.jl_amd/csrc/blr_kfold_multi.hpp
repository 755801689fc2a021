// Exact leave-fold-out (K-fold) predictives of a batched MULTI-OUTPUT state (blr_kfold_multi_batched_*): S target
// columns share one factor per regressor, so a fold's hat block, its Cholesky factor and L^-1 are formed once and only the residual
// depends on the column.  Folds are contiguous blocks of F <= 64 observations, D <= 128.  With z_n = T^-T x_n, q_n = 1 / sqrt(s_n):
//   once per fold    G~ = I - diag(q) Z_f Z_f' diag(q) = L L',   kf_var_n = s_n |L^-1 e_n|^2          (blr_kfold.hpp, steps 1-3)
//   per column c     r_nc = Y[n, c] - x_n'M[:, c],  u_c = L^-1 (q .* r_c),  g_c = L^-T u_c,
//                    kf_mean[n, c] = Y[n, c] - sqrt(s_n) g_nc,
//                    kf_logpdf[f, c] = -1/2 [n_f log 2 pi + sum log s_n - 2 sum log L_ii + |u_c|^2]
//
// kfold_whiten_cols_kernel: grid (tile groups, regressors), 256 threads.  cov_whiten_kernel's tile walk (blr_cov_batched.hpp) with
//   the column passes of loo_cols_kernel (blr_loo_multi.hpp): per tile of 64 inputs z' = (L^-T)'x from the image in LDS, STORED as
//   one row of DP = 16 ceil(D / 16) elements per input (cov_whiten_kernel's layout), then per pass of 16 columns of M the means
//   x_n'M[:, c] on the matrix cores from the same LDS rows, stored as [S][64 ceil(N / 64)] per regressor.  X is read once whatever S is.
//   The means come from X and M, not from z_n'(T M).
// kfold_cols_kernel: grid (fold packs, regressors), 256 threads.  Steps 1-3 are kfold_kernel's (a private copy: that kernel's code
//   object stays as it is), run ONCE per pack; L^-1 = diag(1 / L_ii) (I + V) then stays read-only in the 64 x 65 double block and
//   the epilogue loops over the columns: wave w takes the columns c = w (mod 4), lane = row, with its own copies of the b / u / term
//   vectors in LDS.  kf_var and the degenerate count are taken once per fold (wave 0).
// Every index of the Cholesky and of the epilogue is bounded to the fold's own rows and columns [lo, hi); nothing is masked by a
// multiplication with zero: a NaN in one column of Y stays in that column, a NaN pivot in its fold.  Every sum runs over fold-local
// indices in the order of kfold_kernel's epilogue and every wave runs the same instructions: the bits of a column depend neither on
// S, on its wave or pass nor on the other columns; those of kf_var not on S nor on which outputs are wanted.
// Totals: loo_cols_total_kernel (blr_loo_multi.hpp) over the nfolds x S log densities.
#pragma once
#include "blr_kfold.hpp"
#include "blr_loo_multi.hpp"

namespace blr {

constexpr int kKfoldColsPerPass = kLooColsPerPass;  // columns of M per pass of the whitening kernel
constexpr int kKfoldColWaves = kThreads / 64;       // columns in flight in the epilogue: one per wave

template <typename T>
struct KfoldWhitenArgs {
  const T* X; int64_t ldx, strideX;
  const T* M; int64_t ldm, strideM;   // D x S mean columns per regressor
  const T* img;                       // images of L^-T, IMG_ELEMS apart, the launch's first regressor first
  const int32_t* info;                // [B] status of loo_check_kernel: a regressor with info != 0 is skipped
  T* Z;                               // workspace: 64 ntiles rows of DP elements per regressor, the launch's first regressor first
  T* mean; int64_t ldmn;              // workspace: [S][ldmn] per regressor, the launch's first regressor first (NULL: no column output wanted)
  int D, N, S;
  int ngroups;                        // tile groups per regressor (= gridDim.x)
  int reg0;                           // first regressor of this launch (grid.y <= 65535)
};

// dynamic LDS of kfold_whiten_cols_kernel: the tile and the image's column blocks in use
inline size_t kfold_whiten_cols_lds_bytes(size_t elem, int D) {
  const int NB = (D + 15) / 16;
  return cov_tiles_lds_bytes(elem, D) + (size_t)2 * NB * (NB + 1) * 64 * elem;
}

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void kfold_whiten_cols_kernel(KfoldWhitenArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Mf = Mfma<T>;
  using G = MargGemmCfg<T>;
  using acc4 = typename Mf::acc4;
  constexpr int W = kKfoldColsPerPass, TN = kCovTile, VEC = Mf::VEC;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  if (a.info[reg] != 0) return;  // (block-uniform) the state failed the check: nothing of it is read later
  const int grp = blockIdx.x;
  const int D = a.D, N = a.N;
  const int NB = (D + 15) / 16, DP = 16 * NB, NK = DP / 4, LDX = cov_ldz<T>(DP);
  const int npasses = a.mean != nullptr ? (a.S + W - 1) / W : 0;

  T* const Xs = reinterpret_cast<T*>(smem);  // [TN][LDX]
  T* const img = Xs + TN * LDX;              // [2 NB (NB + 1)][64]

  const BLR_GLOBAL T* const Xg = as_global(a.X + reg * a.strideX);
  const BLR_GLOBAL T* const Mg = as_global(a.M + reg * a.strideM);
  const int ntiles = (N + TN - 1) / TN;
  BLR_GLOBAL T* const Zg = as_global(a.Z + (int64_t)blockIdx.y * ntiles * TN * DP);
  BLR_GLOBAL T* const mg = npasses ? as_global(a.mean + (int64_t)blockIdx.y * a.S * a.ldmn) : nullptr;

  // ---- the tile through registers, as cov_whiten_kernel stages it ----
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
    const T* const xr = Xs + row * LDX;

    // z_n = L^-1 x_n, kept: row n0 + row of the regressor's Z (rows n >= N are zeros, as the tile is)
    {
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
    }
    __builtin_amdgcn_sched_barrier(0);

    // mean' = M'X_tile' per pass: acc[v] = column c0 + crow(lane, v) at input n, stored along n
    for (int pass = 0; pass < npasses; ++pass) {
      const int c0 = pass * W;
      if (npasses > 1) load_fragments(c0);
      acc4 acc = {T(0), T(0), T(0), T(0)};
#pragma unroll
      for (int ks = 0; ks < 32; ++ks)
        if (ks < NK) acc = Mf::mma(mf[ks], xr[4 * ks + g], acc);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int c = c0 + Mf::crow(lane, v);
        if (n < N && c < a.S) mg[(int64_t)c * a.ldmn + n] = acc[v];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <typename T>
struct KfoldColsArgs {
  const T* Z; int64_t strideZ;               // rows of DP elements, strideZ elements per regressor, the launch's first regressor first
  const T* mean; int64_t ldmn;               // x_n'M[:, c]: [S][ldmn] per regressor, the launch's first regressor first
  const T* Y; int64_t ldY, strideY;          // N x S targets per regressor
  const T* s; int64_t strides; int noise_kind;
  const int32_t* info;                       // [B] status of loo_check_kernel: a regressor with info != 0 is skipped
  T* km; int64_t ld_km, stride_km;           // N x S per regressor (may be NULL)
  T* kv; int64_t stride_kv;                  // [N] per regressor (may be NULL)
  double* kl; int64_t ld_kl, stride_kl;      // nfolds x S per regressor (may be NULL)
  unsigned long long* degenerate;            // folds whose Cholesky met a pivot <= 0 or not finite, counted once whatever S is
  int D, N, F, S;
  int reg0;                                  // first regressor of this launch (grid.y <= 65535)
};

// dynamic LDS: the tile of Z, reused by the double block; behind it q, 1 / L_ii and per wave the three column vectors of 64 doubles
inline size_t kfold_cols_lds_bytes(size_t elem, int D) {
  const size_t tile = cov_tiles_lds_bytes(elem, D), block = (size_t)kFoldMax * kFoldLdg * sizeof(double);
  return (tile > block ? tile : block) + (size_t)(2 + 3 * kKfoldColWaves) * kFoldMax * sizeof(double);
}

template <typename T>
__global__ __launch_bounds__(kThreads, 2) void kfold_cols_kernel(KfoldColsArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Mf = Mfma<T>;
  using acc4 = typename Mf::acc4;
  constexpr int TN = kFoldMax, VEC = Mf::VEC, LDG = kFoldLdg;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  if (a.info[reg] != 0) return;  // (block-uniform) outputs untouched
  const int N = a.N, F = a.F;
  const int P = TN / F, PF = P * F;             // folds and rows of a full pack
  const int row0 = (int)blockIdx.x * PF;        // first observation of this pack (< N: the grid has ceil(N / PF) packs)
  const int nrows = min(PF, N - row0);          // rows in use
  const int NB = (a.D + 15) / 16, DP = 16 * NB, NK = DP / 4, LDZ = cov_ldz<T>(DP);

  const size_t tile_bytes = (size_t)TN * LDZ * sizeof(T), block_bytes = (size_t)TN * LDG * sizeof(double);
  T* const Zs = reinterpret_cast<T*>(smem);             // [TN][LDZ]
  double* const Gs = reinterpret_cast<double*>(smem);   // [TN][LDG], after the product
  double* const qs = reinterpret_cast<double*>(smem + (tile_bytes > block_bytes ? tile_bytes : block_bytes));
  double* const rds = qs + TN;                          // 1 / L_ii
  double* const bs = rds + TN + (size_t)3 * TN * wave;  // this wave's q_n r_nc
  double* const us = bs + TN;                           // ... u_c
  double* const ts = us + TN;                           // ... log s_n + 2 log(1 / L_nn) + u_nc^2

  const BLR_GLOBAL T* const sg = as_global(a.s + reg * a.strides);
  const bool diag = a.noise_kind == NOISE_DIAGONAL;

  // ---- 1. the product Z_p Z_p' (rows row0 .. row0 + nrows - 1; the others are zeros) ----
  acc4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = acc4{T(0), T(0), T(0), T(0)};
  {
    const BLR_GLOBAL T* const Zg = as_global(a.Z + (int64_t)blockIdx.y * a.strideZ + (int64_t)row0 * DP);
    {
      const BLR_GLOBAL vecT* const src = reinterpret_cast<const BLR_GLOBAL vecT*>(Zg);
      const int nv = DP / VEC;
      vecT zero;
#pragma unroll
      for (int v = 0; v < VEC; ++v) zero[v] = T(0);
      for (int e = tid; e < TN * nv; e += kThreads) {
        const int r = e / nv, c = e - r * nv;
        *reinterpret_cast<vecT*>(Zs + r * LDZ + c * VEC) = r < nrows ? src[e] : zero;
      }
    }
    T zf[32];
    {
      const int ar = 16 * wave + li;
      const BLR_GLOBAL T* const zr = Zg + (int64_t)ar * DP + g;
#pragma unroll
      for (int ks = 0; ks < 32; ++ks) zf[ks] = (ks < NK && ar < nrows) ? zr[4 * ks] : T(0);
    }
    __syncthreads();
    const T* const zb = Zs + li * LDZ + g;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
      if (ks < NK) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = Mf::mma(zf[ks], zb[16 * c * LDZ + 4 * ks], acc[c]);
      }
    }
  }
  // per row: q_n in double (rows not in use: never read)
  if (tid < TN && tid < nrows) qs[tid] = 1.0 / sqrt((double)(diag ? sg[row0 + tid] : sg[0]));
  __syncthreads();  // every wave is done with the tile: the block takes its bytes; q in place

  // ---- 2. G~ = I - diag(q) Z Z' diag(q), lower triangle of the rows in use ----
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = 16 * c + li;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = 16 * wave + Mf::crow(lane, v);
      if (col <= r && r < nrows) Gs[r * LDG + col] = (r == col ? 1.0 : 0.0) - (qs[r] * qs[col]) * (double)acc[c][v];
    }
  }
  __syncthreads();

  // ---- 3. Cholesky and L^-1, the folds of the pack in lockstep; this thread: row r of the fold [lo, hi), columns c = wave mod 4 ----
  const int r = lane;
  const int lo = (r / F) * F, hi = min(lo + F, nrows);
  const bool rowok = r < nrows;
  double el[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int c = 4 * t + wave;
    el[t] = (rowok && c >= lo && c <= r) ? Gs[r * LDG + c] : 0.0;
  }
  bool bad = false;
  double myrd = 0.0;
  const int kmax = min(F, nrows);
  for (int k = 0; k < kmax; ++k) {
    const int kc = lo + k;
    if (rowok && !bad && kc < hi) {
      const double piv = Gs[kc * LDG + kc];
      if (!(piv > 0.0) || !isfinite(piv)) {
        bad = true;  // (every thread of the fold sees the same pivot)
      } else {
        const double rinv = 1.0 / sqrt(piv);
        if (r == kc) myrd = rinv;
        if (r > kc) {
          const double lr = Gs[r * LDG + kc] * rinv;  // L[r][k]
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const int c = 4 * t + wave;
            if (c >= lo && c <= r) {
              if (c == kc) {
                el[t] = -lr * rinv;  // V[r][k] starts: -L[r][k] / L[k][k]
                Gs[c * LDG + r] = el[t];
              } else {
                const double x = Gs[c * LDG + kc] * rinv;  // c > k: L[c][k]; c < k: V[k][c] / L[k][k]
                el[t] = fused_madd(-lr, x, el[t]);
                Gs[c > kc ? r * LDG + c : c * LDG + r] = el[t];
              }
            }
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- 4. epilogue.  Every wave knows 1 / L_rr and the fold's status of its row r = lane (step 3 ran in all four) ----
  const int n = row0 + r;
  const double kNan = __builtin_nan("");
  const double kLog2Pi = 1.8378770664093454835606594728112;
  const double sv = rowok ? (double)(diag ? sg[n] : sg[0]) : 1.0;
  if (wave == 0 && rowok) rds[r] = myrd;
  __syncthreads();
  // once per fold: the variances and the count (wave 0, one thread per row)
  int ndeg = 0;
  if (wave == 0 && rowok) {
    double cn = myrd * myrd;  // column r of L^-1 = diag(1 / L_ii) (I + V): its norm
    for (int i = r + 1; i < hi; ++i) {
      const double w = Gs[r * LDG + i] * rds[i];
      cn = fused_madd(w, w, cn);
    }
    if (a.kv) a.kv[reg * a.stride_kv + n] = bad ? (T)kNan : (T)(sv * cn);
    if (r == lo) ndeg = bad ? 1 : 0;
  }
  if (wave == 0) loo_count(ndeg, a.degenerate);  // (all 64 lanes)
  if (a.km == nullptr && a.kl == nullptr) return;  // (block-uniform)

  // per column: wave w takes c = w, w + 4, ...; the trip count is the same in every wave (the barriers), a wave past S idles
  const double lterm = rowok ? log(sv) + 2.0 * log(myrd) : 0.0;
  const double sq = sqrt(sv);
  const BLR_GLOBAL T* const Yg = as_global(a.Y + reg * a.strideY);
  const BLR_GLOBAL T* const mg = as_global(a.mean + (int64_t)blockIdx.y * a.S * a.ldmn);
  const int ntrips = (a.S + kKfoldColWaves - 1) / kKfoldColWaves;
  for (int trip = 0; trip < ntrips; ++trip) {
    const int c = kKfoldColWaves * trip + wave;
    const bool mine = rowok && c < a.S;
    double yv = 0.0;
    if (mine) {
      yv = (double)Yg[(int64_t)c * a.ldY + n];
      bs[r] = qs[r] * (yv - (double)mg[(int64_t)c * a.ldmn + n]);
    }
    __syncthreads();
    if (mine) {
      double ui = bs[r];
      for (int j = lo; j < r; ++j) ui = fused_madd(Gs[j * LDG + r], bs[j], ui);  // (I + V) (q .* r_c), row r
      ui *= myrd;
      us[r] = ui;
      ts[r] = lterm + ui * ui;
    }
    __syncthreads();
    if (mine) {
      double gi = myrd * us[r];  // column r of L^-1 times u_c
      for (int i = r + 1; i < hi; ++i) gi = fused_madd(Gs[r * LDG + i] * rds[i], us[i], gi);
      if (a.km) a.km[reg * a.stride_km + (int64_t)c * a.ld_km + n] = bad ? (T)kNan : (T)(yv - sq * gi);
      if (r == lo && a.kl) {  // the fold's first row: its joint log density
        double sum = 0.0;
        for (int i = lo; i < hi; ++i) sum += ts[i];
        a.kl[reg * a.stride_kl + (int64_t)c * a.ld_kl + (row0 + lo) / F] = bad ? kNan : -0.5 * ((double)(hi - lo) * kLog2Pi + sum);
      }
    }
    // (the next trip's first write goes to bs, last read before the barrier above; us and ts are this wave's own)
  }
}

// the instantiations the library uses, defined in blr_kfold_multi.hip
extern template __global__ void kfold_whiten_cols_kernel<double, LAYOUT_COLVECS>(KfoldWhitenArgs<double>);
extern template __global__ void kfold_whiten_cols_kernel<double, LAYOUT_ROWVECS>(KfoldWhitenArgs<double>);
extern template __global__ void kfold_whiten_cols_kernel<float, LAYOUT_COLVECS>(KfoldWhitenArgs<float>);
extern template __global__ void kfold_whiten_cols_kernel<float, LAYOUT_ROWVECS>(KfoldWhitenArgs<float>);
extern template __global__ void kfold_cols_kernel<double>(KfoldColsArgs<double>);
extern template __global__ void kfold_cols_kernel<float>(KfoldColsArgs<float>);

}  // namespace blr
