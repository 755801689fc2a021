// Exact leave-fold-out (K-fold) predictives of the observations a posterior state contains (blr_kfold_batched_*).
// Folds are contiguous blocks of F <= 64 observations.  With A = T'T the precision given all the data, z_n = T^-T x_n, q_n = 1 / sqrt(s_n)
// and r_n = y_n - x_n'mw, for one fold with rows Z_f:
//   G~ = I - diag(q) Z_f Z_f' diag(q) = L L'      (n_f x n_f; positive definite iff the state really contains the fold)
//   u  = L^-1 (q .* r),  g = L^-T u
//   kf_mean_n = y_n - sqrt(s_n) g_n,   kf_var_n = s_n |L^-1 e_n|^2,
//   kf_logpdf_f = -1/2 [n_f log 2 pi + sum log s_n - 2 sum log L_ii + |u|^2]        (the JOINT density of the fold)
// At F = 1 this is blr_loo.hpp: G~ = 1 - h_n.  The rows Z and the means x_n'mw come from cov_whiten_kernel (blr_cov_batched.hpp), which
// reads X once and keeps both in handle workspace.
//
// kfold_kernel: grid (fold packs, regressors), 256 threads; the pack body is kfold_pack, shared with blr_kfold_ragged.hpp.  A workgroup takes P = floor(64 / F) consecutive folds, at most 64 rows of Z:
//   1. the rows into an LDS tile as cov_tiles_kernel stages Z_j (rows past the pack or past N are zeros), the 64 x 64 product on the
//      matrix cores with k = d ascending: wave w owns rows 16 w .. 16 w + 15, its A fragments in registers;
//   2. G~ in double into LDS, 64 rows of 65 doubles -- the row stride is odd in doubles, so the 64 lanes of a column access (lane = row)
//      fall into 64 distinct bank pairs.  The block REUSES the tile's bytes (one barrier): 33 KB + 2.5 KB of vectors per workgroup
//      whatever D, never less than the tile;
//   3. a right-looking Cholesky, all folds of the pack in lockstep over the fold-local column k, ONE barrier per column: thread
//      (row r = lane, wave w) owns the elements (r, c), c = w mod 4, of its row's fold in registers.  In step k every thread reads the
//      pivot G[k][k] (final since the step before) and forms 1 / L_kk itself; nothing is scaled in place, so no thread writes what
//      another reads in the same step.  The same sweep carries the forward substitution of the identity: an element (r, c) is an entry
//      of the Schur complement while c > k and becomes V[r][c], L^-1 = diag(1 / L_ii) (I + V), from step k = c on.  V is kept
//      TRANSPOSED in the strictly upper triangle of the same block, which makes the read of the step -- G[c][k] for c > k, V[k][c] for
//      c < k -- one address expression;
//   4. the epilogue from L^-1 alone (wave 0, one thread per row): u, g, the column norms, the terms of the log density; the fold's
//      first row sums its fold's terms in order.
// Every index of steps 3 and 4 is bounded to the fold's own rows and columns [lo, hi): a cross-fold entry of the block is written by
// step 2 and never read, and nothing is masked by a multiplication with zero -- a NaN pivot of one fold cannot reach its neighbours.
// Every sum runs over fold-local indices in a fixed order: the bits of a fold depend neither on N, on the other folds, on where the
// fold lands in its workgroup nor on which outputs are wanted (L^-1 is always formed).
// D > 128 (correct, not fast): the fold's block comes from a staging covariance C = Z Z' + diag(s) of blr_mean_and_cov_* instead of
// the product: G~_ij = 2 delta_ij - C_ij q_i q_j.
// Totals: loo_total_kernel (blr_loo.hpp) over the folds' log densities.
#pragma once
#include "blr_common.hpp"
#include "blr_loo.hpp"
#include "blr_cov_batched.hpp"

namespace blr {

constexpr int kFoldMax = 64;         // largest fold: one 64 x 64 block per workgroup
constexpr int kFoldLdg = kFoldMax + 1;  // row stride of the double block

template <typename T>
struct KfoldArgs {
  const T* Z; int64_t strideZ;       // rows of DP elements (cov_whiten_kernel), strideZ elements per regressor, the launch's first regressor first
  const T* C; int64_t ldc;           // non-NULL: ONE regressor's N x N covariance Z Z' + diag(s) instead of Z (D > 128)
  const T* m; int64_t stridem;       // x_n'mw, indexed by the global regressor
  const T* y; int64_t stridey;
  const T* s; int64_t strides; int noise_kind;
  const int32_t* info;               // [B] status of loo_check_kernel: a regressor with info != 0 is skipped
  T* km; int64_t stride_km;          // [N] per regressor (may be NULL)
  T* kv; int64_t stride_kv;          // [N] per regressor (may be NULL)
  double* kl; int64_t stride_kl;     // [nfolds] per regressor (may be NULL)
  unsigned long long* degenerate;    // folds whose Cholesky met a pivot <= 0 or not finite (blr_get_stat "kfold_degenerate")
  int D, N, F;
  int reg0;                          // first regressor of this launch (grid.y <= 65535)
};

// dynamic LDS: the tile of Z (product route), then reused by the double block; five vectors of 64 doubles behind it
inline size_t kfold_lds_bytes(size_t elem, int D) {
  const size_t tile = cov_tiles_lds_bytes(elem, D), block = (size_t)kFoldMax * kFoldLdg * sizeof(double);
  return (tile > block ? tile : block) + (size_t)5 * kFoldMax * sizeof(double);
}

// One pack of folds: steps 1-4 above for `nrows` <= 64 rows that start at observation `row0` of ONE regressor.  Every per-observation
// pointer is the regressor's first element of the caller's array (formed once by the caller: no offset is carried along), so the equal-count kernel (strides) and the
// ragged one (blr_kfold_ragged.hpp: packed slices) run the same instructions on the same operands: the bits of a fold are the same.
template <typename T>
struct KfoldPack {
  const BLR_GLOBAL T* Zg;            // row row0 of the regressor's Z, rows of DP elements (product route; unused with C)
  const T* C; int64_t ldc;           // non-NULL: the regressor's N x N covariance instead of Z (D > 128)
  const BLR_GLOBAL T* yg;            // the regressor's targets
  const BLR_GLOBAL T* sg; bool diag;  // its noise: s[n], or one value
  const BLR_GLOBAL T* mg;            // its x_n'mw
  T* km; T* kv;                      // outputs (may be NULL): the regressor's first element of each
  double* kl;                        // (by folds)
  unsigned long long* degenerate;
  int D, F, row0, nrows;
};

template <typename T>
__device__ __forceinline__ void kfold_pack(char* smem, const KfoldPack<T>& a) {
  using Mf = Mfma<T>;
  using acc4 = typename Mf::acc4;
  constexpr int TN = kFoldMax, VEC = Mf::VEC, LDG = kFoldLdg;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int F = a.F;
  const int row0 = a.row0, nrows = a.nrows;
  const int NB = (a.D + 15) / 16, DP = 16 * NB, NK = DP / 4, LDZ = cov_ldz<T>(DP);
  const bool from_cov = a.C != nullptr;

  const size_t tile_bytes = (size_t)TN * LDZ * sizeof(T), block_bytes = (size_t)TN * LDG * sizeof(double);
  T* const Zs = reinterpret_cast<T*>(smem);             // [TN][LDZ]
  double* const Gs = reinterpret_cast<double*>(smem);   // [TN][LDG], after the product
  double* const qs = reinterpret_cast<double*>(smem + (!from_cov && tile_bytes > block_bytes ? tile_bytes : block_bytes));
  double* const bs = qs + TN;    // q_n r_n
  double* const rds = bs + TN;   // 1 / L_ii
  double* const us = rds + TN;   // u
  double* const ts = us + TN;    // log s_n + 2 log(1 / L_nn) + u_n^2

  const BLR_GLOBAL T* const yg = a.yg;
  const BLR_GLOBAL T* const sg = a.sg;
  const bool diag = a.diag;

  // ---- 1. the product Z_p Z_p' (rows row0 .. row0 + nrows - 1; the others are zeros) ----
  acc4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = acc4{T(0), T(0), T(0), T(0)};
  if (!from_cov) {
    const BLR_GLOBAL T* const Zg = a.Zg;
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
  // per row: q_n and q_n r_n in double (rows not in use: never read)
  if (tid < TN && tid < nrows) {
    const int n = row0 + tid;
    const double sv = (double)(diag ? sg[n] : sg[0]);
    const double q = 1.0 / sqrt(sv);
    qs[tid] = q;
    bs[tid] = q * ((double)yg[n] - (double)a.mg[n]);
  }
  __syncthreads();  // every wave is done with the tile: the block takes its bytes; q in place

  // ---- 2. G~ = I - diag(q) Z Z' diag(q), lower triangle of the rows in use ----
  if (!from_cov) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = 16 * c + li;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = 16 * wave + Mf::crow(lane, v);
        if (col <= r && r < nrows) Gs[r * LDG + col] = (r == col ? 1.0 : 0.0) - (qs[r] * qs[col]) * (double)acc[c][v];
      }
    }
  } else {
    const BLR_GLOBAL T* const Cg = as_global(a.C);
    for (int e = tid; e < TN * TN; e += kThreads) {
      const int r = e & (TN - 1), col = e >> 6;
      if (col <= r && r < nrows)
        Gs[r * LDG + col] = (r == col ? 2.0 : 0.0) - (qs[r] * qs[col]) * (double)Cg[(int64_t)(row0 + r) + (int64_t)(row0 + col) * a.ldc];
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

  // ---- 4. epilogue: wave 0, one thread per row (the other waves only keep the barriers) ----
  const bool mine = wave == 0 && rowok;
  const int n = row0 + r;
  double sv = 1.0, yv = 0.0;
  if (mine) {
    sv = (double)(diag ? sg[n] : sg[0]);
    yv = (double)yg[n];
    rds[r] = myrd;
    double ui = bs[r];
    for (int c = lo; c < r; ++c) ui = fused_madd(Gs[c * LDG + r], bs[c], ui);  // (I + V) (q .* r), row r
    ui *= myrd;
    us[r] = ui;
    ts[r] = log(sv) + 2.0 * log(myrd) + ui * ui;
  }
  __syncthreads();
  int ndeg = 0;
  if (mine) {
    const double kNan = __builtin_nan("");
    double gi = myrd * us[r], cn = myrd * myrd;  // column r of L^-1 = diag(1 / L_ii) (I + V): its product with u, its norm
    for (int i = r + 1; i < hi; ++i) {
      const double w = Gs[r * LDG + i] * rds[i];
      gi = fused_madd(w, us[i], gi);
      cn = fused_madd(w, w, cn);
    }
    if (a.km) a.km[n] = bad ? (T)kNan : (T)(yv - sqrt(sv) * gi);
    if (a.kv) a.kv[n] = bad ? (T)kNan : (T)(sv * cn);
    if (r == lo) {  // the fold's first row: its joint log density
      const double kLog2Pi = 1.8378770664093454835606594728112;
      double sum = 0.0;
      for (int i = lo; i < hi; ++i) sum += ts[i];
      if (a.kl) a.kl[(row0 + lo) / F] = bad ? kNan : -0.5 * ((double)(hi - lo) * kLog2Pi + sum);
      ndeg = bad ? 1 : 0;
    }
  }
  if (wave == 0) loo_count(ndeg, a.degenerate);  // (all 64 lanes)
}

template <typename T>
__global__ __launch_bounds__(kThreads, 2) void kfold_kernel(KfoldArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  if (a.info[reg] != 0) return;  // (block-uniform) outputs untouched
  const int PF = (kFoldMax / a.F) * a.F;        // rows of a full pack: floor(64 / F) folds
  const int row0 = (int)blockIdx.x * PF;        // first observation of this pack (< N: the grid has ceil(N / PF) packs)
  const int DP = 16 * ((a.D + 15) / 16);
  KfoldPack<T> p;
  p.Zg = as_global(a.Z + (int64_t)blockIdx.y * a.strideZ + (int64_t)row0 * DP);
  p.C = a.C; p.ldc = a.ldc;
  p.yg = as_global(a.y + reg * a.stridey);
  p.sg = as_global(a.s + reg * a.strides); p.diag = a.noise_kind == NOISE_DIAGONAL;
  p.mg = as_global(a.m + reg * a.stridem);
  p.km = a.km ? a.km + reg * a.stride_km : nullptr;
  p.kv = a.kv ? a.kv + reg * a.stride_kv : nullptr;
  p.kl = a.kl ? a.kl + reg * a.stride_kl : nullptr;
  p.degenerate = a.degenerate;
  p.D = a.D; p.F = a.F; p.row0 = row0; p.nrows = min(PF, a.N - row0);  // rows in use
  kfold_pack<T>(smem, p);
}

// the instantiations the library uses, defined in blr_kfold.hip
extern template __global__ void kfold_kernel<double>(KfoldArgs<double>);
extern template __global__ void kfold_kernel<float>(KfoldArgs<float>);

}  // namespace blr
