// Exact leave-fold-out (K-fold) predictives for LARGE folds (blr_kfold_large_batched_*): the fold is removed in WEIGHT
// space -- one D x D factorisation per fold from statistics gathered in one pass over X -- where blr_kfold.hpp (K23) works in
// observation space on the fold's n_f x n_f hat block and stops at 64 rows.  With the state (mw', T), A = T'T, r0_n = y_n - x_n'mw'
// and fold f = [f F, min((f + 1) F, N)) of n_f observations:
//   G_f = X_f S_f^-1 X_f'    d_f = X_f S_f^-1 r0    q_f = r0' S_f^-1 r0    l_f = sum log s_n        (phase_gram, no prior, mw = mw')
//   A_f = A - G_f = U_f'U_f       u_f = U_f^-T d_f       mw_f = mw' - U_f^-1 u_f
//   kf_mean_n = x_n'mw_f     kf_var_n = s_n + |U_f^-T x_n|^2
//   kf_logpdf[f] = -1/2 [n_f log 2 pi + l_f + logdet A - logdet A_f + q_f + |u_f|^2]
// D <= 128.  Per chunk of regressors, whatever B and the fold count are:
//   kfl_state_kernel    one workgroup per regressor: A in phase_chol's packed layout (pidx, padded to SmallCfg::PACKED), in DOUBLE in
//                       both element types (A - G_f cancels: the difference is rounded once), and logdet A = 2 sum log T_ii to workspace
//   kfl_stats_kernel    one workgroup per (regressor, fold, column block): phase_gram of blr_fused_small.hpp on the block's slice of
//                       X, y, s -- grid_stats_kernel (blr_grid.hpp) pointed at a fold; its loaders come along unchanged (fp64)
//   kfl_stats32_kernel  the same grid in fp32: the float rows widened into LDS, G_f, d_f, q_f, l_f accumulated in double on the fp64
//                       matrix instruction (the statistics buffer is double in both element types)
//   kfl_reduce_kernel   the column blocks 1 .. of a fold added to block 0 in that order (only when a full fold has more than one)
//   kfl_factor_kernel   one workgroup per (regressor, fold): P = A - G_f and b = d_f in LDS, phase_chol with the riding forward
//                       substitution, phase_backsolve; U_f (upper, ld = D), mw_f and the fold's status to workspace, kf_logpdf[f]
//   marg_image_kernel   (blr_marginals.hpp) over the chunk's factors U_f
//   kfl_predict_kernel  (64-input tiles of a fold, fold, regressor): the tile walk of cov_whiten_kernel (blr_cov_batched.hpp) over
//                       the fold's rows with the fold's image and mw_f: z_n = U_f^-T x_n and x_n'mw_f on the matrix cores;
//                       kf_var_n = s_n + |z_n|^2 and kf_mean_n are stored, the rows are not
// X is read twice per call.  The column blocks of a fold follow from its own n_f alone (kfl_splits), every sum has a fixed order and
// nothing but the integer counter of degenerate folds is atomic: the bits of fold f depend on the regressor's T and mw and on the
// fold's own X, y, s and row count only.  phase_chol / phase_backsolve are instantiated with TAG = 2 and inlined into kfl_factor_kernel.
#pragma once
#include "blr_common.hpp"
#include "blr_fused_small.hpp"
#include "blr_loo.hpp"
#include "blr_cov_batched.hpp"
#include "blr_kfold_large_splits.hpp"

namespace blr {

constexpr int64_t kFoldLargeMaxFolds = 1024;  // ceil(N / F): few, large folds (many small ones belong to blr_kfold_batched_*)
// (blr_grid.hpp defines plain kernels and belongs to blr_abi.hip's unit alone: what this family shares with it is restated here)
constexpr int kKflPriorNone = 3;  // phase_gram: neither a precision nor a factor -- the accumulators start from zero (kGridPriorNone)
template <typename T, int NB>
constexpr int kfl_stat_elems() { return SmallCfg<T, NB>::PACKED + SmallCfg<T, NB>::DP; }  // G_f packed, then d_f
#define BLR_KFL_BOUNDS(T, NB) __launch_bounds__(kThreads, ((NB) <= 4 ? 4 : (sizeof(T) == 4 ? BLR_F32_WAVES_PER_SIMD : 2)))

template <typename T>
struct KflArgs {
  const T* X; int64_t ldx, strideX;
  const T* y; int64_t stridey;
  const T* s; int64_t strides;
  const T* mw; int64_t stridemw;
  const T* Tf; int64_t ldt, strideT;
  const int32_t* info;               // [B] status of loo_check_kernel: a regressor with info != 0 is skipped
  T* km; int64_t stride_km;          // [N] per regressor (may be NULL)
  T* kv; int64_t stride_kv;          // [N] per regressor (may be NULL)
  double* kl; int64_t stride_kl;     // [nfolds] per regressor (may be NULL)
  unsigned long long* degenerate;    // folds whose factorisation failed (blr_get_stat "kfold_degenerate")
  // workspace of one chunk, indexed by the chunk-local regressor r = reg - reg0 and the fold:
  double* A;                         // [r] PACKED doubles: T'T, packed lower triangle
  double* ldA;                       // [r] logdet A
  double* stats;                     // [r][fold][column block] PACKED + DP doubles: G_f, d_f
  double* scal;                      // [r][fold][column block] {q_f, l_f}
  T* U;                              // [r][fold] D x D: U_f, upper, ld = D
  T* mwf;                            // [r][fold] D elements: mw_f
  int32_t* finfo;                    // [r][fold] 0: U_f and mw_f are valid; else the fold is skipped (bad regressor) or NaN (bad pivot)
  const T* img;                      // [r][fold] images of U_f^-T (marg_image_kernel)
  int layout, noise_kind;
  int D, N, F, nfolds;               // F <= N here (a fold size beyond N is one fold of N)
  int S;                             // column-block slots per fold: kfl_splits of a full fold
  int ngroups;                       // tile groups per fold (kfl_predict_kernel)
  int reg0;                          // first regressor of this chunk
};

// What a body below needs of ONE fold -- the statistics: of one column block of it --: pointers at its first row, its row count, its
// slots.  The rectangular kernels (kfl_*) and the table-driven ones of the unequal-count form (kflr_*, blr_kfold_large_ragged.hpp) each
// fill one and run the same body: a fold has the same bits whichever grid it came from.
template <typename T>
struct KflFold {
  const T* X;                      // the first row of the fold (statistics: of the column block)
  const T* y;                      // likewise
  const T* s;                      // likewise under diagonal noise; else the regressor's value
  const T* mw;                     // the state's mean
  int64_t ldx;
  int D, n, noise_kind;            // n: rows of the fold (statistics: of the column block)
  double* stats;                   // PACKED + DP doubles: the block's slot (factor: the fold's block 0, reduced)
  double* scal;                    // {q_f, l_f} of that slot
  const double* A;                 // the regressor's A, packed
  const double* ldA;               // ... and logdet A
  T* U; T* mwf; int32_t* finfo;    // the fold's factor, mean and status word
  double* kl;                      // the fold's log density (may be NULL)
  unsigned long long* degenerate;
  const T* img;                    // the fold's image
  T* km; T* kv;                    // at the fold's first row (may be NULL)
  int grp, ngroups;                // predict: this workgroup takes the tiles grp, grp + ngroups, ...
};

// dynamic LDS of kfl_state_kernel: the factor's upper triangle, packed by columns
inline size_t kfl_state_lds_bytes(size_t elem, int D) {
  const size_t DP = (size_t)16 * (((size_t)D + 15) / 16);
  return DP * (DP + 1) / 2 * elem;
}
// of kfl_predict_kernel: the tile, mw_f, and the image's column blocks in use
inline size_t kfl_predict_lds_bytes(size_t elem, int D) {
  const int NB = (D + 15) / 16, DP = 16 * NB;
  return (size_t)kCovTile * (size_t)(DP + 16 / (int)elem) * elem + (size_t)kCovMaxD * elem + (size_t)2 * NB * (NB + 1) * 64 * elem;
}

// ---- A = T'T in the packed layout of phase_chol, logdet A; one workgroup per regressor -------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void kfl_state_kernel(KflArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double scr[kWaves];
  T* const Ts = reinterpret_cast<T*>(smem);  // Ts[pidx(i, j)] = T[j, i], j <= i: column i of the factor, contiguous
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = a.D;
  const int64_t r = blockIdx.x, reg = (int64_t)a.reg0 + r;
  if (a.info[reg] != 0) return;  // (block-uniform)
  const int DP = 16 * ((D + 15) / 16), packed = DP * (DP + 1) / 2;
  const BLR_GLOBAL T* const Tg = as_global(a.Tf + reg * a.strideT);
  for (int i = wave; i < D; i += kWaves)
    for (int j = lane; j <= i; j += kWave) Ts[pidx(i, j)] = Tg[(int64_t)i * a.ldt + j];
  __syncthreads();
  BLR_GLOBAL double* const out = as_global(a.A + r * packed);
  // A[i][k] = sum_{j <= k} T[j, i] T[j, k], j ascending (k <= i), accumulated and kept in double in both element types: A - G_f
  // cancels, and what A's own rounding would add to the difference costs a D^3 / 3 product per regressor to avoid
  for (int i = wave; i < D; i += kWaves) {
    const T* const ci = Ts + pidx(i, 0);
    for (int k = lane; k <= i; k += kWave) {
      const T* const ck = Ts + pidx(k, 0);
      double acc = 0.0;
      for (int j = 0; j <= k; ++j) acc = fused_madd((double)ci[j], (double)ck[j], acc);
      out[pidx(i, k)] = acc;
    }
  }
  for (int idx = D * (D + 1) / 2 + tid; idx < packed; idx += kThreads) out[idx] = 0.0;  // padded rows
  const double v = tid < D ? log((double)Ts[pidx(tid, tid)]) : 0.0;
  const double ld = 2.0 * block_allreduce(v, scr, tid);
  if (tid == 0) a.ldA[r] = ld;
}

// ---- statistics of one column block of one fold: the streaming Gram phase without a prior, centred at the state's mean -----------
template <typename T, int NB, int MODE>
__device__ __forceinline__ void kfl_stats_body(char* smem, const KflFold<T>& v) {
  using C = SmallCfg<T, NB>;
  T* const P = reinterpret_cast<T*>(smem);
  T* const bvec = reinterpret_cast<T*>(smem + C::OFF_B);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  RegCtx<T>* ctx = reinterpret_cast<RegCtx<T>*>(smem + C::OFF_CTX);
  const int tid = threadIdx.x;
  if (tid == 0) {
    ctx->X = v.X;
    ctx->y = v.y;
    ctx->s = v.s;
    ctx->mw = v.mw;
    ctx->Lw = ctx->mw;  // (a valid address: phase_gram loads one word of it and drops the value)
    ctx->ldx = v.ldx;
    ctx->ldl = 0;
    ctx->D = v.D;
    ctx->N = v.n;
    ctx->noise_kind = v.noise_kind;
    ctx->prior_kind = kKflPriorNone;
  }
  __syncthreads();
  phase_gram<T, NB, MODE>(smem);
  BLR_GLOBAL double* const out = as_global(v.stats);
  for (int idx = tid; idx < C::PACKED; idx += kThreads) out[idx] = (double)P[idx];
  if (tid < C::DP) out[C::PACKED + tid] = (double)bvec[tid];
  if (tid == 0) {
    v.scal[0] = scr[4];
    v.scal[1] = scr[5];
  }
}

template <typename T, int NB, int MODE>
__global__ BLR_KFL_BOUNDS(T, NB) void kfl_stats_kernel(KflArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t r = blockIdx.y, reg = (int64_t)a.reg0 + r;
  if (a.info[reg] != 0) return;  // (block-uniform)
  const int f = (int)blockIdx.x / a.S, sp = (int)blockIdx.x - f * a.S;
  const int f0 = f * a.F, nf = min(a.F, a.N - f0);
  int Sf, chunk;
  kfl_splits(nf, &Sf, &chunk);
  if (sp >= Sf) return;  // (block-uniform) a shorter last fold: fewer blocks
  const int n0 = f0 + sp * chunk;
  const bool diag = a.noise_kind == NOISE_DIAGONAL;
  const int64_t slot = ((int64_t)r * a.nfolds + f) * a.S + sp;
  KflFold<T> v;
  v.X = a.X + reg * a.strideX + (a.layout == LAYOUT_COLVECS ? (int64_t)n0 * a.ldx : (int64_t)n0);
  v.y = a.y + reg * a.stridey + n0;
  v.s = a.s + reg * a.strides + (diag ? n0 : 0);
  v.mw = a.mw + reg * a.stridemw;
  v.ldx = a.ldx; v.D = a.D; v.noise_kind = a.noise_kind;
  v.n = max(0, min(chunk, nf - sp * chunk));
  v.stats = a.stats + slot * kfl_stat_elems<T, NB>();
  v.scal = a.scal + 2 * slot;
  kfl_stats_body<T, NB, MODE>(smem, v);
}

// ---- fp32: the same statistics accumulated in DOUBLE on v_mfma_f64_16x16x4 from the float inputs ---------------------------------
// A - G_f cancels: a fold with 19/20 of the state's information multiplies the relative error of G_f by 20, and the fp32 accumulators
// of phase_gram (a few eps32 after some hundred columns) then miss what a careful fp32 computation of the outputs gives -- measured
// at D = 1 with one fold of all the data: 1.02 - 1.25 x the yardstick of tests/_kfold_large_ref.py.  The float inputs are exact in
// double, the matrix core's fp64 rate on 16x16x4 equals its fp32 rate, so this kernel takes the fold's float rows, widens them on the
// way into LDS and accumulates G_f, d_f, q_f and l_f in double; the statistics buffer is double in both element types.
// Stages of 64 inputs through registers into LDS rows (the tile walk of kfl_predict_kernel; a row past the block's end is not read).
// Per stage: thread n < 64 forms w_n = 1 / s_n and r0_n = y_n - x_n'mw; thread d < DP adds sum_n x_dn w_n r0_n to its d_f entry;
// wave w owns the lower-triangular 16 x 16 tiles t = w, w + 4, ... (at most nine) and adds sum_n (x_in w_n) x_kn on the matrix core,
// n ascending.  Every sum has a fixed order.
constexpr int kKflTile = 64;
inline size_t kfl_stats32_lds_bytes(int D) {
  const size_t DP = (size_t)16 * (((size_t)D + 15) / 16);
  return ((size_t)kKflTile * (DP + 1) + 2 * kKflTile + 128) * sizeof(double);
}

template <int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__device__ __forceinline__ void kfl_stats32_body(char* smem, double* scr /* [kWaves], LDS */, const KflFold<float>& a) {
  using Mf = Mfma<double>;
  using acc4 = Mf::acc4;
  constexpr int TN = kKflTile, MAXT = 9;  // 36 tiles at DP = 128: nine per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int nblk = a.n;  // rows of this block
  const int D = a.D, NB = (D + 15) / 16, DP = 16 * NB, LDX = DP + 1, NT = NB * (NB + 1) / 2;
  const bool diag = a.noise_kind == NOISE_DIAGONAL;

  double* const Xs = reinterpret_cast<double*>(smem);  // [TN][LDX]: the odd row stride keeps a column walk (lane = row) off one bank
  double* const ws = Xs + TN * LDX;                     // [TN] 1 / s_n (0 for a row past the block)
  double* const rs = ws + TN;                           // [TN] w_n r0_n
  double* const mws = rs + TN;                          // [128]

  const BLR_GLOBAL float* const Xg = as_global(a.X);
  const BLR_GLOBAL float* const yg = as_global(a.y);
  const BLR_GLOBAL float* const sg = as_global(a.s);
  if (tid < 128) mws[tid] = tid < D ? (double)as_global(a.mw)[tid] : 0.0;

  const int xcnt = DP / 4;
  float xreg[32];
  auto prefetch = [&](int tile) {
    const int t0 = tile * TN;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      if (i < xcnt) {
        const int e = tid + kThreads * i;
        int d, n;
        if (LAYOUT == LAYOUT_COLVECS) { d = (tid & 15) + 16 * (i >> 2); n = (tid >> 4) + 16 * (i & 3); } else { n = e % TN; d = e / TN; }
        const bool ok = d < D && t0 + n < nblk;
        const int64_t at = LAYOUT == LAYOUT_COLVECS ? (int64_t)d + (int64_t)(t0 + n) * a.ldx : (int64_t)(t0 + n) + (int64_t)d * a.ldx;
        xreg[i] = ok ? Xg[at] : 0.0f;
      }
    }
  };
  const int ntiles = (nblk + TN - 1) / TN;
  if (ntiles > 0) prefetch(0);

  // this wave's tiles (wave-uniform), their accumulators
  acc4 acc[MAXT];
  int tI[MAXT], tK[MAXT];
#pragma unroll
  for (int i = 0; i < MAXT; ++i) {
    acc[i] = acc4{0.0, 0.0, 0.0, 0.0};
    const int t = wave + kWaves * i;
    tI[i] = uni(tile_I(t < NT ? t : 0));
    tK[i] = uni(t < NT ? t - tI[i] * (tI[i] + 1) / 2 : -1);  // -1: not a tile of this problem
  }
  double bacc = 0.0, qacc = 0.0, lacc = 0.0;

  for (int tile = 0; tile < ntiles; ++tile) {
    const int t0 = tile * TN;
    __syncthreads();  // the previous stage's readers are done (first stage: nothing pending)
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      if (i < xcnt) {
        const int e = tid + kThreads * i;
        int d, n;
        if (LAYOUT == LAYOUT_COLVECS) { d = (tid & 15) + 16 * (i >> 2); n = (tid >> 4) + 16 * (i & 3); } else { n = e % TN; d = e / TN; }
        Xs[n * LDX + d] = (double)xreg[i];
      }
    }
    __syncthreads();  // (also: mw in place)
    if (tile + 1 < ntiles) prefetch(tile + 1);  // in flight during this stage's products
    if (tid < TN) {  // per input: the weight and the weighted residual
      double wv = 0.0, wr = 0.0;
      if (t0 + tid < nblk) {
        const double sv = (double)sg[diag ? t0 + tid : 0];
        double m = 0.0;
        for (int d = 0; d < D; ++d) m = fused_madd(Xs[tid * LDX + d], mws[d], m);
        const double r0 = (double)yg[t0 + tid] - m;
        wv = 1.0 / sv;
        wr = wv * r0;
        qacc = fused_madd(r0, wr, qacc);
        lacc += log(sv);
      }
      ws[tid] = wv;
      rs[tid] = wr;
    }
    __syncthreads();
    if (tid < DP) {  // d_f: one entry per thread, n ascending
      for (int n = 0; n < TN; ++n) bacc = fused_madd(Xs[n * LDX + tid], rs[n], bacc);
    }
#pragma unroll 1
    for (int ks = 0; ks < TN / 4; ++ks) {
      const double* const xk = Xs + (4 * ks + g) * LDX + li;
      const double wk = ws[4 * ks + g];
#pragma unroll
      for (int i = 0; i < MAXT; ++i) {
        if (tK[i] >= 0) acc[i] = Mf::mma(xk[16 * tI[i]] * wk, xk[16 * tK[i]], acc[i]);  // (wave-uniform branch)
      }
    }
  }

  const int packed = DP * (DP + 1) / 2;
  BLR_GLOBAL double* const out = as_global(a.stats);
#pragma unroll
  for (int i = 0; i < MAXT; ++i) {
    if (tK[i] >= 0) {
      const int col = 16 * tK[i] + li;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * tI[i] + Mf::crow(lane, v);
        if (col <= row) out[pidx(row, col)] = acc[i][v];
      }
    }
  }
  if (tid < DP) out[packed + tid] = bacc;
  const double q = block_allreduce(qacc, scr, tid);
  const double l = block_allreduce(lacc, scr, tid);
  if (tid == 0) {
    a.scal[0] = q;
    a.scal[1] = l;
  }
}

template <int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void kfl_stats32_kernel(KflArgs<float> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double scr[kWaves];
  const int64_t r = blockIdx.y, reg = (int64_t)a.reg0 + r;
  if (a.info[reg] != 0) return;  // (block-uniform)
  const int f = (int)blockIdx.x / a.S, sp = (int)blockIdx.x - f * a.S;
  const int f0 = f * a.F, nf = min(a.F, a.N - f0);
  int Sf, chunk;
  kfl_splits(nf, &Sf, &chunk);
  if (sp >= Sf) return;  // (block-uniform) a shorter last fold: fewer blocks
  const int n0 = f0 + sp * chunk;  // rows of this block: [n0, n0 + v.n)
  const int DP = 16 * ((a.D + 15) / 16);
  const int64_t slot = ((int64_t)r * a.nfolds + f) * a.S + sp;
  KflFold<float> v;
  v.X = a.X + reg * a.strideX + (LAYOUT == LAYOUT_COLVECS ? (int64_t)n0 * a.ldx : (int64_t)n0);
  v.y = a.y + reg * a.stridey + n0;
  v.s = a.s + reg * a.strides + (a.noise_kind == NOISE_DIAGONAL ? n0 : 0);
  v.mw = a.mw + reg * a.stridemw;
  v.ldx = a.ldx; v.D = a.D; v.noise_kind = a.noise_kind;
  v.n = max(0, min(chunk, nf - sp * chunk));
  v.stats = a.stats + slot * (int64_t)(DP * (DP + 1) / 2 + DP);
  v.scal = a.scal + 2 * slot;
  kfl_stats32_body<LAYOUT>(smem, scr, v);
}

// ---- column blocks 1 .. S_f - 1 of a fold added to block 0, in that order (grid_reduce_kernel's pattern) ---------------------------
// st, scal: the fold's block 0, its S_f blocks one behind the other; the workgroup's threads take idx = first, first + step, ...
__device__ __forceinline__ void kfl_reduce_body(double* st, double* scal, int Sf, int SZ, int first, int step, bool lead) {
  for (int idx = first; idx < SZ; idx += step) {
    double acc = st[idx];
    for (int sp = 1; sp < Sf; ++sp) acc += st[(int64_t)sp * SZ + idx];
    st[idx] = acc;
  }
  if (lead) {
    double q = scal[0], l = scal[1];
    for (int sp = 1; sp < Sf; ++sp) {
      q += scal[2 * sp];
      l += scal[2 * sp + 1];
    }
    scal[0] = q;
    scal[1] = l;
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void kfl_reduce_kernel(KflArgs<T> a, int SZ) {
  const int64_t rf = blockIdx.x;  // chunk-local (regressor, fold)
  const int64_t r = rf / a.nfolds;
  const int f = (int)(rf - r * a.nfolds);
  if (a.info[(int64_t)a.reg0 + r] != 0) return;
  const int nf = min(a.F, a.N - f * a.F);
  int Sf, chunk;
  kfl_splits(nf, &Sf, &chunk);
  if (Sf < 2) return;
  kfl_reduce_body(a.stats + rf * a.S * (int64_t)SZ, a.scal + 2 * rf * a.S, Sf, SZ, blockIdx.y * kThreads + threadIdx.x, gridDim.y * kThreads,
                  blockIdx.y == 0 && threadIdx.x == 0);
}

// ---- one fold: A_f = A - G_f, its factor U_f, mw_f, the fold's joint log density ----------------------------------------------------
// Two workgroups per CU (256 registers per lane) in every instantiation: under the statistics kernel's bounds (four per CU at
// NB <= 4, three waves per SIMD in fp32) the instantiations <double, 4> and <float, 8> spilled three vector registers each.
template <typename T, int NB>
__device__ __forceinline__ void kfl_factor_body(char* smem, const KflFold<T>& a) {
  using C = SmallCfg<T, NB>;
  static_assert(2 * C::LDS_BYTES <= 160 * 1024, "two workgroups per CU: twice the dynamic LDS of a launch must fit 160 KB");
  T* const P = reinterpret_cast<T*>(smem);
  T* const bvec = reinterpret_cast<T*>(smem + C::OFF_B);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  const int tid = threadIdx.x;
  const int D = a.D;
  const BLR_GLOBAL double* const st = as_global(a.stats);
  const BLR_GLOBAL double* const Ag = as_global(a.A);
  for (int idx = tid; idx < C::PACKED; idx += kThreads) P[idx] = (T)(Ag[idx] - st[idx]);  // one rounding of the difference
  if (tid < C::DP) bvec[tid] = (T)st[C::PACKED + tid];
  __syncthreads();
  // The phases are inlined HERE (a statement attribute outranks their noinline): as calls they cost this kernel 8 - 12 B of scratch
  // per lane for the call frames; inlined, every instantiation has 0 B and no spilled register within 256.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wignored-attributes"
  int chol_info;
  [[clang::always_inline]] chol_info = phase_chol<T, NB, 2>(smem, D, 1);  // u_f = U_f^-T d_f rides along
  bool bad = chol_info != 0;                                               // a pivot <= 0 or NaN
  double uu = 0.0, ld = 0.0;
  if (!bad) {
    [[clang::always_inline]] phase_backsolve<T, NB, 2>(smem, D, a.U, (int64_t)D);  // bvec <- U_f^-1 u_f; the factor goes out
#pragma clang diagnostic pop
    uu = scr[6];                                                                  // |u_f|^2
    ld = scr[7];                                                                  // logdet A_f
    bad = !isfinite(uu) || !isfinite(ld);                                         // (an infinite pivot; block-uniform: LDS values)
  }
  double* const kl = a.kl;
  if (bad) {
    if (tid == 0) {
      *a.finfo = 2;
      if (kl) *kl = __longlong_as_double(0x7ff8000000000000LL);
      atomicAdd(a.degenerate, 1ull);
    }
    return;
  }
  if (tid < D) a.mwf[tid] = as_global(a.mw)[tid] - bvec[tid];
  if (tid == 0) {
    *a.finfo = 0;
    if (kl) {
      const double LOG2PI = 1.8378770664093454835606594728112;
      const double nf = (double)a.n;
      *kl = -0.5 * (nf * LOG2PI + a.scal[1] + *a.ldA - ld + a.scal[0] + uu);
    }
  }
}

template <typename T, int NB>
__global__ __launch_bounds__(kThreads, 2) void kfl_factor_kernel(KflArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = SmallCfg<T, NB>;
  constexpr int SZ = kfl_stat_elems<T, NB>();
  const int f = blockIdx.x;
  const int64_t r = blockIdx.y, reg = (int64_t)a.reg0 + r;
  const int64_t rf = r * a.nfolds + f;
  if (a.info[reg] != 0) {  // (block-uniform) nothing of this regressor is computed: no image, no prediction
    if (threadIdx.x == 0) a.finfo[rf] = 1;
    return;
  }
  KflFold<T> v;
  v.mw = a.mw + reg * a.stridemw;
  v.D = a.D; v.n = min(a.F, a.N - f * a.F);
  v.stats = a.stats + rf * a.S * (int64_t)SZ;
  v.scal = a.scal + 2 * rf * a.S;
  v.A = a.A + r * C::PACKED;
  v.ldA = a.ldA + r;
  v.U = a.U + rf * (int64_t)a.D * a.D;
  v.mwf = a.mwf + rf * a.D;
  v.finfo = a.finfo + rf;
  v.kl = a.kl ? a.kl + reg * a.stride_kl + f : nullptr;
  v.degenerate = a.degenerate;
  kfl_factor_body<T, NB>(smem, v);
}

// ---- the fold's rows against its own factor: kf_mean_n = x_n'mw_f, kf_var_n = s_n + |U_f^-T x_n|^2 --------------------------------
template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__device__ __forceinline__ void kfl_predict_body(char* smem, const KflFold<T>& a) {
  using Mf = Mfma<T>;
  using G = MargGemmCfg<T>;
  using acc4 = typename Mf::acc4;
  constexpr int TN = kCovTile, VEC = Mf::VEC;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int grp = a.grp;
  const int D = a.D;
  const int nf = a.n;  // the fold's rows
  const int NB = (D + 15) / 16, DP = 16 * NB, LDX = cov_ldz<T>(DP);
  BLR_GLOBAL T* const km = a.km ? as_global(a.km) : nullptr;
  BLR_GLOBAL T* const kv = a.kv ? as_global(a.kv) : nullptr;
  if (*a.finfo != 0) {  // (block-uniform) the NaN rule: every member of the fold
    const T nan = (T)__builtin_nan("");
    for (int n = grp * kThreads + tid; n < nf; n += a.ngroups * kThreads) {
      if (km) km[n] = nan;
      if (kv) kv[n] = nan;
    }
    return;
  }

  T* const Xs = reinterpret_cast<T*>(smem);  // [TN][LDX]
  T* const mws = Xs + TN * LDX;              // [128]
  T* const img = mws + kCovMaxD;             // [2 NB (NB + 1)][64]

  const BLR_GLOBAL T* const Xg = as_global(a.X);
  const BLR_GLOBAL T* const sg = as_global(a.s);
  const int ntiles = (nf + TN - 1) / TN;

  // the tile through registers, as cov_whiten_kernel loads it; a row past the FOLD's end is not read (zeros)
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
        const bool ok = d < D && n0 + n < nf;
        const int64_t at = LAYOUT == LAYOUT_COLVECS ? (int64_t)d + (int64_t)(n0 + n) * a.ldx : (int64_t)(n0 + n) + (int64_t)d * a.ldx;
        xreg[i] = ok ? Xg[at] : T(0);
      }
    }
  };
  if (grp < ntiles) prefetch(grp);

  // ---- once per workgroup: the fold's image and mean ----
  {
    const BLR_GLOBAL vecT* const src = reinterpret_cast<const BLR_GLOBAL vecT*>(as_global(a.img));
    vecT* const dst = reinterpret_cast<vecT*>(img);
    const int nvec = G::frag0(NB) * 64 / VEC;
    for (int e = tid; e < nvec; e += kThreads) dst[e] = src[e];
  }
  if (tid < kCovMaxD) mws[tid] = tid < D ? as_global(a.mwf)[tid] : T(0);

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
    __syncthreads();  // (also: image and mw_f in place)
    if (tile + a.ngroups < ntiles) prefetch(tile + a.ngroups);  // in flight during this tile's products
    const int n = n0 + row;  // fold-local
    const T* const xr = Xs + row * LDX;

    // kf_mean_n = x_n'mw_f: the four lane groups take d = g mod 4, then a fixed two-step butterfly
    T m = T(0);
    for (int d = g; d < DP; d += 4) m = fused_madd(xr[d], mws[d], m);
    m += __shfl_xor(m, 16, 64);
    m += __shfl_xor(m, 32, 64);
    // |z_n|^2, z_n = U_f^-T x_n column block by column block from the image; this lane holds four entries of z_n per block
    T zz = T(0);
#pragma unroll 1
    for (int J = 0; J < NB; ++J) {
      acc4 acc = {T(0), T(0), T(0), T(0)};
      const T* const fb = img + G::frag0(J) * 64 + lane;
#pragma unroll 4
      for (int mm = 0; mm < 4 * (J + 1); ++mm) acc = Mf::mma(fb[mm * 64], xr[G::d_of(mm, g)], acc);
#pragma unroll
      for (int v = 0; v < 4; ++v) zz = fused_madd(acc[v], acc[v], zz);
    }
    zz += __shfl_xor(zz, 16, 64);
    zz += __shfl_xor(zz, 32, 64);
    if (g == 0 && n < nf) {  // (a partial last tile: its rows past the fold store nothing)
      if (km) km[n] = m;
      if (kv) kv[n] = sg[a.noise_kind == NOISE_DIAGONAL ? n : 0] + zz;
    }
  }
}

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void kfl_predict_kernel(KflArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int f = blockIdx.y;
  const int64_t r = blockIdx.z, reg = (int64_t)a.reg0 + r;
  if (a.info[reg] != 0) return;  // (block-uniform) outputs untouched
  const int64_t rf = r * a.nfolds + f;
  const int f0 = f * a.F;  // the fold's rows: [f0, f0 + v.n)
  KflFold<T> v;
  v.X = a.X + reg * a.strideX + (LAYOUT == LAYOUT_COLVECS ? (int64_t)f0 * a.ldx : (int64_t)f0);
  v.s = a.s + reg * a.strides + (a.noise_kind == NOISE_DIAGONAL ? f0 : 0);
  v.ldx = a.ldx; v.D = a.D; v.noise_kind = a.noise_kind;
  v.n = min(a.F, a.N - f0);
  v.mwf = a.mwf + rf * a.D;
  v.finfo = a.finfo + rf;
  v.img = a.img + rf * MargGemmCfg<T>::IMG_ELEMS;
  v.km = a.km ? a.km + reg * a.stride_km + f0 : nullptr;
  v.kv = a.kv ? a.kv + reg * a.stride_kv + f0 : nullptr;
  v.grp = blockIdx.x; v.ngroups = a.ngroups;
  kfl_predict_body<T, LAYOUT>(smem, v);
}

// the instantiations the library uses, defined in blr_kfold_large.hip
#define BLR_KFL_EXTERN_NB(T, NB)                                                    \
  extern template __global__ void kfl_stats_kernel<double, NB, 0>(KflArgs<double>); \
  extern template __global__ void kfl_stats_kernel<double, NB, 1>(KflArgs<double>); \
  extern template __global__ void kfl_stats_kernel<double, NB, 4>(KflArgs<double>); \
  extern template __global__ void kfl_factor_kernel<T, NB>(KflArgs<T>);
#define BLR_KFL_EXTERN(T)                                                                                                  \
  BLR_KFL_EXTERN_NB(T, 1) BLR_KFL_EXTERN_NB(T, 2) BLR_KFL_EXTERN_NB(T, 3) BLR_KFL_EXTERN_NB(T, 4) BLR_KFL_EXTERN_NB(T, 5) \
  BLR_KFL_EXTERN_NB(T, 6) BLR_KFL_EXTERN_NB(T, 7) BLR_KFL_EXTERN_NB(T, 8)                                                  \
  extern template __global__ void kfl_state_kernel<T>(KflArgs<T>);                                                         \
  extern template __global__ void kfl_reduce_kernel<T>(KflArgs<T>, int);                                                   \
  extern template __global__ void kfl_predict_kernel<T, LAYOUT_COLVECS>(KflArgs<T>);                                       \
  extern template __global__ void kfl_predict_kernel<T, LAYOUT_ROWVECS>(KflArgs<T>);
BLR_KFL_EXTERN(double)
BLR_KFL_EXTERN(float)
extern template __global__ void kfl_stats32_kernel<LAYOUT_COLVECS>(KflArgs<float>);
extern template __global__ void kfl_stats32_kernel<LAYOUT_ROWVECS>(KflArgs<float>);
#undef BLR_KFL_EXTERN
#undef BLR_KFL_EXTERN_NB

}  // namespace blr
