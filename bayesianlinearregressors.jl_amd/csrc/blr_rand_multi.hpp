// Draws from a batched MULTI-OUTPUT state (blr_rand_multi_batched_*): S column posteriors N(M[:, c], (U'U)^-1) per
// regressor share one factor, R draws per column, draw j = c R + r:
//   W[:, j] = M[:, c] + U \ Z1[:, j]                 (reference src/bayesian_linear_regression.jl:51, sampling_functions.jl:27-49)
//   Y[:, j] = X'W[:, j] (+ sqrt.(s) .* Z2[:, j])     (:52-53; sampling_functions.jl:16-18 without Z2)
// Replaces S calls of blr_rand_batched_* with mw stepped by a column: each of them reads every factor again per (regressor, block of
// draws), reads X again for the projection and pays its own launches.
//
// rand_cols_solve_kernel<T>: grid (passes of kRandColsPerPass draw columns, regressors of the launch), 256 threads.  Per workgroup:
//   status   every wave forms the regressor's status from the diagonal (the rule of blr_rand_batched_*); pass 0 writes it; a failed
//            regressor writes nothing else;
//   factor   the upper factor once into LDS as packed rows (the image of state_cols_kernel); a diagonal prior needs none;
//   solve    wave w takes the pass's columns w, w + 4, w + 8, w + 12 through state_backward (blr_state_cols.hpp): one chain of D
//            steps, four independent readlane + FMA strands, lanes owning rows lane and lane + 64; then + M[:, j / R] -- a pass may
//            straddle any number of mean columns;
//   stores   W to the caller's buffer, and -- when Y is wanted -- to handle workspace AS THE A FRAGMENTS of the projection
//            (element (d, slot) of a pass at 64 (d / 4) + 16 (d % 4) + slot, rows D .. 16 ceil(D / 16) - 1 and the slots past the last
//            draw zero), so that the projection's operand loads are whole 64-lane rows.
// rand_cols_project_kernel<T, LAYOUT>: one-dimensional grid over (groups of 64-input tiles, regressors of the launch), regressor
// fastest when X is shared (as rand_batched_tile orders them).  The tile walk is marginals_cols_kernel's (inputs become rows of an LDS
// tile through registers, the next tile's loads in flight during the products); the pass loop inside it is loo_cols_kernel's: the
// workgroup keeps its tile and reloads the fragments of a pass from the workspace (L2), so X is read once whatever S R is.  Per pass
// Y' = W'X_tile' on v_mfma_f64_16x16x4 / v_mfma_f32_16x16x4, k = d ascending, then + sqrt(s_n) Z2[n, j] at the store (coalesced along n).
// Every sum has a fixed order, nothing is atomic, a strand of the solve and an output row of an MFMA see their own column only: the
// bits of a draw do not depend on S, on R, on its pass or slot or on the other draws.
#pragma once
#include "blr_common.hpp"
#include "blr_marg_multi.hpp"
#include "blr_state_cols.hpp"

namespace blr {

constexpr int kRandColsPerPass = 16;  // draw columns of a pass: four per wave in the solve, one 16-row A operand in the projection
constexpr int kRandColsPerWave = kRandColsPerPass / kWaves;
static_assert(kRandColsPerPass == 16, "a pass is one 16-row MFMA operand");

template <typename T>
struct RandColsArgs {
  const T* X; int64_t ldx, strideX;    // may be NULL without a projection
  const T* s; int64_t strides;         // read only when Z2 != NULL
  const T* M; int64_t ldm, strideM;    // D x S mean columns per regressor
  const T* U; int64_t ldu, strideU;    // upper factor (ldu >= D) or, with a diagonal prior, d[D]
  const int32_t* chol_info;            // status of the factorisation of a dense prior (NULL for the other kinds)
  const T* Z1; int64_t ldz1, strideZ1;
  const T* Z2; int64_t ldz2, strideZ2;  // NULL: noise-free function values
  T* W; int64_t ldw, strideW;          // caller's weights (may be NULL)
  T* Wf;                               // fragment images for the projection, rand_cols_image_elems apart per regressor of the launch (NULL without one)
  T* Y; int64_t ldy, strideY;
  int32_t* info;
  int noise_kind, prior_kind;          // prior_kind: PRIOR_UPPER_FACTOR or PRIOR_DIAGONAL here
  int D, N, R, SR;                     // SR = S R draws per regressor
  int ngroups;                         // tile groups per regressor (projection)
  int reg0, nreg;                      // first regressor of this launch and their count
};

// workspace of one regressor: a 16 ceil(D / 16) x 16 image per pass
__host__ __device__ inline size_t rand_cols_image_elems(int D, int64_t SR) {
  return (size_t)((SR + kRandColsPerPass - 1) / kRandColsPerPass) * (size_t)(16 * ((D + 15) / 16)) * kRandColsPerPass;
}
inline size_t rand_cols_solve_lds_bytes(size_t elem, int D, bool diagonal) { return diagonal ? 0 : (size_t)state_packed_elems(D) * elem; }
inline size_t rand_cols_project_lds_bytes(size_t elem, int D) {  // the tile of marginals_cols_kernel alone
  const int DP = 16 * ((D + 15) / 16);
  return (size_t)kMargTile * (size_t)(DP + 16 / (int)elem) * elem;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void rand_cols_solve_kernel(RandColsArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int W = kRandColsPerPass, C = kRandColsPerWave;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pass = blockIdx.x;
  const int64_t reg = (int64_t)a.reg0 + blockIdx.y;
  const int D = a.D, DP = 16 * ((D + 15) / 16);
  const int i0 = lane, i1 = lane + 64;
  const bool has0 = i0 < D, has1 = i1 < D;
  const bool diag = a.prior_kind == PRIOR_DIAGONAL;
  const BLR_GLOBAL T* const Ug = as_global(a.U + reg * a.strideU);

  // status (every wave, the same bits): the factorisation's own, else the first non-positive diagonal entry (1-based), else 0
  int bad = a.chol_info ? a.chol_info[reg] : 0;
  if (!bad) {
    const T d0 = has0 ? Ug[diag ? i0 : (int64_t)i0 * a.ldu + i0] : T(1);
    const T d1 = has1 ? Ug[diag ? i1 : (int64_t)i1 * a.ldu + i1] : T(1);
    const unsigned long long m0 = __ballot(!(d0 > T(0))), m1 = __ballot(!(d1 > T(0)));
    bad = m0 ? __builtin_ctzll(m0) + 1 : (m1 ? __builtin_ctzll(m1) + 65 : 0);
  }
  if (pass == 0 && tid == 0) a.info[reg] = bad;
  if (bad) return;  // (block-uniform) a failed regressor's outputs stay untouched

  T* const Rm = reinterpret_cast<T*>(smem);  // packed rows of U: element (j, col) at j D - j (j - 1) / 2 + col
  if (!diag) {
    for (int e = tid; e < D * D; e += kThreads) {
      const int c = e / D, j = e - c * D;
      if (j <= c) Rm[j * D - (j * (j - 1)) / 2 + c] = Ug[(int64_t)c * a.ldu + j];
    }
    __syncthreads();
  }

  const int j0 = pass * W;
  const int ncols = min(W, a.SR - j0);
  const BLR_GLOBAL T* const Zg = as_global(a.Z1 + reg * a.strideZ1);
  T b0[C], b1[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int sl = wave + kWaves * c;
    const int64_t j = j0 + (sl < ncols ? sl : 0);
    b0[c] = (sl < ncols && has0) ? Zg[j * a.ldz1 + i0] : T(0);
    b1[c] = (sl < ncols && has1) ? Zg[j * a.ldz1 + i1] : T(0);
  }
  if (wave < ncols) {  // (wave-uniform; no barrier below)
    if (diag) {        // w = z / sqrt(d), as diag_sample_kernel
      const T q0 = has0 ? sqrt(Ug[i0]) : T(1), q1 = has1 ? sqrt(Ug[i1]) : T(1);
#pragma unroll
      for (int c = 0; c < C; ++c) { b0[c] = b0[c] / q0; b1[c] = b1[c] / q1; }
    } else {
      const T t0 = has0 ? Rm[i0 * D - (i0 * (i0 - 1)) / 2 + i0] : T(1), t1 = has1 ? Rm[i1 * D - (i1 * (i1 - 1)) / 2 + i1] : T(1);
      const T r0 = has0 ? T(1) / t0 : T(0), r1 = has1 ? T(1) / t1 : T(0);
      state_backward<T, C>(Rm, D, lane, r0, r1, b0, b1);
    }
  }
  const BLR_GLOBAL T* const Mg = as_global(a.M + reg * a.strideM);
  BLR_GLOBAL T* const Wg = a.W ? as_global(a.W + reg * a.strideW) : nullptr;
  BLR_GLOBAL T* const Fg = a.Wf ? as_global(a.Wf + (int64_t)blockIdx.y * (int64_t)rand_cols_image_elems(D, a.SR) + (int64_t)pass * DP * W) : nullptr;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int sl = wave + kWaves * c;
    T w0 = T(0), w1 = T(0);
    if (sl < ncols) {
      const int64_t j = j0 + sl;
      const BLR_GLOBAL T* const mcol = Mg + (j / a.R) * a.ldm;
      if (has0) w0 = b0[c] + mcol[i0];
      if (has1) w1 = b1[c] + mcol[i1];
      if (Wg) {
        if (has0) Wg[j * a.ldw + i0] = w0;
        if (has1) Wg[j * a.ldw + i1] = w1;
      }
    }
    if (Fg) {  // every slot and every padded row: the projection reads them unguarded
      if (i0 < DP) Fg[64 * (i0 >> 2) + 16 * (i0 & 3) + sl] = w0;
      if (i1 < DP) Fg[64 * (i1 >> 2) + 16 * (i1 & 3) + sl] = w1;
    }
  }
}

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void rand_cols_project_kernel(RandColsArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Mf = Mfma<T>;
  using acc4 = typename Mf::acc4;
  constexpr int W = kRandColsPerPass, TN = kMargTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  // (group, regressor) of this workgroup: the regressor fastest when X is shared, so that the workgroups that run together read the
  // same tile of X from L2; with one X per regressor its groups are consecutive
  int grp, rl;
  if (a.strideX == 0) { rl = (int)(blockIdx.x % (unsigned)a.nreg); grp = (int)(blockIdx.x / (unsigned)a.nreg); }
  else                { rl = (int)(blockIdx.x / (unsigned)a.ngroups); grp = (int)(blockIdx.x % (unsigned)a.ngroups); }
  const int64_t reg = (int64_t)a.reg0 + rl;
  if (a.info[reg] != 0) return;  // (block-uniform; written by rand_cols_solve_kernel, the launch before) outputs untouched
  const int D = a.D, N = a.N;
  const int NB = (D + 15) / 16, DP = 16 * NB, NK = DP / 4, LDX = marg_cols_ldx<T>(DP);
  const int npasses = (a.SR + W - 1) / W;

  T* const Xs = reinterpret_cast<T*>(smem);  // [TN][LDX]
  const BLR_GLOBAL T* const Xg = as_global(a.X + reg * a.strideX);
  const BLR_GLOBAL T* const sg = a.Z2 ? as_global(a.s + reg * a.strides) : nullptr;
  const BLR_GLOBAL T* const Z2g = a.Z2 ? as_global(a.Z2 + reg * a.strideZ2) : nullptr;
  const BLR_GLOBAL T* const Fg = as_global(a.Wf + (int64_t)rl * (int64_t)rand_cols_image_elems(D, a.SR));
  BLR_GLOBAL T* const Yg = as_global(a.Y + reg * a.strideY);
  const int ntiles = (N + TN - 1) / TN;

  // ---- the tile through registers, as marginals_cols_kernel stages it ----
  const int xcnt = DP / 4;
  T xreg[32];
  auto prefetch = [&](int tile) {
    const int n0 = tile * TN;
    if (LAYOUT == LAYOUT_COLVECS) {
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        if (i < xcnt) {
          const int d = (tid & 15) + 16 * (i >> 2), n = (tid >> 4) + 16 * (i & 3);
          const bool ok = d < D && n0 + n < N;
          xreg[i] = ok ? Xg[(int64_t)d + (int64_t)(n0 + n) * a.ldx] : T(0);
        }
      }
    } else {  // element tid + 256 i is input tid % 64 of feature tid / 64 + 4 i: one pointer per thread, stepped by four rows of X
      const int n = tid & (TN - 1);
      const bool nin = n0 + n < N;
      const BLR_GLOBAL T* p = Xg + (int64_t)(n0 + n) + (int64_t)(tid >> 6) * a.ldx;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        if (i < xcnt) {
          xreg[i] = (nin && (tid >> 6) + 4 * i < D) ? *p : T(0);
          p += 4 * a.ldx;
        }
      }
    }
  };
  if (grp < ntiles) prefetch(grp);

  // A fragments of W' for one pass: mf[ks] = W[4 ks + g, 16 pass + li], one 64-lane row of the image per k-step
  T mf[32];
  auto load_fragments = [&](int pass) {
    const BLR_GLOBAL T* const Fp = Fg + (int64_t)pass * DP * W + lane;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) mf[ks] = ks < NK ? Fp[64 * ks] : T(0);
  };
  if (npasses == 1) load_fragments(0);  // a single pass: once per workgroup
  const T s_iso = (sg && a.noise_kind == NOISE_ISOTROPIC) ? sqrt(sg[0]) : T(0);

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
    __syncthreads();
    if (tile + a.ngroups < ntiles) prefetch(tile + a.ngroups);  // in flight during this tile's products
    const int n = n0 + row;
    const bool nok = n < N;
    T sd = s_iso;  // sqrt(s_n)
    if (sg && a.noise_kind == NOISE_DIAGONAL) sd = nok ? sqrt(sg[n]) : T(0);
    const T* const xr = Xs + row * LDX;

    for (int pass = 0; pass < npasses; ++pass) {
      if (npasses > 1) load_fragments(pass);
      // Y' = W'X_tile': acc[v] = draw 16 pass + crow(lane, v) at input n
      acc4 acc = {T(0), T(0), T(0), T(0)};
#pragma unroll
      for (int ks = 0; ks < 32; ++ks)
        if (ks < NK) acc = Mf::mma(mf[ks], xr[4 * ks + g], acc);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t j = (int64_t)pass * W + Mf::crow(lane, v);
        if (nok && j < a.SR) {
          T y = acc[v];
          if (Z2g) y = fused_madd(sd, Z2g[j * a.ldz2 + n], y);
          Yg[j * a.ldy + n] = y;
        }
      }
    }
  }
}

// the instantiations the library uses, defined in blr_rand_multi.hip
extern template __global__ void rand_cols_solve_kernel<double>(RandColsArgs<double>);
extern template __global__ void rand_cols_solve_kernel<float>(RandColsArgs<float>);
extern template __global__ void rand_cols_project_kernel<double, LAYOUT_COLVECS>(RandColsArgs<double>);
extern template __global__ void rand_cols_project_kernel<double, LAYOUT_ROWVECS>(RandColsArgs<double>);
extern template __global__ void rand_cols_project_kernel<float, LAYOUT_COLVECS>(RandColsArgs<float>);
extern template __global__ void rand_cols_project_kernel<float, LAYOUT_ROWVECS>(RandColsArgs<float>);

}  // namespace blr
