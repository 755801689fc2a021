// Draws from a batch of regressors in a fixed number of launches (blr_rand_batched_*, D <= 128):
//   W_b = mw_b + U_b^-1 Z1_b            (reference src/bayesian_linear_regression.jl:51, sampling_functions.jl:27-49)
//   Y_b = X_b' W_b (+ sqrt.(s_b) .* Z2_b) (:52-53)
// One wave per (regressor, block of NS draws).  Every output bit is a function of that regressor's operands alone: the
// grid decides only WHERE a regressor is computed, never how, so the result does not depend on B or on b's position.
#pragma once
#include "blr_common.hpp"
#include "blr_aux_kernels.hpp"

namespace blr {

template <typename T>
struct RandBatchedArgs {
  const T* X; int64_t ldx, strideX;   // may be NULL when N == 0 or Y == NULL
  const T* s; int64_t strides;        // read only when Z2 != NULL
  const T* mw; int64_t stridemw;
  const T* U; int64_t ldu, strideU;   // upper factor (ldu >= D) or, with a diagonal prior, d[D]
  const int32_t* chol_info;           // status of the factorisation of a dense prior (NULL for the other kinds)
  const T* Z1; int64_t ldz1, strideZ1;
  const T* Z2; int64_t ldz2, strideZ2;  // NULL: noise-free function values
  T* W; int64_t ldw, strideW;         // caller's weights (may be NULL)
  T* Wt; int64_t ldwt, strideWt;      // weights for the separate projection launch (NULL when the projection is fused)
  T* Y; int64_t ldy, strideY;         // may be NULL
  int32_t* info;
  int layout, noise_kind, prior_kind;  // prior_kind: PRIOR_UPPER_FACTOR or PRIOR_DIAGONAL here
  int D, N;
  int64_t S, B, nsb;                   // nsb = draw blocks per regressor
};

template <typename T>
__device__ __forceinline__ T wave_sum(T x) {  // xor butterfly with commutative adds: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// LAPACK-style status of regressor b: the factorisation's own, else the first non-positive diagonal entry (1-based), else 0.
template <typename T>
__device__ __forceinline__ int rand_batched_status(const RandBatchedArgs<T>& a, int64_t b, int lane) {
  if (a.chol_info) {
    const int ci = a.chol_info[b];
    if (ci) return ci;
  }
  const T* Ub = a.U + b * a.strideU;
  const bool diag = a.prior_kind == PRIOR_DIAGONAL;
  const int r0 = lane, r1 = lane + 64;
  const T d0 = r0 < a.D ? Ub[diag ? r0 : (int64_t)r0 * a.ldu + r0] : T(1);
  const T d1 = r1 < a.D ? Ub[diag ? r1 : (int64_t)r1 * a.ldu + r1] : T(1);
  const unsigned long long m0 = __ballot(!(d0 > T(0))), m1 = __ballot(!(d1 > T(0)));
  if (m0) return __builtin_ctzll(m0) + 1;
  if (m1) return __builtin_ctzll(m1) + 65;
  return 0;
}

// ---- weight solve (+ fused projection when FUSE) -------------------------------------------------------------------------------
// Lanes own rows r = lane and lane + 64 of z (NS draws each).  U is column-major upper, so column j (rows 0..j) is contiguous:
// the columns are streamed from last to first, CB at a time with the next block's loads in flight, and substituted column by
// column -- w_j = z_j / U_jj (z_j and U_jj broadcast by readlane), then z_i -= U_ij w_j for i < j.  No LDS: the D(D+1)/2 useful
// entries are read once per wave, and with one wave per regressor at S <= NS the whole batch is resident at once.
template <typename T, int NS, bool FUSE>
__global__ __launch_bounds__(kThreads) void rand_batched_solve_kernel(RandBatchedArgs<T> a) {
  constexpr int CB = 8;
  const int lane = threadIdx.x & 63;
  const int64_t ntask = a.B * a.nsb;
  const int D = a.D;
  const int r0 = lane, r1 = lane + 64;
  for (int64_t task = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); task < ntask; task += (int64_t)gridDim.x * kWaves) {
    const int64_t b = task / a.nsb;
    const int64_t s0 = (task % a.nsb) * NS;
    const int bad = rand_batched_status(a, b, lane);
    if (s0 == 0 && lane == 0) a.info[b] = bad;
    if (bad) continue;  // a failed regressor's outputs stay untouched
    const T* Ub = a.U + b * a.strideU;
    const T* Zb = a.Z1 + b * a.strideZ1;
    T z0[NS], z1[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int64_t sidx = s0 + k;
      const bool ok = sidx < a.S;
      z0[k] = (ok && r0 < D) ? Zb[sidx * a.ldz1 + r0] : T(0);
      z1[k] = (ok && r1 < D) ? Zb[sidx * a.ldz1 + r1] : T(0);
    }
    if (a.prior_kind == PRIOR_DIAGONAL) {  // w = mw + z / sqrt(d), as diag_sample_kernel
      const T q0 = r0 < D ? sqrt(Ub[r0]) : T(1), q1 = r1 < D ? sqrt(Ub[r1]) : T(1);
#pragma unroll
      for (int k = 0; k < NS; ++k) { z0[k] = z0[k] / q0; z1[k] = z1[k] / q1; }
    } else {
      T c0[CB], c1[CB], n0[CB], n1[CB];
      auto load = [&](int jt, T (&a0)[CB], T (&a1)[CB]) {
#pragma unroll
        for (int k = 0; k < CB; ++k) {
          const int j = jt - k;
          a0[k] = (j >= 0 && r0 <= j) ? Ub[(int64_t)j * a.ldu + r0] : T(0);
          a1[k] = (j >= 0 && r1 <= j) ? Ub[(int64_t)j * a.ldu + r1] : T(0);
        }
      };
      load(D - 1, c0, c1);
      for (int jt = D - 1; jt >= 0; jt -= CB) {
        if (jt - CB >= 0) load(jt - CB, n0, n1);
#pragma unroll
        for (int k = 0; k < CB; ++k) {
          const int j = jt - k;
          if (j < 0) break;
          const int lj = j & 63;
          const T ujj = (j < 64) ? readlane(c0[k], lj) : readlane(c1[k], lj);
          const T rinv = T(1) / ujj;
#pragma unroll
          for (int q = 0; q < NS; ++q) {
            const T zj = (j < 64) ? readlane(z0[q], lj) : readlane(z1[q], lj);
            const T wj = zj * rinv;
            z0[q] = r0 < j ? fused_madd(-c0[k], wj, z0[q]) : (r0 == j ? wj : z0[q]);
            z1[q] = r1 < j ? fused_madd(-c1[k], wj, z1[q]) : (r1 == j ? wj : z1[q]);
          }
        }
#pragma unroll
        for (int k = 0; k < CB; ++k) { c0[k] = n0[k]; c1[k] = n1[k]; }
      }
    }
    const T* mwb = a.mw + b * a.stridemw;
    const T m0 = r0 < D ? mwb[r0] : T(0), m1 = r1 < D ? mwb[r1] : T(0);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      z0[k] += m0;
      z1[k] += m1;
      const int64_t sidx = s0 + k;
      if (sidx >= a.S) continue;
      if (a.W) {
        T* Wb = a.W + b * a.strideW + sidx * a.ldw;
        if (r0 < D) Wb[r0] = z0[k];
        if (r1 < D) Wb[r1] = z1[k];
      }
      if (!FUSE && a.Wt) {
        T* Wb = a.Wt + b * a.strideWt + sidx * a.ldwt;
        if (r0 < D) Wb[r0] = z0[k];
        if (r1 < D) Wb[r1] = z1[k];
      }
    }
    if (!FUSE || !a.Y) continue;
    // fused projection (small N x S): y[n, s] = sum_d x[d, n] w[d, s], one fixed-order wave sum per output
    const T* Xb = a.X + b * a.strideX;
    const bool colv = a.layout == LAYOUT_COLVECS;
    for (int nb0 = 0; nb0 < a.N; nb0 += 64) {
      const int nn_end = min(64, a.N - nb0);
      T yv[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) yv[k] = T(0);
      for (int nn = 0; nn < nn_end; ++nn) {
        const int64_t n = nb0 + nn;
        const T x0 = r0 < D ? Xb[colv ? n * a.ldx + r0 : (int64_t)r0 * a.ldx + n] : T(0);
        const T x1 = r1 < D ? Xb[colv ? n * a.ldx + r1 : (int64_t)r1 * a.ldx + n] : T(0);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const T p = wave_sum(fused_madd(x1, z1[k], x0 * z0[k]));
          yv[k] = lane == nn ? p : yv[k];
        }
      }
      const int n = nb0 + lane;
      if (lane < nn_end) {
        T sd = T(0);
        if (a.Z2) {
          const T* sb = a.s + b * a.strides;
          sd = sqrt(a.noise_kind == NOISE_DIAGONAL ? sb[n] : sb[0]);
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const int64_t sidx = s0 + k;
          if (sidx >= a.S) continue;
          T v = yv[k];
          if (a.Z2) v += sd * a.Z2[b * a.strideZ2 + sidx * a.ldz2 + n];
          a.Y[b * a.strideY + sidx * a.ldy + n] = v;
        }
      }
    }
  }
}

// ---- separate projection: rand_project_* tiles over (input tiles x regressors, draw tiles) --------------------------------------
// blockIdx.x enumerates (tile, regressor) with the regressor fastest when X is shared (strideX == 0), so that the workgroups that
// run together read the same tile of X from L2; with one X per regressor the tiles of a regressor are consecutive.
template <typename T>
__device__ __forceinline__ bool rand_batched_tile(const RandBatchedArgs<T>& a, int ntn, int64_t reg0, int64_t nreg, int& tile,
                                                  int64_t& b) {
  const int64_t bx = blockIdx.x;
  if (a.strideX == 0) { b = reg0 + bx % nreg; tile = (int)(bx / nreg); }
  else                { b = reg0 + bx / ntn;  tile = (int)(bx % ntn); }
  return a.info[b] == 0;  // (written by rand_batched_solve_kernel, the launch before)
}

template <typename T>
__global__ __launch_bounds__(kThreads, 2) void rand_batched_project_mfma_kernel(RandBatchedArgs<T> a, int ntn, int64_t reg0, int64_t nreg) {
  int tile;
  int64_t b;
  if (!rand_batched_tile(a, ntn, reg0, nreg, tile, b)) return;
  rand_project_mfma_tile<T>(a.X + b * a.strideX, a.ldx, a.Wt + b * a.strideWt, a.ldwt, a.Z2 ? a.s + b * a.strides : nullptr,
                            a.noise_kind, a.Z2 ? a.Z2 + b * a.strideZ2 : nullptr, a.ldz2, a.Y + b * a.strideY, a.ldy, a.D, a.N, a.S,
                            tile, blockIdx.y);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void rand_batched_project_kernel(RandBatchedArgs<T> a, int ntn, int64_t reg0, int64_t nreg) {
  int tile;
  int64_t b;
  if (!rand_batched_tile(a, ntn, reg0, nreg, tile, b)) return;
  rand_project_tile<T>(a.X + b * a.strideX, a.ldx, a.layout, a.Wt + b * a.strideWt, a.ldwt, a.Z2 ? a.s + b * a.strides : nullptr,
                       a.noise_kind, a.Z2 ? a.Z2 + b * a.strideZ2 : nullptr, a.ldz2, a.Y + b * a.strideY, a.ldy, a.D, a.N, a.S,
                       tile, blockIdx.y);
}

// ---- D > 128: status of every regressor of a factor / diagonal prior (the per-regressor loop needs it before it starts) ---------
template <typename T>
__global__ __launch_bounds__(kThreads) void rand_batched_status_kernel(const T* __restrict__ U, int64_t ldu, int64_t strideU, int diag,
                                                                       int D, int64_t B, int32_t* __restrict__ info) {
  const int lane = threadIdx.x & 63;
  for (int64_t b = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); b < B; b += (int64_t)gridDim.x * kWaves) {
    const T* Ub = U + b * strideU;
    int bad = 0;
    for (int r0 = 0; r0 < D && !bad; r0 += 64) {
      const int r = r0 + lane;
      const T d = r < D ? Ub[diag ? r : (int64_t)r * ldu + r] : T(1);
      const unsigned long long m = __ballot(!(d > T(0)));
      if (m) bad = r0 + __builtin_ctzll(m) + 1;
    }
    if (lane == 0) info[b] = bad;
  }
}

}  // namespace blr
