// The tall-matrix panel sweep (D > 128).  A tall matrix  [ F ; rows ]  (column-major, DP columns) holds an already factored DP x DP
// block F on top and the rows to solve for below it; one 128-column panel at a time, every row x' becomes x'L^-T (forward) and then,
// where the caller wants A^-1 = L^-T L^-1 applied, x'L^-T L^-1 (backward).
//
//   TrsmCfg, trsm_prepare, trsm_sweep<T, BACK>   the LDS-resident sweep over 16-column chunks on MFMA, forward or backward: also the
//                                                core of marg_image_kernel (blr_marginals.hpp), marginals_mfma_kernel,
//                                                sample_weights_mfma_kernel and logpdf_grad_kernel (blr_large.hpp)
//   trsm_block_kernel / trsm_back_block_kernel   one panel step (forward / backward) for 64 rows per workgroup
//   factor_transpose_fill_kernel, factor_sym_fill_kernel, identity_rows_kernel, ainv_copy_kernel   fill and read the tall matrix
//
// The trailing update between two panel steps is gram_tile_kernel (blr_large.hpp); the host side of the whole sweep is TallSweep
// (blr_abi.hip).  Included by blr_large.hpp, below BlockVec and ws_shift, which the kernels here use: not a header to include alone.
#pragma once

namespace blr {

// ---- X <- X L_pp^-T for one block of RB rows below the diagonal block ------------------------------------------------
template <typename T>
struct TrsmCfg {
  static constexpr int RB = 64;                            // rows per workgroup (f32 at 128 rows needs 108 KB of LDS: cannot share a CU with a Gram workgroup)
  static constexpr int LDX = kPB + 1;                      // padded row stride of the X image (conflict-free)
  static constexpr int OFF_X = ((kPB * (kPB + 1) / 2) * (int)sizeof(T) + 15) & ~15;
  static constexpr int OFF_DI = OFF_X + RB * LDX * (int)sizeof(T);
  static constexpr int LDI = 17;                           // padded row stride of the 16 x 16 inverse blocks
  static constexpr int OFF_LI = (OFF_DI + kPB * (int)sizeof(T) + 15) & ~15;
  static constexpr int LDS_BYTES = ((OFF_LI + kPB * LDI * (int)sizeof(T)) + 15) & ~15;
};

// X <- X L^-T on an LDS-resident block: Xs[RB][LDX] rows, L packed lower in P, dinv = 1 / diag(L), Linv = scratch for
// the inverses of the 16 x 16 diagonal blocks of L; `nchunks` 16-column chunks.
// Rows are independent, so each wave owns its row tiles for the whole sweep and the chunk loop needs NO workgroup
// barrier: chunk J first receives  - sum_{K<J} X_K L_JK'  (MFMA, left-looking), then is multiplied by inv(L_JJ)' (MFMA
// again: the per-row substitution of the first version serialised 16 steps per chunk on the vector ALU behind two
// barriers).  The 16 x 16 inverses are formed once per block by 16 lanes each (forward substitution of a unit column).
template <typename T>
__device__ __forceinline__ void trsm_prepare(const T* __restrict__ P, const T* __restrict__ dinv, T* __restrict__ Linv, int nchunks,
                                             int tid) {
  using Cfg = TrsmCfg<T>;
  constexpr int LI = Cfg::LDI;
  if (tid < 16 * nchunks) {
    // column j of inv(L_JJ) by forward substitution, COLUMN-oriented: once x_k is known every pending row takes its update at
    // once (independent multiply-adds) -- the row-oriented form summed k < i terms one after the other for each i: a chain of
    // 136 dependent operations instead of 32
    const int j = tid & 15, j0 = 16 * (tid >> 4);
    T sacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) sacc[i] = (i == j) ? T(1) : T(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const T xk = sacc[k] * dinv[j0 + k];
      Linv[(j0 + k) * LI + j] = xk;
#pragma unroll
      for (int i = k + 1; i < 16; ++i) sacc[i] -= P[pidx(j0, j0) + i * j0 + (i * (i + 1)) / 2 + k] * xk;
    }
  }
  __syncthreads();
}

// element (row 16 (wave + kWaves t) + crow(lane, v), column 16 J + (lane & 15)) of Xs: where value v of the wave's accumulator
// tile t of chunk J lives
template <typename T>
__device__ __forceinline__ int trsm_acc_idx(int lane, int wave, int t, int v, int J) {
  return (16 * (wave + kWaves * t) + Mfma<T>::crow(lane, v)) * TrsmCfg<T>::LDX + 16 * J + (lane & 15);
}

// the sweep proper; Linv from trsm_prepare.  Ends with a workgroup barrier (Xs complete for everybody).
// BACK = false:  X <- X L^-T, chunks from the first to the last:  Y_J = (X_J - sum_{K<J} Y_K L_JK') inv(L_JJ)'.
// BACK = true:   X <- X L^-1 (the OTHER triangular solve: G L = Z), chunks from the last to the first:
//                G_J = (Z_J - sum_{K>J} G_K L_KJ) inv(L_JJ).  After the forward sweep this applies A^-1 = L^-T L^-1 to every row.
template <typename T, bool BACK>
__device__ __forceinline__ void trsm_sweep(T* __restrict__ Xs, const T* __restrict__ P, const T* __restrict__ Linv, int nchunks,
                                           int lane, int wave) {
  using Cfg = TrsmCfg<T>;
  using acc4 = typename Mfma<T>::acc4;
  constexpr int NT = Cfg::RB / 64;  // row tiles per wave
  constexpr int LI = Cfg::LDI;
  const int fr = lane & 15, fq = lane >> 4;
  for (int J = BACK ? nchunks - 1 : 0; BACK ? J >= 0 : J < nchunks; J += BACK ? -1 : 1) {
    acc4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[t][v] = Xs[trsm_acc_idx<T>(lane, wave, t, v, J)];
    for (int K = BACK ? J + 1 : 0; K < (BACK ? nchunks : J); ++K) {  // the chunks already solved
      T fl[4], fx[NT][4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if constexpr (BACK) fl[ks] = P[pidx(16 * K + 4 * ks + fq, 16 * J + fr)];  // B[k][j] = L[16K + k][16J + j]
        else fl[ks] = P[pidx(16 * J + fr, 16 * K + 4 * ks + fq)];                 // B[k][j] = L[16J + j][16K + k]
#pragma unroll
        for (int t = 0; t < NT; ++t) fx[t][ks] = Xs[(16 * (wave + kWaves * t) + fr) * Cfg::LDX + 16 * K + 4 * ks + fq];
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = Mfma<T>::mma(-fx[t][ks], fl[ks], acc[t]);
    }
    // C layout -> LDS -> A fragments (wave-local: LDS operations of one wave complete in order)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) Xs[trsm_acc_idx<T>(lane, wave, t, v, J)] = acc[t][v];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    acc4 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] = acc4{T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      // B[k][j] = inv(L_JJ)[k][j], read transposed by the forward sweep
      const T fi = BACK ? Linv[(16 * J + 4 * ks + fq) * LI + fr] : Linv[(16 * J + fr) * LI + 4 * ks + fq];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const T fu = Xs[(16 * (wave + kWaves * t) + fr) * Cfg::LDX + 16 * J + 4 * ks + fq];
        o[t] = Mfma<T>::mma(fu, fi, o[t]);
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) Xs[trsm_acc_idx<T>(lane, wave, t, v, J)] = o[t][v];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
}

template <typename T>
__device__ __forceinline__ void trsm_core(T* __restrict__ Xs, const T* __restrict__ P, const T* __restrict__ dinv,
                                          T* __restrict__ Linv, int nchunks, int tid, int lane, int wave) {
  trsm_prepare<T>(P, dinv, Linv, nchunks, tid);
  trsm_sweep<T, false>(Xs, P, Linv, nchunks, lane, wave);
}

template <typename T>
struct RowSqArgs {      // optional fused epilogue of the marginal stream: var_n = |Y_n|^2 + s_n   (:40-43)
  double* acc;          // [N] running row sums of squares (NULL: off); panel 0 writes, later panels add
  T* var; const T* s;   // last panel: var[n] = acc[n] + s_n
  int noise_kind, N, first, last;
  int64_t grp_ws, grp_s;  // blockIdx.y = regressor of a group: byte stride of acc / var, element stride of s
};

template <typename T>
__global__ __launch_bounds__(kThreads) void trsm_block_kernel(T* Abar, int64_t lda, int p, int row_begin, int nrows_total,
                                                              const int32_t* info, RowSqArgs<T> rs, int64_t grp_ws = 0) {
  __builtin_amdgcn_s_setprio(3);  // latency-critical chain kernel: issue ahead of co-resident Gram waves
  if (const int64_t g = blockIdx.y) {  // regressor of a group: the tall matrix by grp_ws bytes, one status word each
    Abar = ws_shift(Abar, g * grp_ws); info += g;
    rs.acc = ws_shift(rs.acc, g * rs.grp_ws); rs.var = ws_shift(rs.var, g * rs.grp_ws);
    if (rs.s) rs.s += g * rs.grp_s;
  }
  using Cfg = TrsmCfg<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* const P = reinterpret_cast<T*>(smem);                    // packed lower triangle of L_pp
  T* const Xs = reinterpret_cast<T*>(smem + Cfg::OFF_X);      // [RB][LDX]
  T* const dinv = reinterpret_cast<T*>(smem + Cfg::OFF_DI);   // 1 / L_pp[c][c]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int r0 = row_begin + blockIdx.x * Cfg::RB;            // first global row of this block
  const int nr = min(Cfg::RB, nrows_total - r0);              // a multiple of 128 rows in every caller: whole vectors
  const T* Lpp = Abar + (int64_t)p * kPB * lda + (int64_t)p * kPB;
  T* Xg = Abar + (int64_t)p * kPB * lda + r0;
  {
    // both blocks in flight at once (one round of memory latency instead of eight)
    BlockVec<T, kPB> lb;
    BlockVec<T, Cfg::RB> xb;
    lb.load(Lpp, lda, tid);
    xb.load(Xg, lda, tid);
    if (*info != 0) return;
    lb.to_packed_lower(P, tid);
    xb.to_rows(Xs, Cfg::LDX, nr, tid);
  }
  __syncthreads();
  if (tid < kPB) dinv[tid] = T(1) / P[pidx(tid, tid)];
  __syncthreads();

  trsm_core<T>(Xs, P, dinv, reinterpret_cast<T*>(smem + Cfg::OFF_LI), 8, tid, lane, wave);
  if (rs.acc != nullptr && tid < Cfg::RB) {
    // the finished 128 columns of this row never change again: fold them into the row's sum of squares now
    const int n = r0 - row_begin + tid;
    if (n < rs.N) {
      const T* xr = Xs + tid * Cfg::LDX;
      double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
#pragma unroll 8
      for (int c = 0; c < kPB; c += 4) {
        const double v0 = (double)xr[c], v1 = (double)xr[c + 1], v2 = (double)xr[c + 2], v3 = (double)xr[c + 3];
        q0 += v0 * v0; q1 += v1 * v1; q2 += v2 * v2; q3 += v3 * v3;
      }
      double tot = (q0 + q1) + (q2 + q3);
      if (!rs.first) tot += rs.acc[n];
      if (rs.last) rs.var[n] = (T)tot + ((rs.noise_kind == NOISE_DIAGONAL) ? rs.s[n] : rs.s[0]);
      else rs.acc[n] = tot;
    }
  }
  {
    using BV = BlockVec<T, Cfg::RB>;
#pragma unroll 4
    for (int u = 0; u < BV::NV; ++u) {
      const int vi = u * kThreads + tid;
      const int c = vi / BV::VPC, rr = (vi % BV::VPC) * BV::VEC;
      if (rr < nr) {
        typename BV::vecT o;
#pragma unroll
        for (int e = 0; e < BV::VEC; ++e) o[e] = Xs[(rr + e) * Cfg::LDX + c];
        *reinterpret_cast<typename BV::vecT*>(Xg + (int64_t)c * lda + rr) = o;
      }
    }
  }
}

// L = U' into the top DP x DP block of Ybar (lower, unit padding); U upper column-major (ldu)
template <typename T>
__global__ __launch_bounds__(kThreads) void factor_transpose_fill_kernel(const T* U, int64_t ldu, int D, int DP, T* Ybar,
                                                                         int64_t ldy) {
  __shared__ T tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;  // bx: row block of L, by: col block of L
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int ur = by + tx, uc = bx + k;  // U[ur, uc] = L[uc, ur]; coalesced along ur
    tile[k][tx] = (ur < D && uc < D && ur <= uc) ? U[(int64_t)uc * ldu + ur] : T(0);
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int row = bx + tx, col = by + k;  // L[row, col] = U[col, row] = tile[tx][k]
    if (row < DP && col < DP) {
      T v = tile[tx][k];
      if (row >= D || col >= D) v = (row == col) ? T(1) : T(0);
      if (row >= col) Ybar[(int64_t)col * ldy + row] = v;
    }
  }
}

// Tall matrix  [ F ; X' ; I ]  (ld = rows): F = the factor block with BOTH triangles filled (lower: L, upper: T = L'), the
// inputs as rows, and (for A^-1) the rows of the identity.  Forward panels (trsm_block_kernel + MFMA trailing updates, as
// in the marginal stream) turn every row x' into x'L^-T; backward panels (trsm_back_block_kernel + the same trailing
// update kernel reading the UPPER triangle of F as its second operand) turn that into x'L^-T L^-1 = x'A^-1.

// top block: lower triangle L = U', upper triangle U, unit padding
template <typename T>
__global__ __launch_bounds__(kThreads) void factor_sym_fill_kernel(const T* U, int64_t ldu, int D, int DP, T* Ybar, int64_t ldy, int64_t grp_U = 0,
                                                                   int64_t grp_ws = 0) {
  __shared__ T tile[32][33];
  if (const int64_t g = blockIdx.z) { U += g * grp_U; Ybar = ws_shift(Ybar, g * grp_ws); }  // regressor of a group
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int ur = by + tx, uc = bx + k;
    tile[k][tx] = (ur < D && uc < D && ur <= uc) ? U[(int64_t)uc * ldu + ur] : T(0);
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int row = bx + tx, col = by + k;  // L[row, col] = U[col, row] = tile[tx][k]
    if (row < DP && col < DP && row >= col) {
      T v = tile[tx][k];
      if (row >= D || col >= D) v = (row == col) ? T(1) : T(0);
      Ybar[(int64_t)col * ldy + row] = v;                  // lower (and diagonal)
      if (row > col) Ybar[(int64_t)row * ldy + col] = v;   // mirrored: element (col, row) of the upper triangle
    }
  }
}

// rows [row0, row0 + DP) of the tall matrix := identity
template <typename T>
__global__ __launch_bounds__(kThreads) void identity_rows_kernel(T* Ybar, int64_t ldy, int row0, int DP, int64_t grp_ws = 0) {
  Ybar = ws_shift(Ybar, (int64_t)blockIdx.y * grp_ws);
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < (int64_t)DP * DP; e += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(e / DP), r = (int)(e % DP);
    Ybar[(int64_t)c * ldy + row0 + r] = (r == c) ? T(1) : T(0);
  }
}

// X <- X L_pp^-1 for one block of RB rows (the backward panel step)
template <typename T>
__global__ __launch_bounds__(kThreads) void trsm_back_block_kernel(T* Abar, int64_t lda, int p, int row_begin, int nrows_total,
                                                                   const int32_t* info, int64_t grp_ws = 0) {
  if (const int64_t g = blockIdx.y) { Abar = ws_shift(Abar, g * grp_ws); info += g; }  // regressor of a group
  using Cfg = TrsmCfg<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* const P = reinterpret_cast<T*>(smem);
  T* const Xs = reinterpret_cast<T*>(smem + Cfg::OFF_X);
  T* const dinv = reinterpret_cast<T*>(smem + Cfg::OFF_DI);
  T* const Linv = reinterpret_cast<T*>(smem + Cfg::OFF_LI);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int r0 = row_begin + blockIdx.x * Cfg::RB;
  const int nr = min(Cfg::RB, nrows_total - r0);
  const T* Lpp = Abar + (int64_t)p * kPB * lda + (int64_t)p * kPB;
  T* Xg = Abar + (int64_t)p * kPB * lda + r0;
  {
    BlockVec<T, kPB> lb;
    BlockVec<T, Cfg::RB> xb;
    lb.load(Lpp, lda, tid);
    xb.load(Xg, lda, tid);
    if (*info != 0) return;
    lb.to_packed_lower(P, tid);
    xb.to_rows(Xs, Cfg::LDX, nr, tid);
  }
  __syncthreads();
  if (tid < kPB) dinv[tid] = T(1) / P[pidx(tid, tid)];
  __syncthreads();
  trsm_prepare<T>(P, dinv, Linv, 8, tid);
  trsm_sweep<T, true>(Xs, P, Linv, 8, lane, wave);
  {
    using BV = BlockVec<T, Cfg::RB>;
#pragma unroll 4
    for (int u = 0; u < BV::NV; ++u) {
      const int vi = u * kThreads + tid;
      const int c = vi / BV::VPC, rr = (vi % BV::VPC) * BV::VEC;
      if (rr < nr) {
        typename BV::vecT o;
#pragma unroll
        for (int e = 0; e < BV::VEC; ++e) o[e] = Xs[(rr + e) * Cfg::LDX + c];
        *reinterpret_cast<typename BV::vecT*>(Xg + (int64_t)c * lda + rr) = o;
      }
    }
  }
}

// A^-1 from the identity rows of the tall matrix
template <typename T>
__global__ __launch_bounds__(kThreads) void ainv_copy_kernel(const T* Ybar, int64_t ldy, int row0, int D, T* Ainv, int64_t ldai, int64_t grp_ws = 0,
                                                             int64_t grp_Ai = 0) {
  Ybar = ws_shift(Ybar, (int64_t)blockIdx.y * grp_ws); Ainv += (int64_t)blockIdx.y * grp_Ai;  // regressor of a group
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < (int64_t)D * D; e += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(e / D), r = (int)(e % D);
    Ainv[(int64_t)c * ldai + r] = Ybar[(int64_t)c * ldy + row0 + r];
  }
}

}  // namespace blr
