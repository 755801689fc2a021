// Columns 1 .. S-1 of a rank-k update / downdate of a RESIDENT multi-output state (blr_update_multi_factor_*,
// blr_downdate_multi_factor_*).
//
// Replaces reference test/bayesian_linear_regression.jl:49-70 ("repeated conditioning") and src/bayesian_linear_regression.jl:93 under
// MATRIX targets, and -- the downdate -- their inverse with :55-58 for the removed data.  The state is K17's: one upper factor T
// (A = T'T) and a D x S block M of means.  With W = X S^-1/2 the new precision A' = A +- W W' does not involve Y, so the factor T'
// is column 0's: the ordinary blr_update_factor_* / blr_downdate_factor_* of (X, Y[:, 0]) writes it, with m_0', logpdf_0 and info.
// What remains per further column c, with E_c = S^-1/2 (Y_c - X'm_c) against the column's mean BEFORE the call (upper sign: update):
//   b_c = W E_c       u_c = T'^-T b_c       m_c' = m_c +- T'^-1 u_c       quad_c = |E_c|^2 -+ |u_c|^2
//   logpdf_c = -1/2 [ k log 2pi + sum log s_i +- 2 sum_j log(T'_jj / T_jj) + quad_c ]
// The old diagonal of T (the log-determinant term) is saved by state_diag_kernel before column 0's call overwrites the factor.
//
// state_cols_kernel<T, DOWN>: grid (regressors, column passes), 256 threads; a pass takes kStateColsPerPass columns.  Per workgroup:
//   stream   the observations in chunks of kStateChunk = kSweepMaxK through LDS: thread (observation, column) forms the residual against the old
//            mean in double and adds its square to |E_c|^2; then wave w accumulates b_c for its columns w, w + 4, w + 8, w + 12 in
//            registers (in double: at fp32 the sum over k would otherwise carry the error of the call), lanes owning rows lane and
//            lane + 64 -- the layout of the solves, so b never goes through LDS.
//   solve    the finished factor as packed upper rows in LDS (the layout of rank1_sweep_kernel, over the stream's buffers); a wave
//            runs the forward and the back substitution of its (up to four) columns together: one chain of D steps, four independent
//            readlane + FMA strands in it.  The forward substitution reads row k of T' across the lanes (consecutive addresses); the
//            back substitution reads column k, where two lanes i, j share a bank only if i + j = 2 D + 1 (mod 64): at most two-way.
// fp32 only: the factor column 0's call leaves carries a relative error e_A of a few 1e-7, which m' = m +- d carries as e_A |d|: many
// times the size of m' when the new mean is small beside its correction.  state_save_kernel therefore keeps the whole factor of the
// state BEFORE the call; the kernel forms A m_c = T'(T m_c) and X S^-1 y_c in double and solves the normal equations
// A'm_c' = A m_c +- X S^-1 y_c as four more strands of the same chains (error e_A |m'|); per column the form whose solved vector is
// the smaller (max norm) is written.  The choice depends on the column's own data only.
// A regressor whose status is not 0 gets NaN evidences and nothing else.  Every sum has a fixed order and a column is computed from
// its own data only: its bits do not depend on B, on S, on its position (pass, wave, strand) or on the other columns.
//
// state_cols_global_kernel<T, DOWN> (D > 128; correct, not fast): one workgroup per (column, regressor), b in LDS (double), T' read
// from global memory -- a row-oriented forward substitution and a column-oriented back substitution, both along the columns of T'.
#pragma once
#include "blr_common.hpp"

namespace blr {

constexpr int kStateColsPerPass = 16;                      // columns of a pass: four per wave
constexpr int kStateColsPerWave = kStateColsPerPass / kWaves;
constexpr int kStateChunk = 16;                            // observations per staged chunk: kSweepMaxK (blr_update.hpp; asserted in blr_abi.hip)
constexpr int kStateHeader = 256 + 2 * 16 * 16 * 8;                          // LDS bytes in front of the stream / solve buffers: |E_c|^2 [16], sum log s, the chunk's residuals and scaled targets, [16][16] each (double)
static_assert(kStateColsPerPass * kStateChunk == kThreads, "one thread per (observation, column) of a chunk");

template <typename T>
struct StateColsArgs {
  const T* X; int64_t ldx, strideX; int layout;
  const T* Y; int64_t ldY, strideY;
  const T* s; int64_t strides; int noise_kind;
  T* M; int64_t ldm, strideM;          // in/out: columns 1 .. S-1 (column 0 is the single-column call's)
  const T* Tf; int64_t ldt, strideT;   // the factor AFTER column 0's call (upper triangle read)
  const T* diag0;                      // [B][D] diagonal of the factor BEFORE it (state_diag_kernel)
  const T* T0;                         // fp32 only: [B][D x D] (ld = D) the whole factor BEFORE it (state_save_kernel)
  const double* lp0;                   // [B] evidence of column 0
  const int32_t* info;                 // [B] status of column 0's call
  double* logpdf; int64_t stride_lp;
  int D, k, S;
};

__host__ __device__ constexpr int state_packed_elems(int D) { return (D + 1) * (D + 2) / 2; }  // rows j: columns j .. D, as rank1_sweep_kernel
inline size_t state_cols_lds_bytes(size_t elem, int D) {
  const size_t stream = ((size_t)kStateChunk * (D + 1) + (size_t)kStateColsPerPass * D) * elem;
  const size_t solve = (size_t)state_packed_elems(D) * elem;
  return kStateHeader + (stream > solve ? stream : solve);
}
inline size_t state_cols_global_lds_bytes(int D) { return 64 + (size_t)D * sizeof(double); }

// diag0[b][j] = T_b[j][j]: what the evidence of the further columns needs of the factor column 0's call is about to overwrite
template <typename T>
__global__ __launch_bounds__(kThreads) void state_diag_kernel(const T* Tf, int64_t ldt, int64_t strideT, int D, int64_t total, T* diag0) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / D, j = e - b * D;
  diag0[e] = Tf[b * strideT + j * ldt + j];
}

// T0w[b] = T_b (ld = D): the fp32 kernel forms A m_c = T'(T m_c) of the state before the call from it (see state_cols_kernel)
template <typename T>
__global__ __launch_bounds__(kThreads) void state_save_kernel(const T* Tf, int64_t ldt, int64_t strideT, int D, int64_t total, T* T0w) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / ((int64_t)D * D), r = e - b * (int64_t)D * D, c = r / D, j = r - c * D;
  if (j <= c) T0w[e] = Tf[b * strideT + c * ldt + j];
}

// T''u = b for the wave's columns: step k scales entry k and eliminates it from the rows below with row k of T' (R + off(k))
template <typename T, int C>
__device__ __forceinline__ void state_forward(const T* R, int D, int lane, T r0, T r1, T (&b0)[C], T (&b1)[C]) {
  const int i0 = lane, i1 = lane + 64;
  for (int kb = 0; kb < D; kb += 8) {
    T c0[8], c1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb + u;
      const int kk = k < D ? k : D - 1;
      const T* row = R + (kk * D - (kk * (kk - 1)) / 2);
      c0[u] = (k < D && i0 > k && i0 < D) ? row[i0] : T(0);
      c1[u] = (k < D && i1 > k && i1 < D) ? row[i1] : T(0);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb + u;
      if (k < D) {
        const bool lo = k < 64;
        const T rk = readlane(lo ? r0 : r1, k & 63);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const T uk = readlane(lo ? b0[c] : b1[c], k & 63) * rk;
          if (lane == (k & 63)) { if (lo) b0[c] = uk; else b1[c] = uk; }
          b0[c] = fused_madd(-c0[u], uk, b0[c]);
          b1[c] = fused_madd(-c1[u], uk, b1[c]);
        }
      }
    }
  }
}

// T'd = u, column-oriented: step k scales entry k and eliminates it from the rows above with column k of T'
template <typename T, int C>
__device__ __forceinline__ void state_backward(const T* R, int D, int lane, T r0, T r1, T (&b0)[C], T (&b1)[C]) {
  const int i0 = lane, i1 = lane + 64;
  const T* const row0 = R + (i0 * D - (i0 * (i0 - 1)) / 2);
  const T* const row1 = R + (i1 * D - (i1 * (i1 - 1)) / 2);
  for (int kb = D - 1; kb >= 0; kb -= 8) {
    T c0[8], c1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb - u;
      c0[u] = (k >= 0 && i0 < k) ? row0[k] : T(0);
      c1[u] = (k >= 0 && i1 < k) ? row1[k] : T(0);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb - u;
      if (k >= 0) {
        const bool lo = k < 64;
        const T rk = readlane(lo ? r0 : r1, k & 63);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const T dk = readlane(lo ? b0[c] : b1[c], k & 63) * rk;
          if (lane == (k & 63)) { if (lo) b0[c] = dk; else b1[c] = dk; }
          b0[c] = fused_madd(-c0[u], dk, b0[c]);
          b1[c] = fused_madd(-c1[u], dk, b1[c]);
        }
      }
    }
  }
}

template <typename T, bool DOWN>
__global__ __launch_bounds__(kThreads) void state_cols_kernel(StateColsArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KC = kStateChunk, W = kStateColsPerPass, C = kStateColsPerWave;
  // fp32: the factor column 0's call leaves carries an error e_A of a few 1e-7, and m' = m +- d carries it as e_A |d| -- many times
  // the yardstick of a column whose new mean is small beside its correction.  So the fp32 kernel also solves the normal equations
  // A'm' = A m +- X S^-1 y (right-hand side in double from the state BEFORE the call: error e_A |m'|) in the same chains, and keeps
  // per column the form whose solved vector is the smaller one.  NS strands per wave: the columns' d, then their m'.
  constexpr bool REFINE = sizeof(T) == 4;
  constexpr int NS = REFINE ? 2 * C : C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t reg = blockIdx.x;
  const int pass = blockIdx.y;
  const int D = a.D, k = a.k, LDX = D + 1;
  const int col_first = 1 + pass * W;
  const int ncols = min(W, a.S - col_first);  // (0 only when S == 1)
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  double* const lp_out = a.logpdf ? a.logpdf + reg * a.stride_lp : nullptr;

  if (lp_out && pass == 0 && tid == 0) lp_out[0] = a.lp0[reg];  // (NaN when column 0's call failed)
  if (a.info[reg] != 0) {  // (block-uniform) column 0's call left the state untouched: NaN evidences, nothing else
    if (lp_out && tid < ncols) lp_out[col_first + tid] = kNaN;
    return;
  }
  if (ncols <= 0) return;

  double* const qS = reinterpret_cast<double*>(smem);    // [W] |E_c|^2
  double* const logsS = qS + W;                          // sum log s_i
  // stream buffers
  T* const Xs = reinterpret_cast<T*>(smem + kStateHeader);  // [KC][LDX]
  T* const Ms = Xs + KC * LDX;                              // [W][D] the columns' means before the call
  double* const Es = reinterpret_cast<double*>(smem + 256);  // [KC][W] residuals, scaled twice: (y - x'm) / s
  double* const Ys = Es + KC * W;                            // [KC][W] y / s (fp32 only)
  // solve buffer (over the stream's)
  T* const R = reinterpret_cast<T*>(smem + kStateHeader);   // packed rows of T': element (j, col) at j D - j (j - 1) / 2 + col

  const BLR_GLOBAL T* const Xg = as_global(a.X + reg * a.strideX);
  const BLR_GLOBAL T* const Yg = as_global(a.Y + reg * a.strideY);
  const BLR_GLOBAL T* const sg = as_global(a.s + reg * a.strides);
  BLR_GLOBAL T* const Mg = as_global(a.M + reg * a.strideM);
  const bool diag = a.noise_kind == NOISE_DIAGONAL;

  for (int e = tid; e < ncols * D; e += kThreads) {
    const int c = e / D, d = e - c * D;
    Ms[e] = Mg[(int64_t)(col_first + c) * a.ldm + d];
  }
  if (wave == 0) {  // sum log s_i, lanes striding over the observations
    double logs = 0.0;
    if (diag) {
      for (int i = lane; i < k; i += kWave) logs += log((double)sg[i]);
      logs = wave_allreduce(logs);
    } else {
      logs = (double)k * log((double)sg[0]);
    }
    if (lane == 0) logsS[0] = logs;
  }

  const int oi = tid & (KC - 1), slot = tid >> 4;  // this thread's (observation of the chunk, column of the pass)
  const int i0 = lane, i1 = lane + 64;
  const bool has0 = i0 < D, has1 = i1 < D;
  double q = 0.0;
  double a0[C], a1[C];  // b_c of the wave's columns, rows lane and lane + 64: summed in double whatever the element type
  double g0[C], g1[C];  // fp32: X S^-1 y_c, then A m_c +- it
#pragma unroll
  for (int c = 0; c < C; ++c) a0[c] = a1[c] = g0[c] = g1[c] = 0.0;

  for (int n0 = 0; n0 < k; n0 += KC) {
    const int kc = min(KC, k - n0);
    __syncthreads();  // (the means are in LDS; the previous chunk has been read)
    for (int e = tid; e < kc * D; e += kThreads) {
      int i, d;
      if (a.layout == LAYOUT_COLVECS) { i = e / D; d = e - i * D; } else { d = e / kc; i = e - d * kc; }
      Xs[i * LDX + d] = a.layout == LAYOUT_COLVECS ? Xg[(int64_t)(n0 + i) * a.ldx + d] : Xg[(int64_t)d * a.ldx + n0 + i];
    }
    __syncthreads();
    {
      double ev = 0.0, yv = 0.0;
      if (oi < kc && slot < ncols) {
        double mu = 0.0;
        const T* const xr = Xs + oi * LDX;
        const T* const mr = Ms + slot * D;
        for (int d = 0; d < D; ++d) mu = __builtin_fma((double)xr[d], (double)mr[d], mu);
        const double sv = (double)(diag ? sg[n0 + oi] : sg[0]);  // (positive: column 0's call has checked it)
        const double rs = 1.0 / sqrt(sv);
        const double yy = (double)Yg[(int64_t)(col_first + slot) * a.ldY + n0 + oi];
        const double e = (yy - mu) * rs;
        q = __builtin_fma(e, e, q);
        ev = e * rs;
        yv = yy * rs * rs;
      }
      Es[oi * W + slot] = ev;
      if (REFINE) Ys[oi * W + slot] = yv;
    }
    __syncthreads();
    for (int i = 0; i < kc; ++i) {  // b_c += x_i (e_ic / sqrt(s_i)), observations in ascending order
      const double x0 = has0 ? (double)Xs[i * LDX + i0] : 0.0, x1 = has1 ? (double)Xs[i * LDX + i1] : 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double ev = Es[i * W + wave + kWaves * c];
        a0[c] = __builtin_fma(x0, ev, a0[c]);
        a1[c] = __builtin_fma(x1, ev, a1[c]);
        if (REFINE) {
          const double yv = Ys[i * W + wave + kWaves * c];
          g0[c] = __builtin_fma(x0, yv, g0[c]);
          g1[c] = __builtin_fma(x1, yv, g1[c]);
        }
      }
    }
  }
  // |E_c|^2: the 16 observation lanes of a column, fixed butterfly
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) q += __shfl_xor(q, m, 64);
  if (oi == 0) qS[slot] = q;
  __syncthreads();

  if (REFINE) {  // A m_c = T'(T m_c) from the factor before the call, in double: g_c = A m_c +- X S^-1 y_c
    const BLR_GLOBAL T* const T0g = as_global(a.T0 + reg * (int64_t)D * D);
    for (int e = tid; e < D * D; e += kThreads) {
      const int c = e / D, j = e - c * D;
      if (j <= c) R[j * D - (j * (j - 1)) / 2 + c] = T0g[e];
    }
    __syncthreads();
    if (wave < ncols) {
      const T* const row0 = R + (i0 * D - (i0 * (i0 - 1)) / 2);
      const T* const row1 = R + (i1 * D - (i1 * (i1 - 1)) / 2);
      T mo0[C], mo1[C];
      double t0v[C], t1v[C], h0[C], h1[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int sl = wave + kWaves * c;
        const BLR_GLOBAL T* const mcol = Mg + (int64_t)(col_first + (sl < ncols ? sl : 0)) * a.ldm;
        mo0[c] = has0 ? mcol[i0] : T(0);
        mo1[c] = has1 ? mcol[i1] : T(0);
        t0v[c] = t1v[c] = h0[c] = h1[c] = 0.0;
      }
      for (int j = 0; j < D; ++j) {  // t = T m: row i of T (columns j >= i)
        const double e0 = (has0 && j >= i0) ? (double)row0[j] : 0.0, e1 = (has1 && j >= i1) ? (double)row1[j] : 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double mj = (double)readlane(j < 64 ? mo0[c] : mo1[c], j & 63);
          t0v[c] = __builtin_fma(e0, mj, t0v[c]);
          t1v[c] = __builtin_fma(e1, mj, t1v[c]);
        }
      }
      for (int i = 0; i < D; ++i) {  // h = T't: row i of T across the lanes (columns >= i)
        const T* const row = R + (i * D - (i * (i - 1)) / 2);
        const double e0 = (has0 && i0 >= i) ? (double)row[i0] : 0.0, e1 = (has1 && i1 >= i) ? (double)row[i1] : 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double ti = readlane(i < 64 ? t0v[c] : t1v[c], i & 63);
          h0[c] = __builtin_fma(e0, ti, h0[c]);
          h1[c] = __builtin_fma(e1, ti, h1[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        g0[c] = DOWN ? h0[c] - g0[c] : h0[c] + g0[c];
        g1[c] = DOWN ? h1[c] - g1[c] : h1[c] + g1[c];
      }
    }
    __syncthreads();
  }
  // the finished factor -> packed rows
  const BLR_GLOBAL T* const Tg = as_global(a.Tf + reg * a.strideT);
  for (int e = tid; e < D * D; e += kThreads) {
    const int c = e / D, j = e - c * D;
    if (j <= c) R[j * D - (j * (j - 1)) / 2 + c] = Tg[(int64_t)c * a.ldt + j];
  }
  __syncthreads();
  if (wave >= ncols) return;  // (no barrier below)

  const T t0 = has0 ? R[i0 * D - (i0 * (i0 - 1)) / 2 + i0] : T(1), t1 = has1 ? R[i1 * D - (i1 * (i1 - 1)) / 2 + i1] : T(1);
  const T r0 = has0 ? T(1) / t0 : T(0), r1 = has1 ? T(1) / t1 : T(0);
  const BLR_GLOBAL T* const dg = as_global(a.diag0 + reg * D);
  double dld = (has0 ? log((double)t0) - log((double)dg[i0]) : 0.0) + (has1 ? log((double)t1) - log((double)dg[i1]) : 0.0);
  dld = wave_allreduce(dld);  // sum_j log(T'_jj / T_jj)

  T b0[NS], b1[NS];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    b0[c] = (T)a0[c]; b1[c] = (T)a1[c];
    if (REFINE) { b0[C + c] = (T)g0[c]; b1[C + c] = (T)g1[c]; }
  }
  state_forward<T, NS>(R, D, lane, r0, r1, b0, b1);
  double uu[C];
#pragma unroll
  for (int c = 0; c < C; ++c) uu[c] = wave_allreduce(__builtin_fma((double)b0[c], (double)b0[c], (double)b1[c] * (double)b1[c]));
  state_backward<T, NS>(R, D, lane, r0, r1, b0, b1);

  const double kLog2Pi = 1.8378770664093454835606594728112;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int sl = wave + kWaves * c;
    if (sl < ncols) {
      BLR_GLOBAL T* const mcol = Mg + (int64_t)(col_first + sl) * a.ldm;
      bool normal = false;  // (wave-uniform)
      if (REFINE) {
        float nd = fmaxf(has0 ? fabsf((float)b0[c]) : 0.f, has1 ? fabsf((float)b1[c]) : 0.f);
        float nm = fmaxf(has0 ? fabsf((float)b0[NS - C + c]) : 0.f, has1 ? fabsf((float)b1[NS - C + c]) : 0.f);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { nd = fmaxf(nd, __shfl_xor(nd, m, 64)); nm = fmaxf(nm, __shfl_xor(nm, m, 64)); }
        normal = nm < nd;
      }
      if (normal) {
        if (has0) mcol[i0] = b0[NS - C + c];
        if (has1) mcol[i1] = b1[NS - C + c];
      } else {
        if (has0) mcol[i0] = DOWN ? mcol[i0] - b0[c] : mcol[i0] + b0[c];
        if (has1) mcol[i1] = DOWN ? mcol[i1] - b1[c] : mcol[i1] + b1[c];
      }
      if (lp_out && lane == 0) {
        const double quad = DOWN ? qS[sl] + uu[c] : qS[sl] - uu[c];
        const double ld2 = DOWN ? -2.0 * dld : 2.0 * dld;
        lp_out[col_first + sl] = -0.5 * ((double)k * kLog2Pi + logsS[0] + ld2 + quad);
      }
    }
  }
}

// D > 128: grid (columns 1 .. S-1, regressors of the launch); a.* point at the launch's first regressor
template <typename T, bool DOWN>
__global__ __launch_bounds__(kThreads) void state_cols_global_kernel(StateColsArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int64_t reg = blockIdx.y;
  const int col = 1 + (int)blockIdx.x;
  const int D = a.D, k = a.k;
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  double* const lp_out = a.logpdf ? a.logpdf + reg * a.stride_lp : nullptr;
  if (a.info[reg] != 0) {
    if (lp_out && tid == 0) lp_out[col] = kNaN;
    return;
  }
  double* const scr = reinterpret_cast<double*>(smem);  // [kWaves] of block_allreduce
  double* const bv = reinterpret_cast<double*>(smem + 64);  // [D] b, then u, then d: in double whatever the element type
  const T* const Xg = a.X + reg * a.strideX;
  const T* const yg = a.Y + reg * a.strideY + (int64_t)col * a.ldY;
  const T* const sg = a.s + reg * a.strides;
  const T* const Tg = a.Tf + reg * a.strideT;
  T* const mg = a.M + reg * a.strideM + (int64_t)col * a.ldm;
  const bool diag = a.noise_kind == NOISE_DIAGONAL, colvecs = a.layout == LAYOUT_COLVECS;
  for (int d = tid; d < D; d += kThreads) bv[d] = 0.0;
  double q = 0.0, logs = 0.0;
  for (int i = 0; i < k; ++i) {
    double part = 0.0;
    for (int d = tid; d < D; d += kThreads) {
      const T x = colvecs ? Xg[(int64_t)i * a.ldx + d] : Xg[(int64_t)d * a.ldx + i];
      part = __builtin_fma((double)x, (double)mg[d], part);
    }
    const double mu = block_allreduce(part, scr, tid);
    const double sv = (double)(diag ? sg[i] : sg[0]);
    const double rs = 1.0 / sqrt(sv);
    const double e = ((double)yg[i] - mu) * rs;
    q = __builtin_fma(e, e, q);
    logs += log(sv);
    const double ev = e * rs;
    for (int d = tid; d < D; d += kThreads) {
      const T x = colvecs ? Xg[(int64_t)i * a.ldx + d] : Xg[(int64_t)d * a.ldx + i];
      bv[d] = __builtin_fma((double)x, ev, bv[d]);
    }
  }
  __syncthreads();
  // T''u = b, row-oriented: u_i = (b_i - sum_{j < i} T'_ji u_j) / T'_ii, column i of T' being contiguous
  for (int i = 0; i < D; ++i) {
    const T* const tc = Tg + (int64_t)i * a.ldt;
    double part = 0.0;
    for (int j = tid; j < i; j += kThreads) part = __builtin_fma((double)tc[j], bv[j], part);
    const double sum = block_allreduce(part, scr, tid);
    if (tid == 0) bv[i] = (bv[i] - sum) / (double)tc[i];
    __syncthreads();
  }
  double part = 0.0, dpart = 0.0;
  const T* const dg = a.diag0 + reg * D;
  for (int j = tid; j < D; j += kThreads) {
    part = __builtin_fma(bv[j], bv[j], part);
    dpart += log((double)Tg[(int64_t)j * a.ldt + j]) - log((double)dg[j]);
  }
  const double uu = block_allreduce(part, scr, tid);
  const double dld = block_allreduce(dpart, scr, tid);
  // T'd = u, column-oriented
  for (int j = D - 1; j >= 0; --j) {
    const T* const tc = Tg + (int64_t)j * a.ldt;
    const double dj = bv[j] / (double)tc[j];
    __syncthreads();
    for (int i = tid; i < j; i += kThreads) bv[i] = __builtin_fma(-(double)tc[i], dj, bv[i]);
    if (tid == 0) bv[j] = dj;
    __syncthreads();
  }
  for (int d = tid; d < D; d += kThreads) mg[d] = (T)(DOWN ? (double)mg[d] - bv[d] : (double)mg[d] + bv[d]);
  if (lp_out && tid == 0) {
    const double kLog2Pi = 1.8378770664093454835606594728112;
    const double quad = DOWN ? q + uu : q - uu;
    const double ld2 = DOWN ? -2.0 * dld : 2.0 * dld;
    lp_out[col] = -0.5 * ((double)k * kLog2Pi + logs + ld2 + quad);
  }
}

// the instantiations the library uses, defined in blr_state_cols.hip (state_save_kernel: fp32 only)
extern template __global__ void state_cols_kernel<double, false>(StateColsArgs<double>);
extern template __global__ void state_cols_kernel<double, true>(StateColsArgs<double>);
extern template __global__ void state_cols_kernel<float, false>(StateColsArgs<float>);
extern template __global__ void state_cols_kernel<float, true>(StateColsArgs<float>);
extern template __global__ void state_cols_global_kernel<double, false>(StateColsArgs<double>);
extern template __global__ void state_cols_global_kernel<double, true>(StateColsArgs<double>);
extern template __global__ void state_cols_global_kernel<float, false>(StateColsArgs<float>);
extern template __global__ void state_cols_global_kernel<float, true>(StateColsArgs<float>);
extern template __global__ void state_diag_kernel<double>(const double*, int64_t, int64_t, int, int64_t, double*);
extern template __global__ void state_diag_kernel<float>(const float*, int64_t, int64_t, int, int64_t, float*);
extern template __global__ void state_save_kernel<float>(const float*, int64_t, int64_t, int, int64_t, float*);

}  // namespace blr
