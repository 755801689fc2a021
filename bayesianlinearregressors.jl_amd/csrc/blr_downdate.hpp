// Rank-k DOWNDATE of a resident posterior state: the inverse of blr_update.hpp (forget observations).
//
//   reference test/bayesian_linear_regression.jl:49-70   "repeated conditioning" -- the call removes what a conditioning added
//   reference src/bayesian_linear_regression.jl:55-58    logpdf, reported for the REMOVED data given the data that remains
//
// State: mean m [D] and upper factor T of the precision (A = T'T).  k observations (x_i, y_i, s_i) that the state contains
// leave it:  T''T' = T'T - sum w_i w_i',  w_i = x_i / sqrt(s_i).  As in the update the mean travels as an offset d from the
// ORIGINAL mean (m' = m + d, right-hand side u starting at 0, e_i = (y_i - x_i'm) / sqrt(s_i)); k = 0 leaves both bit-for-bit.
// Per observation, the mirror of the update's Givens sweep (LINPACK dchdd):
//   1. a = T^-T w (forward solve; prefix-consistent: the leading minor of order j of the downdated precision is positive
//      definite iff sum_{l<=j} a_l^2 < 1, so the first j where that fails is the LAPACK-style info);
//   2. alpha^2 = 1 - a'a (double);  zeta = (e - a'u) / alpha (double) -- the standardised residual of the observation given the
//      data that remains;
//   3. D rotations, bottom up, with Q [a; alpha] = e_last.  Their coefficients come from suffix sums instead of dchdd's serial
//      chain: alpha_j^2 = alpha^2 + sum_{l>=j} a_l^2, c_j = alpha_{j+1} / alpha_j, s_j = a_j / alpha_j (a scan, in double);
//   4. Q applied to [T | u] stacked over [0 | zeta]; column c meets only rotations j <= c, so COLUMNS ARE INDEPENDENT:
//        t = c_j xx + s_j r_jc,  r_jc = c_j r_jc - s_j xx,  xx = t   (j = c .. 0, xx = 0, or zeta for the u column).
//      The new diagonal is c_j T_jj > 0 (xx is still 0 when a column meets its own row): no sign normalisation is needed.
// At the end d = T'^-1 u' and  log p(y_k | rest) = -1/2 [k log 2pi + sum log s_i + 2 sum_j log(T_jj / T'_jj) + sum zeta_i^2].
// Nothing is written back unless every observation was removed: a failed regressor's state is bit-for-bit untouched.
//
// Two kernels, one algorithm:
//   downdate_lds_kernel (D <= 128): one workgroup per regressor, [T | u] packed in LDS as in rank1_sweep_kernel (71 KB at fp64
//     D = 128: two workgroups per CU).  Wave 0 runs the forward solve (a serial chain of D readlane + FMA steps) and the scans;
//     all four waves then apply the rotations, one column per thread.
//   downdate_g_* (any D up to the library's 8192; option NO_DOWNDATE_LDS forces it at D <= 128): the state is copied into a
//     ROW-major workspace (coalesced rows for the solve and the rotations, and the caller's state untouched until the end),
//     then two launches per observation: the blocked forward solve + scans (one workgroup per regressor), and the rotations
//     spread over ceil((D + 1) / 256) workgroups per regressor.  A blocked back substitution and the copy back close the call.
#pragma once
#include "blr_common.hpp"
#include "blr_update.hpp"  // SweepArgs: the same operands as the update

namespace blr {

constexpr int kDowndateLdsMaxD = 128;

__device__ __forceinline__ double wave_scan_incl(double x, int lane) {  // inclusive prefix sum over the 64 lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double v = __shfl_up(x, o, 64);
    if (lane >= o) x += v;
  }
  return x;
}
__device__ __forceinline__ double wave_rscan_incl(double x, int lane) {  // inclusive suffix sum: lanes lane..63
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double v = __shfl_down(x, o, 64);
    if (lane + o < 64) x += v;
  }
  return x;
}

__host__ __device__ constexpr int downdate_lds_scalars(int D, int item) { return ((((D + 1) * (D + 2) / 2 + 3 * (D + 1)) * item) + 15) & ~15; }
template <typename T>
__host__ __device__ constexpr int downdate_lds_bytes(int D) { return downdate_lds_scalars(D, (int)sizeof(T)) + 64; }

// The downdate of ONE regressor by its workgroup: state `reg` of a's arrays, its k observations at Xg / yg / sg (sg: k variances
// under diagonal noise, one otherwise).  a.X, a.y, a.s, their strides and a.k are not read here: downdate_lds_kernel takes the
// slice from them, downdate_ragged_kernel (blr_revise_ragged.hpp) from the packed arrays and `offsets`.  k must be uniform over the
// workgroup: it bounds the loop whose barriers every wave meets, and iscr[1] -- read by every wave after the same barrier -- is
// the loop's only other exit.
template <typename T>
__device__ __forceinline__ void downdate_lds_body(char* smem, const SweepArgs<T>& a, int64_t reg, const T* Xg, const T* yg, const T* sg, int k) {
  const int D = a.D, tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  T* const R = reinterpret_cast<T*>(smem);                // packed rows: row j at off(j), columns j..D (column D = u_j)
  T* const mv = R + (D + 1) * (D + 2) / 2;                // m [D] (the ORIGINAL mean; the offset d goes to column D)
  T* const cs = mv + (D + 1);                             // rotation cosines c_j
  T* const sn = cs + (D + 1);                             // rotation sines s_j
  double* const dsc = reinterpret_cast<double*>(smem + downdate_lds_scalars(D, (int)sizeof(T)));  // [0] zeta
  int* const iscr = reinterpret_cast<int*>(dsc + 4);      // [0] first bad diagonal, [1] status
  auto off = [&](int j) { return j * (D + 1) - (j * (j - 1)) / 2 - j; };  // R[off(j) + col] = element (j, col)
  const T* Tg = a.Tf + reg * a.strideT;
  T* mg = a.mw + reg * a.stridemw;
  const bool diag = a.noise_kind == NOISE_DIAGONAL;
  if (tid == 0) { iscr[0] = 0x7fffffff; iscr[1] = 0; }
  __syncthreads();
  for (int e = tid; e < D * D; e += kThreads) {
    const int c = e / D, j = e - c * D;
    if (j <= c) {
      const T v = Tg[(int64_t)c * a.ldt + j];
      R[off(j) + c] = v;
      if (j == c && !(v > T(0))) atomicMin(&iscr[0], c + 1);
    }
  }
  for (int j = tid; j < D; j += kThreads) { R[off(j) + D] = T(0); mv[j] = mg[j]; }
  const int c0 = lane, c1 = lane + 64;
  const bool has0 = c0 < D, has1 = c1 < D;
  double logd0 = 0.0, logs = 0.0, quad = 0.0;
  if (wave == 0) {
    // the noise is checked for all k observations before any is removed (reference :79 comes before :86)
    int bad_noise = 0x7fffffff;
    for (int i = lane; i < k; i += 64) {
      const T si = diag ? sg[i] : sg[0];
      if (!(si > T(0)) && bad_noise == 0x7fffffff) bad_noise = i + 1;
      logs += log((double)(si > T(0) ? si : T(1)));
    }
    logs = wave_allreduce(logs);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(bad_noise, m, 64); bad_noise = o < bad_noise ? o : bad_noise; }
    if (lane == 0 && bad_noise != 0x7fffffff) iscr[1] = bad_noise;
  }
  __syncthreads();
  if (iscr[0] != 0x7fffffff) { if (tid == 0) iscr[1] = iscr[0]; }  // a bad factor wins over a bad variance
  __syncthreads();
  const int st0 = iscr[1];
  if (wave == 0 && st0 == 0) {
    for (int j = lane; j < D; j += 64) logd0 += log((double)R[off(j) + j]);
    logd0 = wave_allreduce(logd0);
  }
  __syncthreads();  // (st0 read by every wave before wave 0 may write the status again)
  // iscr[1] changes only in wave 0 between the two barriers of an iteration and is read by all after the first: uniform
  for (int i = 0; i < (st0 == 0 ? k : 0); ++i) {
    if (wave == 0) {
      const T si = diag ? sg[i] : sg[0];
      const T rs = fast_rsqrt(si);
      T w0 = T(0), w1 = T(0);
      if (has0) w0 = (a.layout == LAYOUT_COLVECS) ? Xg[(int64_t)i * a.ldx + c0] : Xg[(int64_t)c0 * a.ldx + i];
      if (has1) w1 = (a.layout == LAYOUT_COLVECS) ? Xg[(int64_t)i * a.ldx + c1] : Xg[(int64_t)c1 * a.ldx + i];
      double mu = (double)w0 * (double)(has0 ? mv[c0] : T(0)) + (double)w1 * (double)(has1 ? mv[c1] : T(0));
      mu = wave_allreduce(mu);
      w0 *= rs; w1 *= rs;
      const double e = ((double)yg[i] - mu) * (double)rs;
      // a = T^-T w, column-oriented: a_j = w_j / T_jj, then w_c -= T_jc a_j for c > j (row j of T: contiguous in LDS)
      const T rd0 = has0 ? fast_rcp(R[off(c0) + c0]) : T(0), rd1 = has1 ? fast_rcp(R[off(c1) + c1]) : T(0);
      for (int j = 0; j < D; ++j) {
        const T* rw = R + off(j);
        const T aj = (j < 64) ? readlane(w0, j) * readlane(rd0, j) : readlane(w1, j - 64) * readlane(rd1, j - 64);
        if (lane == (j & 63)) { if (j < 64) w0 = aj; else w1 = aj; }
        if (has0 && c0 > j) w0 = fused_madd(-rw[c0], aj, w0);
        if (has1 && c1 > j) w1 = fused_madd(-rw[c1], aj, w1);
      }
      // prefix sums of a^2 (failure index), suffix sums (rotation coefficients), a'u -- all in double
      const double q0 = (double)w0 * (double)w0, q1 = (double)w1 * (double)w1;
      const double P0 = wave_scan_incl(q0, lane);
      const double P1 = readlane(P0, 63) + wave_scan_incl(q1, lane);
      const double alpha2 = 1.0 - readlane(P1, 63);
      const double Q1 = wave_rscan_incl(q1, lane);
      const double Q0 = readlane(Q1, 0) + wave_rscan_incl(q0, lane);
      // sums over l > c: the next lane's suffix (the shuffles run on every lane: a lane that sits out a shuffle reads as 0)
      const double Q0s = __shfl_down(Q0, 1, 64), Q1s = __shfl_down(Q1, 1, 64), Q1all = readlane(Q1, 0);
      const double Q0n = lane < 63 ? Q0s : Q1all;
      const double Q1n = lane < 63 ? Q1s : 0.0;
      const double atu = wave_allreduce((double)w0 * (double)(has0 ? R[off(c0) + D] : T(0)) +
                                        (double)w1 * (double)(has1 ? R[off(c1) + D] : T(0)));
      if (!(alpha2 > 0.0)) {
        const uint64_t m0 = __ballot(has0 && !(P0 < 1.0)), m1 = __ballot(has1 && !(P1 < 1.0));
        if (lane == 0) iscr[1] = m0 ? __ffsll((unsigned long long)m0) : m1 ? 64 + __ffsll((unsigned long long)m1) : D;
      } else {
        const double al0 = sqrt(alpha2 + Q0), al1 = sqrt(alpha2 + Q1);
        if (has0) { cs[c0] = (T)(sqrt(alpha2 + Q0n) / al0); sn[c0] = (T)((double)w0 / al0); }
        if (has1) { cs[c1] = (T)(sqrt(alpha2 + Q1n) / al1); sn[c1] = (T)((double)w1 / al1); }
        const double zeta = (e - atu) / sqrt(alpha2);
        quad += zeta * zeta;
        if (lane == 0) dsc[0] = zeta;
      }
    }
    __syncthreads();
    if (iscr[1] != 0) break;
    // the rotations, one column per thread (column D = the right-hand side u, entering with zeta below it)
    if (tid <= D) {
      const int c = tid;
      T* const col = R + c;
      T xx = (c == D) ? (T)dsc[0] : T(0);
      int j = c < D - 1 ? c : D - 1;
      T r = col[off(j)];
      for (; j >= 0; --j) {
        const T rn = j > 0 ? col[off(j - 1)] : T(0);
        const T cj = cs[j], sj = sn[j];
        col[off(j)] = cj * r - sj * xx;
        xx = cj * xx + sj * r;
        r = rn;
      }
    }
    __syncthreads();
  }
  const int bad = iscr[1];
  double logpdf = 0.0;
  if (wave == 0 && bad == 0) {
    // d = T'^-1 u': the update's column-oriented back substitution, then m' = m + d
    T u0 = has0 ? R[off(c0) + D] : T(0), u1 = has1 ? R[off(c1) + D] : T(0);
    const T r0 = has0 ? fast_rcp(R[off(c0) + c0]) : T(0), r1 = has1 ? fast_rcp(R[off(c1) + c1]) : T(0);
    double logd1 = (has0 ? log((double)R[off(c0) + c0]) : 0.0) + (has1 ? log((double)R[off(c1) + c1]) : 0.0);
    logd1 = wave_allreduce(logd1);
    for (int j = D - 1; j >= 0; --j) {
      const T dj = (j < 64) ? readlane(u0, j) * readlane(r0, j) : readlane(u1, j - 64) * readlane(r1, j - 64);
      if (lane == (j & 63)) { if (j < 64) u0 = dj; else u1 = dj; }
      if (c0 < j) u0 = fused_madd(-R[off(c0) + j], dj, u0);
      if (c1 < j) u1 = fused_madd(-R[off(c1) + j], dj, u1);
    }
    if (has0) mg[c0] = mv[c0] + u0;
    if (has1) mg[c1] = mv[c1] + u1;
    const double kLog2Pi = 1.8378770664093454835606594728112;
    logpdf = -0.5 * ((double)k * kLog2Pi + logs + 2.0 * (logd0 - logd1) + quad);
  }
  if (bad == 0) {
    for (int e = tid; e < D * D; e += kThreads) {
      const int c = e / D, j = e - c * D;
      if (j <= c) a.Tf[reg * a.strideT + (int64_t)c * a.ldt + j] = R[off(j) + c];
    }
  }
  if (tid == 0) {
    a.info[reg] = bad;
    if (a.logpdf) a.logpdf[reg] = bad ? __longlong_as_double(0x7ff8000000000000LL) : logpdf;
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void downdate_lds_kernel(SweepArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t reg = blockIdx.x;
  downdate_lds_body<T>(smem, a, reg, a.X + reg * a.strideX, a.y + reg * a.stridey, a.s + reg * a.strides, a.k);
}

// ---- global-memory route -------------------------------------------------------------------------------------------------
// Workspace of regressor r (ws.* + r * stride): W = the state's factor ROW-major (D x D, element (j, c) at j * D + c, only
// j <= c is used), u [D], cs [D], sn [D]; sc [4] doubles: log-sum of the variances, log det T (before), sum zeta^2, zeta;
// st: the status (0 while every observation so far was removed).
template <typename T>
struct DowndateWs {
  T *W, *u, *cs, *sn;
  int64_t strideW, stridev;
  double* sc;
  int* st;
};

constexpr int kDdTile = 64;

// copy between the caller's column-major factor and the row-major workspace; tile (rb, cb) of the upper triangle per workgroup
template <typename T, bool TO_WS>
__global__ __launch_bounds__(kThreads) void downdate_g_copy_kernel(SweepArgs<T> a, DowndateWs<T> w) {
  __shared__ T tile[kDdTile][kDdTile + 1];
  const int D = a.D, tid = threadIdx.x, nt = (D + kDdTile - 1) / kDdTile;
  const int64_t reg = blockIdx.x;
  const int rb = blockIdx.y / nt, cb = blockIdx.y - rb * nt;
  if (rb > cb) return;
  if (!TO_WS && w.st[reg] != 0) return;
  const int j0 = rb * kDdTile, c0 = cb * kDdTile;
  T* Tg = a.Tf + reg * a.strideT;
  T* W = w.W + reg * w.strideW;
  const int l = tid & 63;
  for (int q = tid >> 6; q < kDdTile; q += kWaves) {  // q: column (caller side) or row (workspace side) within the tile
    if (TO_WS) {
      const int j = j0 + l, c = c0 + q;
      if (j < D && c < D && j <= c) tile[q][l] = Tg[(int64_t)c * a.ldt + j];
    } else {
      const int j = j0 + q, c = c0 + l;
      if (j < D && c < D && j <= c) tile[l][q] = W[(int64_t)j * D + c];
    }
  }
  __syncthreads();
  for (int q = tid >> 6; q < kDdTile; q += kWaves) {
    if (TO_WS) {
      const int j = j0 + q, c = c0 + l;
      if (j < D && c < D && j <= c) W[(int64_t)j * D + c] = tile[l][q];
    } else {
      const int j = j0 + l, c = c0 + q;
      if (j < D && c < D && j <= c) Tg[(int64_t)c * a.ldt + j] = tile[q][l];
    }
  }
}

// checks in the reference's order (factor, then noise), log-sums, u = 0
template <typename T>
__global__ __launch_bounds__(kThreads) void downdate_g_prep_kernel(SweepArgs<T> a, DowndateWs<T> w) {
  __shared__ double dscr[kWaves];
  __shared__ int iscr[kWaves];
  const int D = a.D, tid = threadIdx.x;
  const int64_t reg = blockIdx.x;
  const T* Tg = a.Tf + reg * a.strideT;
  const T* sg = a.s + reg * a.strides;
  const bool diag = a.noise_kind == NOISE_DIAGONAL;
  int bf = 0x7fffffff, bn = 0x7fffffff;
  double ld = 0.0, ls = 0.0;
  for (int j = tid; j < D; j += kThreads) {
    const T v = Tg[(int64_t)j * a.ldt + j];
    if (!(v > T(0)) && bf == 0x7fffffff) bf = j + 1;
    ld += log((double)(v > T(0) ? v : T(1)));
    w.u[reg * w.stridev + j] = T(0);
  }
  for (int i = tid; i < a.k; i += kThreads) {
    const T si = diag ? sg[i] : sg[0];
    if (!(si > T(0)) && bn == 0x7fffffff) bn = i + 1;
    ls += log((double)(si > T(0) ? si : T(1)));
  }
  bf = block_min_int(bf, iscr, tid);
  bn = block_min_int(bn, iscr, tid);
  ld = block_allreduce(ld, dscr, tid);
  ls = block_allreduce(ls, dscr, tid);
  if (tid == 0) {
    w.st[reg] = bf != 0x7fffffff ? bf : bn != 0x7fffffff ? bn : 0;
    w.sc[reg * 4 + 0] = ls;
    w.sc[reg * 4 + 1] = ld;
    w.sc[reg * 4 + 2] = 0.0;
    w.sc[reg * 4 + 3] = 0.0;
  }
}

template <typename T>
__host__ __device__ constexpr int downdate_g_solve_lds(int D) { return ((D * (int)sizeof(T) + 15) & ~15) + 2 * kThreads * 8 + 64; }

// observation i: blocked forward solve a = T^-T w, scans, rotation coefficients and zeta (one workgroup per regressor)
template <typename T>
__global__ __launch_bounds__(kThreads) void downdate_g_solve_kernel(SweepArgs<T> a, DowndateWs<T> w, int i) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int D = a.D, tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int64_t reg = blockIdx.x;
  if (w.st[reg] != 0) return;
  T* const wl = reinterpret_cast<T*>(smem);                                       // w, then a
  double* const dp = reinterpret_cast<double*>(smem + ((D * (int)sizeof(T) + 15) & ~15));  // chunk prefix sums
  double* const dq = dp + kThreads;                                                // chunk suffix sums
  __shared__ double dscr[kWaves];
  __shared__ int iscr[kWaves];
  const T* W = w.W + reg * w.strideW;
  const T* u = w.u + reg * w.stridev;
  const T* Xg = a.X + reg * a.strideX;
  const T* mg = a.mw + reg * a.stridemw;
  const T si = a.noise_kind == NOISE_DIAGONAL ? a.s[reg * a.strides + i] : a.s[reg * a.strides];
  const T rs = fast_rsqrt(si);
  double mu = 0.0;
  for (int c = tid; c < D; c += kThreads) {
    const T x = (a.layout == LAYOUT_COLVECS) ? Xg[(int64_t)i * a.ldx + c] : Xg[(int64_t)c * a.ldx + i];
    mu += (double)x * (double)mg[c];
    wl[c] = x * rs;
  }
  mu = block_allreduce(mu, dscr, tid);  // (its barriers also publish wl)
  const double e = ((double)a.y[reg * a.stridey + i] - mu) * (double)rs;
  for (int j0 = 0; j0 < D; j0 += 64) {
    const int nb = D - j0 < 64 ? D - j0 : 64;
    if (wave == 0) {
      T v = lane < nb ? wl[j0 + lane] : T(0);
      const T rd = lane < nb ? fast_rcp(W[(int64_t)(j0 + lane) * D + j0 + lane]) : T(0);
      for (int jj = 0; jj < nb; ++jj) {
        const T aj = readlane(v, jj) * readlane(rd, jj);
        if (lane == jj) v = aj;
        if (lane > jj && lane < nb) v = fused_madd(-W[(int64_t)(j0 + jj) * D + j0 + lane], aj, v);
      }
      if (lane < nb) wl[j0 + lane] = v;
    }
    __syncthreads();
    for (int c = j0 + nb + tid; c < D; c += kThreads) {
      T acc = wl[c];
      for (int jj = 0; jj < nb; ++jj) acc = fused_madd(-W[(int64_t)(j0 + jj) * D + c], wl[j0 + jj], acc);
      wl[c] = acc;
    }
    __syncthreads();
  }
  // scans over contiguous chunks of a (thread t: [t C, (t + 1) C)), fixed order
  __shared__ double total;
  const int C = (D + kThreads - 1) / kThreads, jb = tid * C < D ? tid * C : D, je = jb + C < D ? jb + C : D;
  double loc = 0.0, atu = 0.0;
  for (int j = jb; j < je; ++j) { const double aj = (double)wl[j]; loc += aj * aj; atu += aj * (double)u[j]; }
  dq[tid] = loc;
  atu = block_allreduce(atu, dscr, tid);  // (its barriers publish dq)
  if (tid == 0) {
    double run = 0.0;
    for (int t = 0; t < kThreads; ++t) { dp[t] = run; run += dq[t]; }   // dp[t]: sum over the chunks before t
    total = run;
    run = 0.0;
    for (int t = kThreads - 1; t >= 0; --t) { const double v = dq[t]; dq[t] = run; run += v; }  // dq[t]: after t
  }
  __syncthreads();
  const double alpha2 = 1.0 - total;
  if (!(alpha2 > 0.0)) {
    int cand = 0x7fffffff;
    double P = dp[tid];
    for (int j = jb; j < je; ++j) {
      const double aj = (double)wl[j];
      P += aj * aj;
      if (!(P < 1.0)) { cand = j + 1; break; }
    }
    cand = block_min_int(cand, iscr, tid);
    if (tid == 0) w.st[reg] = cand != 0x7fffffff ? cand : D;
    return;
  }
  T* cs = w.cs + reg * w.stridev;
  T* sn = w.sn + reg * w.stridev;
  double sfx = dq[tid];
  for (int j = je - 1; j >= jb; --j) {
    const double aj = (double)wl[j], after = sfx;
    sfx += aj * aj;
    const double al = sqrt(alpha2 + sfx);
    cs[j] = (T)(sqrt(alpha2 + after) / al);
    sn[j] = (T)(aj / al);
  }
  if (tid == 0) {
    const double zeta = (e - atu) / sqrt(alpha2);
    w.sc[reg * 4 + 2] += zeta * zeta;
    w.sc[reg * 4 + 3] = zeta;
  }
}

// observation i: the rotations, one column per thread, ceil((D + 1) / 256) workgroups per regressor (column D = u).  The row
// loop is uniform over a wave (its lanes meet the same row together: coalesced), a lane joins at its own diagonal.
template <typename T>
__global__ __launch_bounds__(kThreads) void downdate_g_apply_kernel(SweepArgs<T> a, DowndateWs<T> w) {
  const int D = a.D;
  const int64_t reg = blockIdx.x;
  if (w.st[reg] != 0) return;
  const int c = blockIdx.y * kThreads + threadIdx.x;
  const int cw = (int)blockIdx.y * kThreads + (int)(threadIdx.x | 63);  // the wave's last column
  T* W = w.W + reg * w.strideW;
  T* u = w.u + reg * w.stridev;
  const T* cs = w.cs + reg * w.stridev;
  const T* sn = w.sn + reg * w.stridev;
  T xx = c == D ? (T)w.sc[reg * 4 + 3] : T(0);
  for (int j = cw < D ? cw : D - 1; j >= 0; --j) {
    if (j <= c && c <= D) {
      T* p = c == D ? u + j : W + (int64_t)j * D + c;
      const T r = *p, cj = cs[j], sj = sn[j];
      *p = cj * r - sj * xx;
      xx = cj * xx + sj * r;
    }
  }
}

template <typename T>
__host__ __device__ constexpr int downdate_g_finish_lds(int D) { return ((D * (int)sizeof(T) + 15) & ~15) + 64; }

// d = T'^-1 u' (blocked, from the bottom), m' = m + d, the log density, the status
template <typename T>
__global__ __launch_bounds__(kThreads) void downdate_g_finish_kernel(SweepArgs<T> a, DowndateWs<T> w) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double dscr[kWaves];
  const int D = a.D, tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int64_t reg = blockIdx.x;
  T* const dv = reinterpret_cast<T*>(smem);
  const int st = w.st[reg];
  double logpdf = 0.0;
  if (st == 0) {
    const T* W = w.W + reg * w.strideW;
    const T* u = w.u + reg * w.stridev;
    for (int c = tid; c < D; c += kThreads) dv[c] = u[c];
    __syncthreads();
    for (int j1 = D; j1 > 0; j1 -= 64) {
      const int j0 = j1 > 64 ? j1 - 64 : 0, nb = j1 - j0;
      if (wave == 0) {
        T v = lane < nb ? dv[j0 + lane] : T(0);
        const T rd = lane < nb ? fast_rcp(W[(int64_t)(j0 + lane) * D + j0 + lane]) : T(0);
        for (int jj = nb - 1; jj >= 0; --jj) {
          const T dj = readlane(v, jj) * readlane(rd, jj);
          if (lane == jj) v = dj;
          if (lane < jj) v = fused_madd(-W[(int64_t)(j0 + lane) * D + j0 + jj], dj, v);
        }
        if (lane < nb) dv[j0 + lane] = v;
      }
      __syncthreads();
      for (int r = tid; r < j0; r += kThreads) {
        T acc = dv[r];
        for (int jj = 0; jj < nb; ++jj) acc = fused_madd(-W[(int64_t)r * D + j0 + jj], dv[j0 + jj], acc);
        dv[r] = acc;
      }
      __syncthreads();
    }
    double ld1 = 0.0;
    for (int j = tid; j < D; j += kThreads) ld1 += log((double)W[(int64_t)j * D + j]);
    ld1 = block_allreduce(ld1, dscr, tid);
    T* mg = a.mw + reg * a.stridemw;
    for (int c = tid; c < D; c += kThreads) mg[c] = mg[c] + dv[c];
    const double kLog2Pi = 1.8378770664093454835606594728112;
    const double* sc = w.sc + reg * 4;
    logpdf = -0.5 * ((double)a.k * kLog2Pi + sc[0] + 2.0 * (sc[1] - ld1) + sc[2]);
  }
  if (tid == 0) {
    a.info[reg] = st;
    if (a.logpdf) a.logpdf[reg] = st ? __longlong_as_double(0x7ff8000000000000LL) : logpdf;
  }
}

}  // namespace blr
