// Columns 1 .. S-1 of a batched multi-output posterior (blr_posterior_multi_batched_*).
//
// Replaces reference src/bayesian_linear_regression.jl:55-58 (logpdf), :60-69 (posterior) and :72-89 (shared quantities) under a
// map over fxs whose targets are MATRICES: S columns per regressor share the design matrix, the noise and the prior, so the Gram
// matrix and its factor T (chol(Lw + X S^-1 X').U, :86) are formed once -- by the ordinary update of column 0, on whatever route
// blr_posterior_batched_* gives the shape.  What remains per further column s is
//   b_s = X S^-1 (y_s - X'mw)        q_s = (y_s - X'mw)' S^-1 (y_s - X'mw)        u_s = T^-T b_s        mw_s = mw + T^-1 u_s      (:64, :68)
//   logpdf_s = logpdf_0 + (q_0 - |u_0|^2) / 2 - (q_s - |u_s|^2) / 2                                                             (:84 + :57)
// (the log-determinants and N log 2 pi are those of column 0: K8's identity).
//
// multi_cols_kernel: grid (regressors, column passes), 256 threads.  A pass takes kMultiColsPerPass column SLOTS: slot 0 is always
// column 0 (its q_0 and u_0 enter every other column's evidence; its outputs stay those of the update that made the factor), slots
// 1 .. 63 are the pass's own columns.  Per workgroup:
//   stream   X in chunks of kMultiKC observations through LDS (one read of X per pass): mu_n = x_n'mw, the weighted residuals
//            (y_ns - mu_n) / s_n of every slot, B += X_chunk R_chunk on the fp64 / fp32 matrix cores (16x16x4, k in ascending order),
//            q_s in double.  The next chunk's loads are in flight while this one is multiplied.
//   solve    the finished factor as a packed triangle in LDS (over the stream's buffers), one wave per right-hand side: forward
//            substitution, |u_s|^2 in double, back substitution, mean and evidence out.
// A regressor whose status is not 0 gets NaN evidences and nothing else.  Every sum has a fixed order and every column is computed from
// its own data only: the bits of a column do not depend on B, on S, on its slot or on the other columns.
#pragma once
#include "blr_common.hpp"

namespace blr {

constexpr int kMultiColsPerPass = 64;  // column slots of a pass (slot 0 = column 0): four 16-column MFMA tiles
constexpr int kMultiKC = 32;           // observations per staged chunk (eight k-steps)
constexpr int kMultiHeader = 2048;     // LDS bytes in front of the stream / solve buffers: q[64], |u|^2[64] (double), mw[128]

template <typename T>
struct MultiColsArgs {
  const T* X; int64_t ldx, strideX;
  const T* Y; int64_t ldY, strideY;
  const T* s; int64_t strides;
  const T* mw; int64_t stridemw;
  const T* Tf; int64_t ldt, strideT;  // the factor of every regressor (upper triangle read), as column 0's update wrote it
  const double* lp0;                  // [B] evidence of column 0
  const int32_t* info;                // [B] status of the shared factorisation
  T* mw_post; int64_t ldmp, stride_mwpost;
  double* logpdf; int64_t stride_lp;
  int noise_kind, D, N, S;
};

// dynamic LDS of a launch whose passes hold up to `nslots` columns (slot 0 included)
inline size_t multi_cols_lds_bytes(size_t elem, int D, int nslots) {
  const size_t DP = (size_t)((D + 15) / 16 * 16);
  const size_t stream = (size_t)8 * kMultiKC * sizeof(double) + (size_t)kMultiKC * (DP + 1) * elem + (size_t)kMultiKC * (kMultiColsPerPass + 1) * elem;
  const size_t solve = (((size_t)D * (D + 1) / 2 * elem + 7) & ~(size_t)7) + (size_t)nslots * DP * elem;
  return kMultiHeader + (stream > solve ? stream : solve);
}

// L u = b with L = T' (row i of L at P + pidx(i, 0)); lanes own rows lane and lane + 64; r = 1 / L_ii of the owned rows
template <typename T>
__device__ __forceinline__ void multi_forward(const T* P, int D, int lane, T r0, T r1, T& b0, T& b1) {
  const int i0 = lane, i1 = lane + 64;
  for (int kb = 0; kb < D; kb += 8) {
    T c0[8], c1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb + u;
      c0[u] = (k < D && i0 > k && i0 < D) ? P[pidx(i0, k)] : T(0);
      c1[u] = (k < D && i1 > k && i1 < D) ? P[pidx(i1, k)] : T(0);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb + u;
      if (k < D) {
        const bool lo = k < 64;
        const T uk = readlane(lo ? b0 : b1, k & 63) * readlane(lo ? r0 : r1, k & 63);
        if (lane == (k & 63)) { if (lo) b0 = uk; else b1 = uk; }
        b0 -= c0[u] * uk;
        b1 -= c1[u] * uk;
      }
    }
  }
}

// T m = u (column-oriented, as phase_backsolve of the fused kernel)
template <typename T>
__device__ __forceinline__ void multi_backward(const T* P, int D, int lane, T r0, T r1, T& b0, T& b1) {
  const int i0 = lane, i1 = lane + 64;
  for (int kb = D - 1; kb >= 0; kb -= 8) {
    T c0[8], c1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb - u;
      const T* row = P + pidx(k >= 0 ? k : 0, 0);
      c0[u] = (k >= 0 && i0 < k) ? row[i0] : T(0);
      c1[u] = (k >= 0 && i1 < k) ? row[i1] : T(0);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = kb - u;
      if (k >= 0) {
        const bool lo = k < 64;
        const T mk = readlane(lo ? b0 : b1, k & 63) * readlane(lo ? r0 : r1, k & 63);
        if (lane == (k & 63)) { if (lo) b0 = mk; else b1 = mk; }
        b0 -= c0[u] * mk;
        b1 -= c1[u] * mk;
      }
    }
  }
}

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void multi_cols_kernel(MultiColsArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using M = Mfma<T>;
  constexpr int KC = kMultiKC, NEW = kMultiColsPerPass - 1, LDR = kMultiColsPerPass + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t reg = blockIdx.x;
  const int pass = blockIdx.y;
  const int D = a.D, N = a.N;
  const int NB = (D + 15) / 16, DP = 16 * NB, LDX = DP + 1;
  const int col_first = 1 + pass * NEW;                            // column of slot 1
  const int ncols = min(NEW, a.S - col_first);                     // this pass's own columns (0 only when S == 1)
  const int nslots = ncols + 1, NT = (nslots + 15) / 16;
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  double* const lp_out = a.logpdf ? a.logpdf + reg * a.stride_lp : nullptr;

  if (a.info[reg] != 0) {  // (block-uniform) the shared factorisation failed: NaN evidences, nothing else
    if (lp_out && tid < nslots && (tid > 0 || pass == 0)) lp_out[tid == 0 ? 0 : col_first + tid - 1] = kNaN;
    return;
  }
  if (ncols <= 0) {  // S == 1: the call is column 0's update
    if (lp_out && tid == 0 && pass == 0) lp_out[0] = a.lp0[reg];
    return;
  }

  double* const qS = reinterpret_cast<double*>(smem);
  double* const uuS = qS + kMultiColsPerPass;
  T* const mwS = reinterpret_cast<T*>(smem + 2 * kMultiColsPerPass * sizeof(double));
  // stream buffers
  double* const mup = reinterpret_cast<double*>(smem + kMultiHeader);                  // [8][KC] partial x_n'mw
  T* const Xs = reinterpret_cast<T*>(smem + kMultiHeader + 8 * KC * sizeof(double));  // [KC][LDX]
  T* const Rs = Xs + KC * LDX;                                                        // [KC][LDR]
  // solve buffers (over the stream's)
  T* const P = reinterpret_cast<T*>(smem + kMultiHeader);                              // packed factor: row i of L = T' at pidx(i, 0)
  T* const Bs = reinterpret_cast<T*>(smem + kMultiHeader + (((size_t)D * (D + 1) / 2 * sizeof(T) + 7) & ~(size_t)7));  // [nslots][DP]

  const BLR_GLOBAL T* const Xg = as_global(a.X + reg * a.strideX);
  const BLR_GLOBAL T* const Yg = as_global(a.Y + reg * a.strideY);
  const BLR_GLOBAL T* const sg = as_global(a.s + reg * a.strides);
  const BLR_GLOBAL T* const mwg = as_global(a.mw + reg * a.stridemw);
  if (tid < 128) mwS[tid] = tid < D ? mwg[tid] : T(0);

  // thread roles of the column work: observation n_t of the chunk, segment seg (features seg * 2 NB .. and slots seg, seg + 8, ..)
  const int n_t = tid & (KC - 1), seg = tid >> 5;
  const int xcnt = 2 * NB;  // staged elements of X per thread and chunk (DP * KC / 256)
  T xreg[16], yreg[8], ycur[8];
  T sreg = T(1), scur = T(1);
  if (a.noise_kind == NOISE_ISOTROPIC) sreg = scur = sg[0];

  auto prefetch = [&](int n0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i < xcnt) {
        const int e = tid + kThreads * i;
        int d, n;
        if (LAYOUT == LAYOUT_COLVECS) { d = e % DP; n = e / DP; } else { n = e % KC; d = e / KC; }
        const bool ok = d < D && n0 + n < N;
        const int64_t at = LAYOUT == LAYOUT_COLVECS ? (int64_t)d + (int64_t)(n0 + n) * a.ldx : (int64_t)(n0 + n) + (int64_t)d * a.ldx;
        xreg[i] = ok ? Xg[at] : T(0);
      }
    }
    const bool nok = n0 + n_t < N;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = seg + 8 * i;
      const int col = j == 0 ? 0 : col_first + j - 1;
      yreg[i] = (nok && j < nslots) ? Yg[(int64_t)col * a.ldY + n0 + n_t] : T(0);
    }
    if (a.noise_kind == NOISE_DIAGONAL) sreg = nok ? sg[n0 + n_t] : T(1);
  };

  typename M::acc4 acc[2][4];
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[ib][jt] = typename M::acc4{0, 0, 0, 0};
  double q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = 0.0;

  if (N > 0) prefetch(0);
  for (int n0 = 0; n0 < N; n0 += KC) {
    // staged registers -> LDS
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i < xcnt) {
        const int e = tid + kThreads * i;
        int d, n;
        if (LAYOUT == LAYOUT_COLVECS) { d = e % DP; n = e / DP; } else { n = e % KC; d = e / KC; }
        Xs[n * LDX + d] = xreg[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) ycur[i] = yreg[i];
    scur = sreg;
    __syncthreads();
    if (n0 + KC < N) prefetch(n0 + KC);
    // mu_n = x_n'mw: eight partial sums per observation, added 0 .. 7
    {
      double part = 0.0;
      const T* xr = Xs + n_t * LDX + seg * xcnt;
      const T* mr = mwS + seg * xcnt;
      for (int d = 0; d < xcnt; ++d) part = __builtin_fma((double)xr[d], (double)mr[d], part);
      mup[seg * KC + n_t] = part;
    }
    __syncthreads();
    {
      double mu = mup[n_t];
#pragma unroll
      for (int g = 1; g < 8; ++g) mu += mup[g * KC + n_t];
      const bool nok = n0 + n_t < N;
      const double w = 1.0 / (double)scur;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = seg + 8 * i;
        double r = 0.0;
        if (nok && j < nslots) {
          const double delta = (double)ycur[i] - mu;
          r = delta * w;
          q[i] = __builtin_fma(delta, r, q[i]);
        }
        Rs[n_t * LDR + j] = (T)r;
      }
    }
    __syncthreads();
    // B += X_chunk R_chunk: wave w owns row blocks w and w + 4, every column tile in use
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      const int krow = 4 * ks + (lane >> 4);
      T bf[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) bf[jt] = jt < NT ? Rs[krow * LDR + 16 * jt + (lane & 15)] : T(0);
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        const int I = wave + 4 * ib;
        if (I < NB) {
          const T af = Xs[krow * LDX + 16 * I + (lane & 15)];
#pragma unroll
          for (int jt = 0; jt < 4; ++jt)
            if (jt < NT) acc[ib][jt] = M::mma(af, bf[jt], acc[ib][jt]);
        }
      }
    }
    __syncthreads();
  }

  // q_s: sum over the 32 observation lanes of a segment (fixed butterfly)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    double v = q[i];
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (n_t == 0) qS[seg + 8 * i] = v;
  }
  // B -> LDS, column by column; the factor -> packed triangle
#pragma unroll
  for (int ib = 0; ib < 2; ++ib) {
    const int I = wave + 4 * ib;
    if (I < NB) {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = 16 * jt + (lane & 15);
        if (jt < NT && j < nslots) {
#pragma unroll
          for (int v = 0; v < 4; ++v) Bs[j * DP + 16 * I + M::crow(lane, v)] = acc[ib][jt][v];
        }
      }
    }
  }
  {
    const BLR_GLOBAL T* const Tg = as_global(a.Tf + reg * a.strideT);
    for (int c = wave; c < D; c += kWaves)
      for (int r = lane; r <= c; r += kWave) P[pidx(c, r)] = Tg[(int64_t)c * a.ldt + r];
  }
  __syncthreads();

  {
    const int i0 = lane, i1 = lane + 64;
    const T r0 = i0 < D ? T(1) / P[pidx(i0, i0)] : T(0);
    const T r1 = i1 < D ? T(1) / P[pidx(i1, i1)] : T(0);
    for (int j = wave; j < nslots; j += kWaves) {
      T b0 = i0 < D ? Bs[j * DP + i0] : T(0);
      T b1 = i1 < D ? Bs[j * DP + i1] : T(0);
      multi_forward<T>(P, D, lane, r0, r1, b0, b1);
      const double uu = wave_allreduce((double)b0 * (double)b0 + (double)b1 * (double)b1);
      if (lane == 0) uuS[j] = uu;
      if (j > 0 && a.mw_post) {
        multi_backward<T>(P, D, lane, r0, r1, b0, b1);
        BLR_GLOBAL T* const out = as_global(a.mw_post + reg * a.stride_mwpost + (int64_t)(col_first + j - 1) * a.ldmp);
        if (i0 < D) out[i0] = mwS[i0] + b0;  // :68
        if (i1 < D) out[i1] = mwS[i1] + b1;
      }
    }
  }
  __syncthreads();
  if (lp_out && tid < nslots) {
    const double lp0 = a.lp0[reg];
    if (tid == 0) {
      if (pass == 0) lp_out[0] = lp0;
    } else {
      lp_out[col_first + tid - 1] = lp0 + 0.5 * ((qS[0] - uuS[0]) - (qS[tid] - uuS[tid]));
    }
  }
}

// the instantiations the library uses, defined in blr_multi.hip
extern template __global__ void multi_cols_kernel<double, LAYOUT_COLVECS>(MultiColsArgs<double>);
extern template __global__ void multi_cols_kernel<double, LAYOUT_ROWVECS>(MultiColsArgs<double>);
extern template __global__ void multi_cols_kernel<float, LAYOUT_COLVECS>(MultiColsArgs<float>);
extern template __global__ void multi_cols_kernel<float, LAYOUT_ROWVECS>(MultiColsArgs<float>);

}  // namespace blr
