// Exact leave-one-out (LOO) predictives of the observations a posterior state contains (blr_loo_batched_*).
// With A = T'T the precision given all the data, mw' its mean and s_n the noise variance of observation n:
//   sigma2_n = x_n'A^-1 x_n = |T^-T x_n|^2     (the marginal stream's var without its noise term)
//   m_n      = x_n'mw'                          (the marginal stream's mean)
//   r_n = y_n - m_n,   1 - h_n = (s_n - sigma2_n) / s_n
//   var_n = s_n / (1 - h_n),   mean_n = y_n - r_n / (1 - h_n),
//   logpdf_n = -1/2 [log 2 pi + log s_n - log(1 - h_n) + r_n^2 / (s_n (1 - h_n))]
// (Woodbury on K = X'Lw^-1 X + S: [K^-1]_nn = (s_n - sigma2_n) / s_n^2, [K^-1 delta]_n = r_n / s_n; Rasmussen & Williams eq.
// 5.12 -- the prior mean cancels.)  The same numbers as blr_downdate_factor_* at k = 1 for every n, from one marginal pass.
// Two routes share loo_predictive, the one place the formula lives:
//   D = 128, aligned ColVecs / RowVecs, N >= 64: marginals_gemm_kernel<T, ROWV, LooGemmArgs<T>> (blr_marginals.hpp) -- the marginal product stream with y_n in
//     the tile loads and the epilogue at the store; nothing N-long but the outputs goes to memory;
//   everything else: the marginal routes with zero noise into handle workspace, then loo_finish_kernel.
// Totals: loo_total_kernel, the fixed-order block sum of logpdf_sum_kernel once per regressor.
#pragma once
#include "blr_common.hpp"
#include "blr_aux_kernels.hpp"

namespace blr {

template <typename T>
struct LooArgs {
  const T* y; int64_t stridey;
  const T* s; int64_t strides; int noise_kind;
  T* lm; int64_t stride_lm;        // LOO predictive means (may be NULL)
  T* lv; int64_t stride_lv;        // LOO predictive variances, noise included (may be NULL)
  double* ll; int64_t stride_ll;   // LOO log densities (may be NULL when no total is asked for)
  unsigned long long* degenerate;  // counter of observations with 1 - h_n <= 0 or not finite (blr_get_stat "loo_degenerate")
  const int32_t* info;             // per-regressor status of loo_check_kernel: a regressor with info != 0 is skipped
  int N;
};

struct LooOut { double mean, var, logpdf; };

// the epilogue, in double whatever the element type (fp32 would lose the difference s_n - sigma2_n twice otherwise).  Returns
// false for a degenerate leverage: the three outputs are then NaN.
__device__ __forceinline__ bool loo_predictive(double y, double m, double sig2, double s, LooOut& o) {
  const double kLog2Pi = 1.8378770664093454835606594728112;
  const double omh = (s - sig2) / s;  // 1 - h_n
  if (!(omh > 0.0) || !isfinite(omh)) {
    const double nan = __builtin_nan("");
    o.mean = nan; o.var = nan; o.logpdf = nan;
    return false;
  }
  const double r = y - m;
  o.var = s / omh;
  o.mean = y - r / omh;
  o.logpdf = -0.5 * (kLog2Pi + log(s) - log(omh) + r * r / (s * omh));
  return true;
}

// observation n of regressor reg: the epilogue and the stores; returns false for a degenerate leverage
template <typename T>
__device__ __forceinline__ bool loo_store(const LooArgs<T>& l, int64_t reg, int n, double y, double m, double sig2, double s) {
  LooOut o;
  const bool ok = loo_predictive(y, m, sig2, s, o);
  if (l.lm) l.lm[reg * l.stride_lm + n] = (T)o.mean;
  if (l.lv) l.lv[reg * l.stride_lv + n] = (T)o.var;
  if (l.ll) l.ll[reg * l.stride_ll + n] = o.logpdf;
  return ok;
}

// the degenerate observations of a wave, one integer add per wave (all 64 lanes must take part)
__device__ __forceinline__ void loo_count(int c, unsigned long long* ctr) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
  if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(ctr, (unsigned long long)c);
}

// ---- status, in the update's and downdate's order: a non-positive diagonal entry j of T (1-based), else a non-positive s_i ----
template <typename T>
__global__ __launch_bounds__(kThreads) void loo_check_kernel(const T* __restrict__ Tf, int64_t ldt, int64_t strideT, int D,
                                                             const T* __restrict__ s, int64_t strides, int noise_kind, int N,
                                                             int32_t* __restrict__ info) {
  __shared__ int bad[2];
  const int tid = threadIdx.x;
  const int64_t reg = blockIdx.x;
  if (tid == 0) { bad[0] = 0x7fffffff; bad[1] = 0x7fffffff; }
  __syncthreads();
  const T* Tg = Tf + reg * strideT;
  for (int j = tid; j < D; j += kThreads)
    if (!(Tg[(int64_t)j * ldt + j] > T(0))) atomicMin(&bad[0], j + 1);
  const int ns = noise_kind == NOISE_DIAGONAL ? N : (N > 0 ? 1 : 0);
  const T* sg = s + reg * strides;
  for (int i = tid; i < ns; i += kThreads)
    if (!(sg[i] > T(0))) atomicMin(&bad[1], i + 1);
  __syncthreads();
  if (tid == 0) info[reg] = bad[0] != 0x7fffffff ? bad[0] : (bad[1] != 0x7fffffff ? bad[1] : 0);
}

// ---- composed route: the epilogue over the marginal routes' mean and latent variance (chunk-local, ldw apart) ----------------
template <typename T>
__global__ __launch_bounds__(kThreads) void loo_finish_kernel(LooArgs<T> l, const T* __restrict__ mean, const T* __restrict__ var,
                                                              int64_t ldw, int reg0) {
  const int64_t reg = reg0 + (int64_t)blockIdx.y;
  if (l.info[reg] != 0) return;
  const T* y = l.y + reg * l.stridey;
  const T* s = l.s + reg * l.strides;
  const T* m = mean + (int64_t)blockIdx.y * ldw;
  const T* v = var + (int64_t)blockIdx.y * ldw;
  const bool diag = l.noise_kind == NOISE_DIAGONAL;
  int ndeg = 0;
  for (int n = blockIdx.x * kThreads + threadIdx.x; n < l.N; n += gridDim.x * kThreads)
    if (!loo_store(l, reg, n, (double)y[n], (double)m[n], (double)v[n], (double)(diag ? s[n] : s[0]))) ++ndeg;
  loo_count(ndeg, l.degenerate);
}

// ---- loo_total[reg] = sum_n logpdf_n in a fixed order (no float atomics: the same bits at any B and position) -------------------
// (a plain kernel is declared here and defined once, in blr_abi.hip)
__global__ __launch_bounds__(kThreads) void loo_total_kernel(const double* __restrict__ ll, int64_t stride_ll, int N, double* __restrict__ total,
                                 const int32_t* __restrict__ info, int reg0);

}  // namespace blr
