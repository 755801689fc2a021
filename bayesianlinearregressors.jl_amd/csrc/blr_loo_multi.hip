// The instantiations of loo_cols_kernel and loo_cols_finish_kernel (blr_loo_multi.hpp), both element types, ColVecs and RowVecs, and
// the definition of loo_cols_total_kernel.  Host side: blr_abi.hip (loo_multi_batched).
#include "blr_loo_multi.hpp"

namespace blr {

__global__ __launch_bounds__(kThreads) void loo_cols_total_kernel(const double* __restrict__ ll, int64_t ld_ll, int64_t stride_ll, int N,
                                                                         double* __restrict__ total, int64_t stride_lt,
                                                                         const int32_t* __restrict__ info, int reg0) {
  const int64_t reg = (int64_t)reg0 + blockIdx.y;
  if (info[reg] != 0) return;
  const double t = fixed_order_sum(ll + reg * stride_ll + (int64_t)blockIdx.x * ld_ll, N);
  if (threadIdx.x == 0) total[reg * stride_lt + blockIdx.x] = t;
}

template __global__ void loo_cols_kernel<double, LAYOUT_COLVECS>(LooColsArgs<double>);
template __global__ void loo_cols_kernel<double, LAYOUT_ROWVECS>(LooColsArgs<double>);
template __global__ void loo_cols_kernel<float, LAYOUT_COLVECS>(LooColsArgs<float>);
template __global__ void loo_cols_kernel<float, LAYOUT_ROWVECS>(LooColsArgs<float>);
template __global__ void loo_cols_finish_kernel<double>(LooColsArgs<double>, const double*, int64_t, int64_t, const double*, int64_t);
template __global__ void loo_cols_finish_kernel<float>(LooColsArgs<float>, const float*, int64_t, int64_t, const float*, int64_t);

}  // namespace blr
