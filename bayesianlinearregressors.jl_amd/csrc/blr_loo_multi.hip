// loo_cols_kernel, loo_cols_finish_kernel and loo_cols_total_kernel (blr_loo_multi.hpp) instantiated in a translation unit of their own, so
// the code objects of the existing kernels stay as they are: both element types, ColVecs and RowVecs.  Host side: blr_abi.hip
// (loo_multi_batched).
#include <hip/hip_runtime.h>

#define BLR_NO_PLAIN_KERNELS  // loo_total_kernel and logpdf_sum_kernel live in blr_abi.hip
#include "blr_loo_multi.hpp"

namespace blr {

// ---- loo_total[reg][c] = sum_n logpdf[n, c] in a fixed order: one workgroup per (column, regressor) -------------------------------
__global__ __launch_bounds__(kThreads) void loo_cols_total_kernel(const double* __restrict__ ll, int64_t ld_ll, int64_t stride_ll, int N,
                                                                         double* __restrict__ total, int64_t stride_lt,
                                                                         const int32_t* __restrict__ info, int reg0) {
  const int64_t reg = (int64_t)reg0 + blockIdx.y;
  if (info[reg] != 0) return;
  const double t = fixed_order_sum(ll + reg * stride_ll + (int64_t)blockIdx.x * ld_ll, N);
  if (threadIdx.x == 0) total[reg * stride_lt + blockIdx.x] = t;
}

namespace {

template <typename T>
const void* ptr_of(int layout) {
  return layout == LAYOUT_ROWVECS ? reinterpret_cast<const void*>(loo_cols_kernel<T, LAYOUT_ROWVECS>)
                                  : reinterpret_cast<const void*>(loo_cols_kernel<T, LAYOUT_COLVECS>);
}
template <typename T>
void launch_of(int layout, dim3 grid, size_t lds, hipStream_t stream, const LooColsArgs<T>& a) {
  if (layout == LAYOUT_ROWVECS) hipLaunchKernelGGL((loo_cols_kernel<T, LAYOUT_ROWVECS>), grid, dim3(kThreads), lds, stream, a);
  else hipLaunchKernelGGL((loo_cols_kernel<T, LAYOUT_COLVECS>), grid, dim3(kThreads), lds, stream, a);
}

}  // namespace

const void* loo_cols_kernel_ptr_f64(int layout) { return ptr_of<double>(layout); }
const void* loo_cols_kernel_ptr_f32(int layout) { return ptr_of<float>(layout); }
void loo_cols_kernel_launch_f64(int layout, dim3 grid, size_t lds, hipStream_t stream, const LooColsArgs<double>& a) {
  launch_of<double>(layout, grid, lds, stream, a);
}
void loo_cols_kernel_launch_f32(int layout, dim3 grid, size_t lds, hipStream_t stream, const LooColsArgs<float>& a) {
  launch_of<float>(layout, grid, lds, stream, a);
}
void loo_cols_finish_launch_f64(dim3 grid, hipStream_t stream, const LooColsArgs<double>& a, const double* mean, int64_t ldmn, int64_t stridemn,
                                const double* var, int64_t ldw) {
  hipLaunchKernelGGL(loo_cols_finish_kernel<double>, grid, dim3(kThreads), 0, stream, a, mean, ldmn, stridemn, var, ldw);
}
void loo_cols_finish_launch_f32(dim3 grid, hipStream_t stream, const LooColsArgs<float>& a, const float* mean, int64_t ldmn, int64_t stridemn,
                                const float* var, int64_t ldw) {
  hipLaunchKernelGGL(loo_cols_finish_kernel<float>, grid, dim3(kThreads), 0, stream, a, mean, ldmn, stridemn, var, ldw);
}
void loo_cols_total_launch(dim3 grid, hipStream_t stream, const double* ll, int64_t ld_ll, int64_t stride_ll, int N, double* total,
                           int64_t stride_lt, const int32_t* info, int reg0) {
  hipLaunchKernelGGL(loo_cols_total_kernel, grid, dim3(kThreads), 0, stream, ll, ld_ll, stride_ll, N, total, stride_lt, info, reg0);
}

}  // namespace blr
