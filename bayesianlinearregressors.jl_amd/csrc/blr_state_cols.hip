// state_cols_kernel, state_cols_global_kernel and state_diag_kernel (blr_state_cols.hpp) instantiated in a translation unit of their
// own, so the code objects of the existing kernels stay as they are: both element types, update and downdate.  Host side:
// blr_abi.hip (state_multi_factor).
#include <hip/hip_runtime.h>

#include "blr_state_cols.hpp"

namespace blr {
namespace {

template <typename T>
const void* ptr_of(bool down, bool global) {
  if (global) return down ? reinterpret_cast<const void*>(state_cols_global_kernel<T, true>) : reinterpret_cast<const void*>(state_cols_global_kernel<T, false>);
  return down ? reinterpret_cast<const void*>(state_cols_kernel<T, true>) : reinterpret_cast<const void*>(state_cols_kernel<T, false>);
}
template <typename T>
void launch_of(bool down, bool global, dim3 grid, size_t lds, hipStream_t stream, const StateColsArgs<T>& a) {
  if (global) {
    if (down) hipLaunchKernelGGL((state_cols_global_kernel<T, true>), grid, dim3(kThreads), lds, stream, a);
    else hipLaunchKernelGGL((state_cols_global_kernel<T, false>), grid, dim3(kThreads), lds, stream, a);
  } else {
    if (down) hipLaunchKernelGGL((state_cols_kernel<T, true>), grid, dim3(kThreads), lds, stream, a);
    else hipLaunchKernelGGL((state_cols_kernel<T, false>), grid, dim3(kThreads), lds, stream, a);
  }
}
template <typename T>
void diag_of(hipStream_t stream, const T* Tf, int64_t ldt, int64_t strideT, int D, int64_t B, T* diag0) {
  const int64_t total = B * D;
  hipLaunchKernelGGL(state_diag_kernel<T>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, Tf, ldt, strideT, D,
                     total, diag0);
}

}  // namespace

const void* state_cols_kernel_ptr_f64(bool down, bool global) { return ptr_of<double>(down, global); }
const void* state_cols_kernel_ptr_f32(bool down, bool global) { return ptr_of<float>(down, global); }
void state_cols_kernel_launch_f64(bool down, bool global, dim3 grid, size_t lds, hipStream_t stream, const StateColsArgs<double>& a) {
  launch_of<double>(down, global, grid, lds, stream, a);
}
void state_cols_kernel_launch_f32(bool down, bool global, dim3 grid, size_t lds, hipStream_t stream, const StateColsArgs<float>& a) {
  launch_of<float>(down, global, grid, lds, stream, a);
}
void state_diag_kernel_launch_f64(hipStream_t stream, const double* Tf, int64_t ldt, int64_t strideT, int D, int64_t B, double* diag0) {
  diag_of<double>(stream, Tf, ldt, strideT, D, B, diag0);
}
void state_diag_kernel_launch_f32(hipStream_t stream, const float* Tf, int64_t ldt, int64_t strideT, int D, int64_t B, float* diag0) {
  diag_of<float>(stream, Tf, ldt, strideT, D, B, diag0);
}

void state_save_kernel_launch_f32(hipStream_t stream, const float* Tf, int64_t ldt, int64_t strideT, int D, int64_t B, float* T0w) {
  const int64_t total = B * D * D;
  hipLaunchKernelGGL(state_save_kernel<float>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, Tf, ldt, strideT, D,
                     total, T0w);
}

}  // namespace blr
