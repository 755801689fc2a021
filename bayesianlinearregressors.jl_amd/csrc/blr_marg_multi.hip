// marginals_cols_kernel (blr_marg_multi.hpp) instantiated in a translation unit of its own, so the code objects of the existing kernels stay
// as they are: both element types, ColVecs and RowVecs.  Host side: blr_abi.hip (marginals_multi_batched).
#include <hip/hip_runtime.h>

#include "blr_marg_multi.hpp"

namespace blr {
namespace {

template <typename T>
const void* ptr_of(int layout) {
  return layout == LAYOUT_ROWVECS ? reinterpret_cast<const void*>(marginals_cols_kernel<T, LAYOUT_ROWVECS>)
                                  : reinterpret_cast<const void*>(marginals_cols_kernel<T, LAYOUT_COLVECS>);
}
template <typename T>
void launch_of(int layout, dim3 grid, size_t lds, hipStream_t stream, const MargColsArgs<T>& a) {
  if (layout == LAYOUT_ROWVECS) hipLaunchKernelGGL((marginals_cols_kernel<T, LAYOUT_ROWVECS>), grid, dim3(kThreads), lds, stream, a);
  else hipLaunchKernelGGL((marginals_cols_kernel<T, LAYOUT_COLVECS>), grid, dim3(kThreads), lds, stream, a);
}

}  // namespace

const void* marginals_cols_kernel_ptr_f64(int layout) { return ptr_of<double>(layout); }
const void* marginals_cols_kernel_ptr_f32(int layout) { return ptr_of<float>(layout); }
void marginals_cols_kernel_launch_f64(int layout, dim3 grid, size_t lds, hipStream_t stream, const MargColsArgs<double>& a) {
  launch_of<double>(layout, grid, lds, stream, a);
}
void marginals_cols_kernel_launch_f32(int layout, dim3 grid, size_t lds, hipStream_t stream, const MargColsArgs<float>& a) {
  launch_of<float>(layout, grid, lds, stream, a);
}

}  // namespace blr
