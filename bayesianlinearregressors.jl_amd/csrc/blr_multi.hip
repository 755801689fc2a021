// The instantiations of multi_cols_kernel (blr_multi.hpp): both element types, ColVecs and RowVecs.  Host side: blr_abi.hip
// (posterior_multi_batched).
#include "blr_multi.hpp"

namespace blr {

template __global__ void multi_cols_kernel<double, LAYOUT_COLVECS>(MultiColsArgs<double>);
template __global__ void multi_cols_kernel<double, LAYOUT_ROWVECS>(MultiColsArgs<double>);
template __global__ void multi_cols_kernel<float, LAYOUT_COLVECS>(MultiColsArgs<float>);
template __global__ void multi_cols_kernel<float, LAYOUT_ROWVECS>(MultiColsArgs<float>);

}  // namespace blr
