// The instantiations of marginals_cols_kernel (blr_marg_multi.hpp): both element types, ColVecs and RowVecs.  Host side: blr_abi.hip
// (marginals_multi_batched).
#include "blr_marg_multi.hpp"

namespace blr {

template __global__ void marginals_cols_kernel<double, LAYOUT_COLVECS>(MargColsArgs<double>);
template __global__ void marginals_cols_kernel<double, LAYOUT_ROWVECS>(MargColsArgs<double>);
template __global__ void marginals_cols_kernel<float, LAYOUT_COLVECS>(MargColsArgs<float>);
template __global__ void marginals_cols_kernel<float, LAYOUT_ROWVECS>(MargColsArgs<float>);

}  // namespace blr
