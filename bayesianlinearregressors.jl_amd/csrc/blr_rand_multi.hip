// The instantiations of rand_cols_solve_kernel and rand_cols_project_kernel (blr_rand_multi.hpp): both element types, ColVecs and
// RowVecs.  Host side: blr_abi.hip (rand_multi_batched).
#include "blr_rand_multi.hpp"

namespace blr {

template __global__ void rand_cols_solve_kernel<double>(RandColsArgs<double>);
template __global__ void rand_cols_solve_kernel<float>(RandColsArgs<float>);
template __global__ void rand_cols_project_kernel<double, LAYOUT_COLVECS>(RandColsArgs<double>);
template __global__ void rand_cols_project_kernel<double, LAYOUT_ROWVECS>(RandColsArgs<double>);
template __global__ void rand_cols_project_kernel<float, LAYOUT_COLVECS>(RandColsArgs<float>);
template __global__ void rand_cols_project_kernel<float, LAYOUT_ROWVECS>(RandColsArgs<float>);

}  // namespace blr
