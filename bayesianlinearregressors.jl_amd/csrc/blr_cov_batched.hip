// The instantiations of cov_whiten_kernel and cov_tiles_kernel (blr_cov_batched.hpp): both element types, ColVecs and RowVecs.  Host
// side: blr_abi.hip (mean_and_cov_batched).
#include "blr_cov_batched.hpp"

namespace blr {

template __global__ void cov_whiten_kernel<double, LAYOUT_COLVECS>(CovArgs<double>);
template __global__ void cov_whiten_kernel<double, LAYOUT_ROWVECS>(CovArgs<double>);
template __global__ void cov_whiten_kernel<float, LAYOUT_COLVECS>(CovArgs<float>);
template __global__ void cov_whiten_kernel<float, LAYOUT_ROWVECS>(CovArgs<float>);
template __global__ void cov_tiles_kernel<double>(CovArgs<double>);
template __global__ void cov_tiles_kernel<float>(CovArgs<float>);

}  // namespace blr
