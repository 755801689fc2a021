// The instantiations of state_cols_kernel, state_cols_global_kernel, state_diag_kernel and state_save_kernel (blr_state_cols.hpp): both
// element types, update and downdate (state_save_kernel: fp32 only, the one that reads the saved factor).  Host side: blr_abi.hip
// (state_multi_factor).
#include "blr_state_cols.hpp"

namespace blr {

template __global__ void state_cols_kernel<double, false>(StateColsArgs<double>);
template __global__ void state_cols_kernel<double, true>(StateColsArgs<double>);
template __global__ void state_cols_kernel<float, false>(StateColsArgs<float>);
template __global__ void state_cols_kernel<float, true>(StateColsArgs<float>);
template __global__ void state_cols_global_kernel<double, false>(StateColsArgs<double>);
template __global__ void state_cols_global_kernel<double, true>(StateColsArgs<double>);
template __global__ void state_cols_global_kernel<float, false>(StateColsArgs<float>);
template __global__ void state_cols_global_kernel<float, true>(StateColsArgs<float>);
template __global__ void state_diag_kernel<double>(const double*, int64_t, int64_t, int, int64_t, double*);
template __global__ void state_diag_kernel<float>(const float*, int64_t, int64_t, int, int64_t, float*);
template __global__ void state_save_kernel<float>(const float*, int64_t, int64_t, int, int64_t, float*);

}  // namespace blr
