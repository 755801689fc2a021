// The instantiations of kfold_kernel (blr_kfold.hpp): both element types.  Host side: blr_abi.hip (kfold_batched).
#include "blr_kfold.hpp"

namespace blr {

template __global__ void kfold_kernel<double>(KfoldArgs<double>);
template __global__ void kfold_kernel<float>(KfoldArgs<float>);

}  // namespace blr
