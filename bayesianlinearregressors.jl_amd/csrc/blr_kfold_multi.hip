// The instantiations of kfold_whiten_cols_kernel and kfold_cols_kernel (blr_kfold_multi.hpp): both element types, the whitening pass
// for ColVecs and RowVecs.  Host side: blr_abi.hip (kfold_multi_batched).
#include "blr_kfold_multi.hpp"

namespace blr {

template __global__ void kfold_whiten_cols_kernel<double, LAYOUT_COLVECS>(KfoldWhitenArgs<double>);
template __global__ void kfold_whiten_cols_kernel<double, LAYOUT_ROWVECS>(KfoldWhitenArgs<double>);
template __global__ void kfold_whiten_cols_kernel<float, LAYOUT_COLVECS>(KfoldWhitenArgs<float>);
template __global__ void kfold_whiten_cols_kernel<float, LAYOUT_ROWVECS>(KfoldWhitenArgs<float>);
template __global__ void kfold_cols_kernel<double>(KfoldColsArgs<double>);
template __global__ void kfold_cols_kernel<float>(KfoldColsArgs<float>);

}  // namespace blr
