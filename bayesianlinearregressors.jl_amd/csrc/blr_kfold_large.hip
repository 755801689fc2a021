// The instantiations of the large-fold K-fold kernels (blr_kfold_large.hpp): both element types, every block count of the
// factorisation kernel, the fp64 statistics kernel with the three loaders of phase_gram the route uses, the fp32 statistics kernel.  Host side: blr_abi.hip (kfold_large_batched).
#include "blr_kfold_large.hpp"

namespace blr {

#define BLR_KFL_STATS(NB)                                                           \
  template __global__ void kfl_stats_kernel<double, NB, 0>(KflArgs<double>);        \
  template __global__ void kfl_stats_kernel<double, NB, 1>(KflArgs<double>);        \
  template __global__ void kfl_stats_kernel<double, NB, 4>(KflArgs<double>);
BLR_KFL_STATS(1) BLR_KFL_STATS(2) BLR_KFL_STATS(3) BLR_KFL_STATS(4) BLR_KFL_STATS(5) BLR_KFL_STATS(6) BLR_KFL_STATS(7) BLR_KFL_STATS(8)
template __global__ void kfl_stats32_kernel<LAYOUT_COLVECS>(KflArgs<float>);
template __global__ void kfl_stats32_kernel<LAYOUT_ROWVECS>(KflArgs<float>);
#define BLR_KFL_NB(T, NB) template __global__ void kfl_factor_kernel<T, NB>(KflArgs<T>);
#define BLR_KFL(T)                                                                                      \
  BLR_KFL_NB(T, 1) BLR_KFL_NB(T, 2) BLR_KFL_NB(T, 3) BLR_KFL_NB(T, 4) BLR_KFL_NB(T, 5) BLR_KFL_NB(T, 6) \
  BLR_KFL_NB(T, 7) BLR_KFL_NB(T, 8)                                                                     \
  template __global__ void kfl_state_kernel<T>(KflArgs<T>);                                             \
  template __global__ void kfl_reduce_kernel<T>(KflArgs<T>, int);                                       \
  template __global__ void kfl_predict_kernel<T, LAYOUT_COLVECS>(KflArgs<T>);                           \
  template __global__ void kfl_predict_kernel<T, LAYOUT_ROWVECS>(KflArgs<T>);
BLR_KFL(double)
BLR_KFL(float)

}  // namespace blr
