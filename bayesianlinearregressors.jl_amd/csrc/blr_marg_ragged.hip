// The kernels of the ragged marginal stream and the ragged leave-one-out (blr_marg_ragged.hpp) instantiated in a translation unit
// of their own: the code objects of the existing kernels stay as they are.  Host side: blr_abi.hip (marg_ragged_launch).
#include <hip/hip_runtime.h>

#include "blr_marg_ragged.hpp"

namespace blr {

__global__ __launch_bounds__(kThreads) void loo_ragged_total_kernel(const double* __restrict__ ll, const int64_t* __restrict__ offsets,
                                                                    double* __restrict__ total, const int32_t* __restrict__ info) {
  const int64_t reg = blockIdx.x;
  if (info[reg] != 0) return;
  const int64_t o0 = offsets[reg];
  const double t = fixed_order_sum(ll + o0, offsets[reg + 1] - o0);  // (an empty regressor: 0)
  if (threadIdx.x == 0) total[reg] = t;
}

BLR_MARG_RAGGED_INSTANCES(template, double)
BLR_MARG_RAGGED_INSTANCES(template, float)

}  // namespace blr
