// The kernels of the ragged condition / forget pair (blr_revise_ragged.hpp) instantiated in a translation unit of their own.
// Host side: blr_abi.hip (revise_ragged).
#include <hip/hip_runtime.h>

#include "blr_fused_small.hpp"  // uni
#include "blr_revise_ragged.hpp"

namespace blr {

BLR_REVISE_RAGGED_INSTANCES(template, double)
BLR_REVISE_RAGGED_INSTANCES(template, float)

__global__ __launch_bounds__(kThreads) void revise_ragged_idle_kernel(const int64_t* offsets, int64_t B, double* logpdf, int32_t* info) {
  for (int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x; b < B; b += (int64_t)gridDim.x * kThreads) {
    if (offsets[b + 1] != offsets[b]) continue;
    info[b] = 0;
    if (logpdf) logpdf[b] = 0.0;
  }
}

}  // namespace blr
