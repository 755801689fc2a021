// loo_x16_kernel (blr_loo_x16.hpp) in a translation unit of its own: the code objects of the marginal kernels on 16-bit features
// (blr_marg_x16.hip) and of every other kernel stay as they are.  Both formats x four loaders.  Host side: blr_abi.hip
// (blr_loo_batched_x16).
#include <hip/hip_runtime.h>

// (the planes' layout only: marg_planes_x16_kernel and marginals_x16_kernel are defined in blr_marg_x16.hip)
#define BLR_X16_DECLS_ONLY
#include "blr_marg_x16.hpp"
#undef BLR_X16_DECLS_ONLY
#include "blr_loo_x16.hpp"

namespace blr {
namespace {

template <int FMT>
const void* ptr_fmt(int mode) {
  switch (mode) {
    case 0: return reinterpret_cast<const void*>(loo_x16_kernel<FMT, 0>);
    case 1: return reinterpret_cast<const void*>(loo_x16_kernel<FMT, 1>);
    case 2: return reinterpret_cast<const void*>(loo_x16_kernel<FMT, 2>);
    case 3: return reinterpret_cast<const void*>(loo_x16_kernel<FMT, 3>);
    default: return nullptr;
  }
}
template <int FMT>
void launch_fmt(int mode, dim3 grid, size_t lds, hipStream_t stream, const LooX16Args& a) {
  switch (mode) {
    case 0: hipLaunchKernelGGL((loo_x16_kernel<FMT, 0>), grid, dim3(kThreads), lds, stream, a); break;
    case 1: hipLaunchKernelGGL((loo_x16_kernel<FMT, 1>), grid, dim3(kThreads), lds, stream, a); break;
    case 2: hipLaunchKernelGGL((loo_x16_kernel<FMT, 2>), grid, dim3(kThreads), lds, stream, a); break;
    case 3: hipLaunchKernelGGL((loo_x16_kernel<FMT, 3>), grid, dim3(kThreads), lds, stream, a); break;
    default: break;
  }
}

}  // namespace

const void* loo_x16_kernel_ptr(int fmt, int mode) { return fmt == 0 ? ptr_fmt<0>(mode) : ptr_fmt<1>(mode); }

void loo_x16_launch(int fmt, int mode, unsigned groups, unsigned nb, size_t lds, hipStream_t stream, const LooX16Args& a) {
  if (fmt == 0) launch_fmt<0>(mode, dim3(groups, nb), lds, stream, a);
  else launch_fmt<1>(mode, dim3(groups, nb), lds, stream, a);
}

}  // namespace blr
