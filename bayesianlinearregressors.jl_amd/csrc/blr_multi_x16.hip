// multi_cols_x16_kernel (blr_multi_x16.hpp) instantiated in a translation unit of its own: both formats, NB = 2, 4, 6, 8, loader
// MODE 0 .. 3, as fused_x16_kernel (blr_fused_x16.hip).  Host side: blr_abi.hip (blr_posterior_multi_batched_x16).
// Development / sanitizer builds (-DBLR_DEV_FAST): NB = 8 only, the other shapes report a NULL kernel pointer.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "blr_multi_x16.hpp"

namespace blr {
namespace {

#if defined(BLR_DEV_FAST)
template <int NB>
constexpr bool kBuilt = NB == 8;
#else
template <int NB>
constexpr bool kBuilt = true;
#endif

using KernelFn = void (*)(MultiX16Args);

template <int FMT, int NB>
KernelFn fn_nb(int mode) {
  if constexpr (kBuilt<NB>) switch (mode) {
    case 0: return multi_cols_x16_kernel<FMT, NB, 0>;
    case 1: return multi_cols_x16_kernel<FMT, NB, 1>;
    case 2: return multi_cols_x16_kernel<FMT, NB, 2>;
    case 3: return multi_cols_x16_kernel<FMT, NB, 3>;
    default: break;
  }
  return nullptr;
}

KernelFn fn(int fmt, int NB, int mode) {
  switch (NB) {
    case 2: return fmt == X16_BF16 ? fn_nb<X16_BF16, 2>(mode) : fn_nb<X16_F16, 2>(mode);
    case 4: return fmt == X16_BF16 ? fn_nb<X16_BF16, 4>(mode) : fn_nb<X16_F16, 4>(mode);
    case 6: return fmt == X16_BF16 ? fn_nb<X16_BF16, 6>(mode) : fn_nb<X16_F16, 6>(mode);
    default: return fmt == X16_BF16 ? fn_nb<X16_BF16, 8>(mode) : fn_nb<X16_F16, 8>(mode);
  }
}

}  // namespace

const void* multi_x16_kernel_ptr(int fmt, int NB, int mode) { return reinterpret_cast<const void*>(fn(fmt, NB, mode)); }

void multi_x16_kernel_launch(int fmt, int NB, int mode, unsigned B, unsigned passes, size_t lds, hipStream_t stream, const MultiX16Args& a) {
  if (const KernelFn k = fn(fmt, NB, mode)) hipLaunchKernelGGL(k, dim3(B, passes), dim3(kThreads), lds, stream, a);
}

}  // namespace blr
