// fused_x16_kernel (blr_fused_x16.hpp) instantiated in a translation unit of its own: the phase functions it shares with
// fused_small_kernel are compiled for it separately and the code objects of the existing kernels stay as they are.
// Both formats, NB = 2, 4, 6, 8 (the dispatch pads an odd block count up: the padding rows are zero in LDS and the factorisation
// walks ceil(D / 16) blocks whatever NB is), loader MODE 0 .. 3.  Host side: blr_abi.hip (blr_posterior_batched_x16).
// Development / sanitizer builds (-DBLR_DEV_FAST): NB = 8 only, the other shapes report a NULL kernel pointer.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "blr_fused_x16.hpp"

namespace blr {
namespace {

#if defined(BLR_DEV_FAST)
template <int NB>
constexpr bool kBuilt = NB == 8;
#else
template <int NB>
constexpr bool kBuilt = true;
#endif

template <int FMT, int NB>
const void* ptr_nb(int mode) {
  if constexpr (kBuilt<NB>) switch (mode) {
    case 0: return reinterpret_cast<const void*>(fused_x16_kernel<FMT, NB, 0>);
    case 1: return reinterpret_cast<const void*>(fused_x16_kernel<FMT, NB, 1>);
    case 2: return reinterpret_cast<const void*>(fused_x16_kernel<FMT, NB, 2>);
    case 3: return reinterpret_cast<const void*>(fused_x16_kernel<FMT, NB, 3>);
    default: break;
  }
  return nullptr;
}
template <int FMT, int NB>
void launch_nb(int mode, unsigned grid, hipStream_t stream, const X16Args& a) {
  constexpr size_t lds = X16Cfg<NB>::LDS_BYTES;
  if constexpr (kBuilt<NB>) switch (mode) {
    case 0: hipLaunchKernelGGL((fused_x16_kernel<FMT, NB, 0>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    case 1: hipLaunchKernelGGL((fused_x16_kernel<FMT, NB, 1>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    case 2: hipLaunchKernelGGL((fused_x16_kernel<FMT, NB, 2>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    case 3: hipLaunchKernelGGL((fused_x16_kernel<FMT, NB, 3>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    default: break;
  }
}

// run f(std::integral_constant<int, NB>) for the run-time NB in {2, 4, 6, 8} (the caller has checked it)
template <typename F>
auto with_nb(int nb, F f) {
  switch (nb) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

}  // namespace

const void* x16_kernel_ptr(int fmt, int NB, int mode) {
  return with_nb(NB, [&](auto nb) {
    return fmt == X16_BF16 ? ptr_nb<X16_BF16, decltype(nb)::value>(mode) : ptr_nb<X16_F16, decltype(nb)::value>(mode);
  });
}
size_t x16_kernel_lds(int NB) {
  return with_nb(NB, [](auto nb) { return (size_t)X16Cfg<decltype(nb)::value>::LDS_BYTES; });
}
void x16_kernel_launch(int fmt, int NB, int mode, unsigned grid, hipStream_t stream, const X16Args& a) {
  with_nb(NB, [&](auto nb) {
    if (fmt == X16_BF16) launch_nb<X16_BF16, decltype(nb)::value>(mode, grid, stream, a);
    else launch_nb<X16_F16, decltype(nb)::value>(mode, grid, stream, a);
  });
}

}  // namespace blr
