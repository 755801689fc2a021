// ragged_x16_kernel, ragged_x16_part_kernel and ragged_x16_finish_kernel (blr_ragged_x16.hpp) instantiated in a translation unit of
// their own: the phase functions they share with fused_small_kernel and fused_ragged_kernel are compiled for them separately and the
// code objects of the existing kernels stay as they are.  Both formats, NB = 2, 4, 6, 8 (the dispatch pads an odd block count up, as
// for fused_x16_kernel), ColVecs and RowVecs; the loader is picked inside the kernels.  Host side: blr_abi.hip
// (blr_posterior_ragged_x16).  Development / sanitizer builds (-DBLR_DEV_FAST): NB = 8 only, the other shapes report a NULL pointer.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "blr_ragged_x16.hpp"

namespace blr {
namespace {

#if defined(BLR_DEV_FAST)
template <int NB>
constexpr bool kBuilt = NB == 8;
#else
template <int NB>
constexpr bool kBuilt = true;
#endif

using Kernel = void (*)(RaggedX16Args);

template <int FMT, int NB>
Kernel kernel_nb(int which, bool rowvecs) {
  if constexpr (kBuilt<NB>) switch (which) {
    case 0: return rowvecs ? ragged_x16_kernel<FMT, NB, true> : ragged_x16_kernel<FMT, NB, false>;
    case 1: return rowvecs ? ragged_x16_part_kernel<FMT, NB, true> : ragged_x16_part_kernel<FMT, NB, false>;
    case 2: return ragged_x16_finish_kernel<NB>;
    default: break;
  }
  return nullptr;
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

Kernel kernel_of(int which, int fmt, int NB, bool rowvecs) {
  return with_nb(NB, [&](auto nb) {
    return fmt == X16_BF16 ? kernel_nb<X16_BF16, decltype(nb)::value>(which, rowvecs) : kernel_nb<X16_F16, decltype(nb)::value>(which, rowvecs);
  });
}

}  // namespace

const void* ragged_x16_kernel_ptr(int which, int fmt, int NB, bool rowvecs) {
  return reinterpret_cast<const void*>(kernel_of(which, fmt, NB, rowvecs));
}
size_t ragged_x16_kernel_lds(int which, int NB) {
  return with_nb(NB, [&](auto nb) {
    constexpr int N = decltype(nb)::value;
    return which == 2 ? (size_t)SmallCfg<float, N>::LDS_BYTES : (size_t)X16Cfg<N>::LDS_BYTES;
  });
}
size_t ragged_x16_packed_elems(int NB) {
  return with_nb(NB, [](auto nb) { return (size_t)SmallCfg<float, decltype(nb)::value>::PACKED; });
}
void ragged_x16_kernel_launch(int which, int fmt, int NB, bool rowvecs, unsigned grid, hipStream_t stream, const RaggedX16Args& a) {
  const Kernel k = kernel_of(which, fmt, NB, rowvecs);
  if (k) hipLaunchKernelGGL(k, dim3(grid), dim3(kThreads), ragged_x16_kernel_lds(which, NB), stream, a);
}

}  // namespace blr
