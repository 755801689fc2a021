// fused_ragged_kernel (blr_ragged.hpp) instantiated away from the rest of the library: a translation unit of its own, so the phase
// functions it shares with fused_small_kernel are compiled for it separately and the code objects of the existing kernels stay as
// they are.  All NB = 1 .. 8, both element types, loader MODE 0 (ColVecs, generic), 1 (RowVecs) and 4 (ColVecs, LDS-DMA).
// Host side: blr_abi.hip (posterior_ragged).  Development / sanitizer builds (-DBLR_DEV_FAST): <double, 8, *> only, the other
// shapes report a NULL kernel pointer.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "blr_ragged.hpp"

namespace blr {
namespace {

#if defined(BLR_DEV_FAST)
template <typename T, int NB>
constexpr bool kBuilt = sizeof(T) == 8 && NB == 8;
#else
template <typename T, int NB>
constexpr bool kBuilt = true;
#endif

template <typename T, int NB>
const void* ptr_nb(int mode) {
  if constexpr (kBuilt<T, NB>) switch (mode) {
    case 0: return reinterpret_cast<const void*>(fused_ragged_kernel<T, NB, 0>);
    case 1: return reinterpret_cast<const void*>(fused_ragged_kernel<T, NB, 1>);
    case 4: return reinterpret_cast<const void*>(fused_ragged_kernel<T, NB, 4>);
    default: break;
  }
  return nullptr;
}
template <typename T, int NB>
void launch_nb(int mode, unsigned grid, hipStream_t stream, const RaggedArgs<T>& a) {
  constexpr size_t lds = SmallCfg<T, NB>::LDS_BYTES;
  if constexpr (kBuilt<T, NB>) switch (mode) {
    case 0: hipLaunchKernelGGL((fused_ragged_kernel<T, NB, 0>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    case 1: hipLaunchKernelGGL((fused_ragged_kernel<T, NB, 1>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    case 4: hipLaunchKernelGGL((fused_ragged_kernel<T, NB, 4>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    default: break;
  }
}

// run f(std::integral_constant<int, NB>) for the run-time NB in 1 .. 8 (the callers have checked the range)
template <int NB = 1, typename F>
auto with_nb(int nb, F f) {
  if constexpr (NB == 8) return f(std::integral_constant<int, 8>{});
  else return nb == NB ? f(std::integral_constant<int, NB>{}) : with_nb<NB + 1>(nb, f);
}

template <typename T>
const void* ptr_of(int NB, int mode) {
  return with_nb(NB, [&](auto nb) { return ptr_nb<T, decltype(nb)::value>(mode); });
}
template <typename T>
size_t lds_of(int NB) {
  return with_nb(NB, [](auto nb) { return (size_t)SmallCfg<T, decltype(nb)::value>::LDS_BYTES; });
}
template <typename T>
void launch_of(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedArgs<T>& a) {
  with_nb(NB, [&](auto nb) { launch_nb<T, decltype(nb)::value>(mode, grid, stream, a); });
}

}  // namespace

const void* ragged_kernel_ptr_f64(int NB, int mode) { return ptr_of<double>(NB, mode); }
const void* ragged_kernel_ptr_f32(int NB, int mode) { return ptr_of<float>(NB, mode); }
size_t ragged_kernel_lds_f64(int NB) { return lds_of<double>(NB); }
size_t ragged_kernel_lds_f32(int NB) { return lds_of<float>(NB); }
void ragged_kernel_launch_f64(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedArgs<double>& a) {
  launch_of<double>(NB, mode, grid, stream, a);
}
void ragged_kernel_launch_f32(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedArgs<float>& a) {
  launch_of<float>(NB, mode, grid, stream, a);
}

}  // namespace blr
