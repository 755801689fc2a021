// The kernels of the ragged evidence grid (blr_grid_ragged.hpp) instantiated away from the rest of the library: a translation unit of
// its own, so the phase functions they share with fused_small_kernel and grid_eval_kernel are compiled for them separately and the
// code objects of the existing kernels stay as they are.  All NB = 1 .. 8, both element types; the statistics kernel with loader MODE
// 0 (ColVecs, generic), 1 (RowVecs) and 4 (ColVecs, LDS-DMA).  Host side: blr_abi.hip (logpdf_grid_ragged).  Development / sanitizer
// builds (-DBLR_DEV_FAST): <double, 8> only, the other shapes report a NULL kernel pointer.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "blr_grid_ragged.hpp"

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
const void* stats_ptr_nb(int mode) {
  if constexpr (kBuilt<T, NB>) switch (mode) {
    case 0: return reinterpret_cast<const void*>(ragged_evidence_stats_kernel<T, NB, 0>);
    case 1: return reinterpret_cast<const void*>(ragged_evidence_stats_kernel<T, NB, 1>);
    case 4: return reinterpret_cast<const void*>(ragged_evidence_stats_kernel<T, NB, 4>);
    default: break;
  }
  return nullptr;
}
template <typename T, int NB>
const void* eval_ptr_nb() {
  if constexpr (kBuilt<T, NB>) return reinterpret_cast<const void*>(ragged_evidence_eval_kernel<T, NB>);
  return nullptr;
}
template <typename T, int NB>
void stats_launch_nb(int mode, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<T>& a) {
  constexpr size_t lds = SmallCfg<T, NB>::LDS_BYTES;
  if constexpr (kBuilt<T, NB>) switch (mode) {
    case 0: hipLaunchKernelGGL((ragged_evidence_stats_kernel<T, NB, 0>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    case 1: hipLaunchKernelGGL((ragged_evidence_stats_kernel<T, NB, 1>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    case 4: hipLaunchKernelGGL((ragged_evidence_stats_kernel<T, NB, 4>), dim3(grid), dim3(kThreads), lds, stream, a); break;
    default: break;
  }
}
template <typename T, int NB>
void eval_launch_nb(unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<T>& a) {
  constexpr size_t lds = SmallCfg<T, NB>::LDS_BYTES;
  if constexpr (kBuilt<T, NB>) hipLaunchKernelGGL((ragged_evidence_eval_kernel<T, NB>), dim3(grid), dim3(kThreads), lds, stream, a);
}

// run f(std::integral_constant<int, NB>) for the run-time NB in 1 .. 8 (the callers have checked the range)
template <int NB = 1, typename F>
auto with_nb(int nb, F f) {
  if constexpr (NB == 8) return f(std::integral_constant<int, 8>{});
  else return nb == NB ? f(std::integral_constant<int, NB>{}) : with_nb<NB + 1>(nb, f);
}

template <typename T>
const void* stats_ptr_of(int NB, int mode) {
  return with_nb(NB, [&](auto nb) { return stats_ptr_nb<T, decltype(nb)::value>(mode); });
}
template <typename T>
const void* eval_ptr_of(int NB) {
  return with_nb(NB, [](auto nb) { return eval_ptr_nb<T, decltype(nb)::value>(); });
}
template <typename T>
size_t lds_of(int NB) {
  return with_nb(NB, [](auto nb) { return (size_t)SmallCfg<T, decltype(nb)::value>::LDS_BYTES; });
}
template <typename T>
int stat_elems_of(int NB) {
  return with_nb(NB, [](auto nb) { return evidence_stat_elems<T, decltype(nb)::value>(); });
}
template <typename T>
void stats_launch_of(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<T>& a) {
  with_nb(NB, [&](auto nb) { stats_launch_nb<T, decltype(nb)::value>(mode, grid, stream, a); });
}
template <typename T>
void reduce_launch_of(int NB, unsigned B, hipStream_t stream, const RaggedEvidenceArgs<T>& a) {
  hipLaunchKernelGGL(ragged_evidence_reduce_kernel<T>, dim3(B, 8), dim3(kThreads), 0, stream, a, stat_elems_of<T>(NB));
}
template <typename T>
void eval_launch_of(int NB, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<T>& a) {
  with_nb(NB, [&](auto nb) { eval_launch_nb<T, decltype(nb)::value>(grid, stream, a); });
}

}  // namespace

const void* ragged_evidence_stats_ptr_f64(int NB, int mode) { return stats_ptr_of<double>(NB, mode); }
const void* ragged_evidence_stats_ptr_f32(int NB, int mode) { return stats_ptr_of<float>(NB, mode); }
const void* ragged_evidence_eval_ptr_f64(int NB) { return eval_ptr_of<double>(NB); }
const void* ragged_evidence_eval_ptr_f32(int NB) { return eval_ptr_of<float>(NB); }
size_t ragged_evidence_lds_f64(int NB) { return lds_of<double>(NB); }
size_t ragged_evidence_lds_f32(int NB) { return lds_of<float>(NB); }
int ragged_evidence_stat_elems_f64(int NB) { return stat_elems_of<double>(NB); }
int ragged_evidence_stat_elems_f32(int NB) { return stat_elems_of<float>(NB); }
void ragged_evidence_stats_launch_f64(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<double>& a) {
  stats_launch_of<double>(NB, mode, grid, stream, a);
}
void ragged_evidence_stats_launch_f32(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<float>& a) {
  stats_launch_of<float>(NB, mode, grid, stream, a);
}
void ragged_evidence_reduce_launch_f64(int NB, unsigned B, hipStream_t stream, const RaggedEvidenceArgs<double>& a) {
  reduce_launch_of<double>(NB, B, stream, a);
}
void ragged_evidence_reduce_launch_f32(int NB, unsigned B, hipStream_t stream, const RaggedEvidenceArgs<float>& a) {
  reduce_launch_of<float>(NB, B, stream, a);
}
void ragged_evidence_eval_launch_f64(int NB, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<double>& a) {
  eval_launch_of<double>(NB, grid, stream, a);
}
void ragged_evidence_eval_launch_f32(int NB, unsigned grid, hipStream_t stream, const RaggedEvidenceArgs<float>& a) {
  eval_launch_of<float>(NB, grid, stream, a);
}

}  // namespace blr
