// Host side of the C ABI declared in include/blr_mi355x.h: argument validation, host<->device
// staging for BLR_MEM_HOST calls, kernel dispatch.  No exception crosses the boundary.
#include "../../include/blr_mi355x.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the symbols are resolved with dlopen / dlsym on first use
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <functional>
#include <map>
#include <queue>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "blr_aux_kernels.hpp"
#include "blr_fused_small.hpp"
#include "blr_large.hpp"
#include "blr_planes.hpp"
#include "blr_dense.hpp"
#include "blr_update.hpp"
#include "blr_downdate.hpp"
#include "blr_fused_wave.hpp"
#include "blr_fused_i8.hpp"
#include "blr_marginals.hpp"
#include "blr_rand_batched.hpp"
#include "blr_grid.hpp"
#include "blr_ragged.hpp"
#include "blr_marg_ragged.hpp"
#include "blr_multi.hpp"
#include "blr_marg_multi.hpp"
#include "blr_cov_batched.hpp"
#include "blr_loo_multi.hpp"
#include "blr_state_cols.hpp"
#include "blr_rand_multi.hpp"
#include "blr_kfold.hpp"
#include "blr_kfold_large.hpp"
#include "blr_kfold_multi.hpp"
#include "blr_kfold_ragged.hpp"
#include "blr_kfold_large_ragged.hpp"
#include "blr_revise_ragged.hpp"
#include "blr_grid_ragged.hpp"
#include "blr_host.hpp"
#include "blr_large_plan.hpp"

using namespace blr;

// ---- the non-template kernels declared in blr_aux_kernels.hpp and blr_loo.hpp: their one definition ------------------------------
namespace blr {

__global__ __launch_bounds__(kThreads) void logpdf_sum_kernel(const double* __restrict__ lp, int64_t B,
                                                              double* __restrict__ total) {
  const double t = fixed_order_sum(lp, B);
  if (threadIdx.x == 0) *total = t;
}

// loo_total[reg] = sum_n logpdf_n in a fixed order (no float atomics: the same bits at any B and position)
__global__ __launch_bounds__(kThreads) void loo_total_kernel(const double* __restrict__ ll, int64_t stride_ll, int N,
                                                             double* __restrict__ total, const int32_t* __restrict__ info, int reg0) {
  const int64_t reg = reg0 + (int64_t)blockIdx.x;
  if (info[reg] != 0) return;
  const double t = fixed_order_sum(ll + reg * stride_ll, N);
  if (threadIdx.x == 0) total[reg] = t;
}

}  // namespace blr

namespace {

// ---- RCCL, bound at run time -------------------------------------------------------------------------------------
// The library has no link-time dependency on librccl: a single-GPU host never loads it, and a process that already has a
// RCCL (PyTorch ships one) gets that one.  Only the calls of the path's single exchange are bound.
struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
  std::string why;
};
RcclApi& rccl() {
  static RcclApi api = [] {
    RcclApi a;
    void* lib = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) { a.why = std::string("librccl not found: ") + dlerror(); return a; }
    auto sym = [&](const char* n) { return dlsym(lib, n); };
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(sym("ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(sym("ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(sym("ncclCommDestroy"));
    a.AllGather = reinterpret_cast<decltype(a.AllGather)>(sym("ncclAllGather"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(sym("ncclAllReduce"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("ncclGetErrorString"));
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllGather && a.AllReduce && a.GetErrorString;
    if (!a.ok) a.why = "librccl lacks a required symbol";
    return a;
  }();
  return api;
}
int rccl_fail(blr_handle* h, ncclResult_t r, const char* what) {
  if (h) h->err = std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(r) : "RCCL error");
  return -(2000 + (int)r);
}

constexpr int kMaxSmallD = 128;
constexpr int kMaxLargeD = 8192;


int set_lds_once(blr_handle* h, const void* kern, size_t bytes) {
  auto it = h->lds_limit.find(kern);
  if (it != h->lds_limit.end() && it->second >= bytes) return 0;
  HIP_TRY(h, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  h->lds_limit[kern] = bytes;
  return 0;
}

template <typename... Args>
int set_lds_once(blr_handle* h, void (*kern)(Args...), size_t bytes) {  // (a kernel by its name: no cast at the call)
  return set_lds_once(h, reinterpret_cast<const void*>(kern), bytes);
}

// Calls nested inside an entry point (device operands) must not drain the stream -- or, blr_posterior_ragged_*, must: the handle's
// mode for the lifetime of this object, the caller's again afterwards.
struct AsyncScope {
  blr_handle* const h;
  const bool was;
  AsyncScope(blr_handle* hh, bool async) : h(hh), was(hh->async) { h->async = async; }
  ~AsyncScope() { h->async = was; }
  AsyncScope(const AsyncScope&) = delete;
  AsyncScope& operator=(const AsyncScope&) = delete;
};

int bad_arg(blr_handle* h, int pos, const char* why) {
  if (h) h->err = std::string("argument ") + std::to_string(pos) + ": " + why;
  return -pos;
}

int ensure_stats(blr_handle* h) {
  if (h->stats_dev) return 0;
  HIP_TRY(h, hipMalloc((void**)&h->stats_dev, 16 * sizeof(unsigned long long)));
  HIP_TRY(h, hipMemsetAsync(h->stats_dev, 0, 16 * sizeof(unsigned long long), h->stream));
  return 0;
}

// The handle's counter words and the exchange buffer of backsolve_wave_kernel: zero at allocation, afterwards only written by
// that kernel with launch epochs that are never reused, so a stale granule can never carry the current tag.
int ensure_xchg(blr_handle* h, size_t bytes) {
  if (!h->ticket) {
    HIP_TRY(h, hipMalloc((void**)&h->ticket, 2048));
    HIP_TRY(h, hipMemsetAsync(h->ticket, 0, 2048, h->stream));
  }
  return h->xchg.reserve(h, bytes, blr_handle::kXchgFloor, true);
}
template <typename T>
constexpr size_t wave_solve_lds() {
  return (((size_t)kPB * (kPB + 1) / 2 * sizeof(T) + 15) & ~(size_t)15) + 3 * kPB * sizeof(T) + 8 * sizeof(double) + 16;
}
// launches one wavefront solve of NC x S workgroups; fills the synchronisation fields of `b`
template <typename T>
int launch_wave_solve(blr_handle* h, WaveSolveArgs<T>& b, int NC, int64_t S) {
  int rc = ensure_xchg(h, (size_t)S * b.DP * 2 * sizeof(unsigned long long));
  if (rc) return rc;
  b.xchg = reinterpret_cast<unsigned long long*>(h->xchg.p); b.ticket = h->ticket;  // tickets, the launch count behind the granule tags: device-side (WaveSolveArgs)
  if (const int rc_lds = set_lds_once(h, backsolve_wave_kernel<T>, (size_t)((int)wave_solve_lds<T>()))) return rc_lds;
  hipLaunchKernelGGL(backsolve_wave_kernel<T>, dim3(NC, (unsigned)S), dim3(kThreads), wave_solve_lds<T>(), h->stream, b);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return hip_fail(h, le, "launch of backsolve_wave_kernel");  // nothing ran: the counters did not move
  return 0;
}

size_t extent(int64_t B, int64_t stride, size_t one) {  // elements spanned by B items at `stride`
  if (B <= 0) return 0;
  return (size_t)((B - 1) * stride) + one;
}
size_t mat_extent(int64_t rows, int64_t cols, int64_t ld) {
  if (rows <= 0 || cols <= 0) return 0;
  return (size_t)((cols - 1) * ld + rows);
}

template <typename T>
bool aligned16(const T* p, int64_t ld, int64_t stride) {
  return ((uintptr_t)p % 16 == 0) && ((ld * (int64_t)sizeof(T)) % 16 == 0) && ((stride * (int64_t)sizeof(T)) % 16 == 0);
}

// ---- fused small-D dispatch -----------------------------------------------------------------------
template <typename T, int NB, int MODE>
int launch_fused_small(blr_handle* h, const PosteriorArgs<T>& a) {
  using C = SmallCfg<T, NB>;
  auto kern = fused_small_kernel<T, NB, MODE>;
  // every launch: the attribute is per DEVICE, and handles on different devices share this code (a process-wide
  // "already set" flag left the second device at the 64 KB default)
  if (const int rc_lds = set_lds_once(h, kern, (size_t)(C::LDS_BYTES))) return rc_lds;
  int grid = (int)std::min<int64_t>(a.B, 1 << 20);
  if (a.retry_only) grid = std::min(grid, 2 * h->cus);  // (one round of workgroups, each walking its share: see the kernel's head)
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), C::LDS_BYTES, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  if (!a.retry_only) {
    static const std::string name = std::string("fused_small_kernel<") + (sizeof(T) == 8 ? "double" : "float") + ", " + std::to_string(NB) + ", " +
                                    std::to_string(MODE) + ">";
    h->route = name.c_str();
    h->route_i8_B = 0;
  }
  return 0;
}

template <typename T, int NB>
int launch_fused_small_mode(blr_handle* h, const PosteriorArgs<T>& a) {
  if (a.layout == BLR_LAYOUT_ROWVECS) return launch_fused_small<T, NB, 1>(h, a);
  if (a.vec_ok) {
    if (h->opt.no_ldsdma) return launch_fused_small<T, NB, 3>(h, a);  // A/B experiments only
    return launch_fused_small<T, NB, 4>(h, a);
  }
  return launch_fused_small<T, NB, 0>(h, a);
}

// D = 32 / 64, ColVecs with aligned columns: one wavefront per regressor (blr_fused_wave.hpp)
template <typename T, int NB, int NW>
int launch_fused_wave_nw(blr_handle* h, const PosteriorArgs<T>& a) {
  using C = WaveCfg<T, NB>;
  const int grid = (int)std::min<int64_t>(a.B, (int64_t)h->cus * 8 / NW);  // 8 waves per CU (18.6 KB of LDS each)
  if (NW * C::LDS_BYTES > 64 * 1024) {
    int rc = set_lds_once(h, fused_wave_kernel<T, NB, NW>, (size_t)NW * C::LDS_BYTES);
    if (rc) return rc;
  }
  hipLaunchKernelGGL((fused_wave_kernel<T, NB, NW>), dim3(grid), dim3(64 * NW), NW * C::LDS_BYTES, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  static const std::string name = std::string("fused_wave_kernel<") + (sizeof(T) == 8 ? "double" : "float") + ", " + std::to_string(NB) + ", " +
                                  std::to_string(NW) + ">";
  h->route = name.c_str();
  h->route_i8_B = 0;
  return 0;
}
// The chip has 2048 wave slots for this kernel.  A batch that cannot fill them with one regressor per wave splits each
// regressor's observations over 2 or 4 waves instead (BLR_MI355X_WAVE_SPLIT=1|2|4 overrides; the tests run all three).
template <typename T, int NB>
int launch_fused_wave(blr_handle* h, const PosteriorArgs<T>& a) {
  int nw = a.B >= 2048 ? 1 : (a.B >= 1024 ? 2 : 4);
  if (h->opt.wave_split) nw = h->opt.wave_split;
  if (nw == 1) return launch_fused_wave_nw<T, NB, 1>(h, a);
  if (nw == 2) return launch_fused_wave_nw<T, NB, 2>(h, a);
  return launch_fused_wave_nw<T, NB, 4>(h, a);
}

// D = 128, fp64, aligned ColVecs, isotropic noise, diagonal prior, whole 32-column k-steps: the Gram matrix on the int8 matrix
// cores (blr_fused_i8.hpp), followed by the fp64 kernel in retry-only mode for the regressors the fast path handed back
// (a row bound broken, non-finite input): every regressor leaves with the status and the numbers of an
// fp64-accurate update, none is computed twice on the fast path.
constexpr size_t kSmall8Lds = SmallCfg<double, 8>::LDS_BYTES;
int launch_fused_i8(blr_handle* h, const PosteriorArgs<double>& a) {
  const bool diag = a.noise_kind == BLR_NOISE_DIAGONAL, rowv = a.layout == BLR_LAYOUT_ROWVECS;
  // (the kernel's four instantiations: blr_i8_kernels.hip)
  // (default plans: six digit groups under isotropic noise, seven under diagonal noise; option I8_GROUPS asks for the other one)
  const int groups_default = diag ? kI8GroupsDiag : kI8GroupsIso;
  const bool alt = h->opt.i8_groups != 0 && h->opt.i8_groups != groups_default && i8_kernel_ptr_alt(diag, rowv) != nullptr;
  const int groups = alt ? h->opt.i8_groups : groups_default;
  const void* const kern = alt ? i8_kernel_ptr_alt(diag, rowv) : (diag ? i8_kernel_ptr_diag(rowv) : i8_kernel_ptr_iso(rowv));
  if (kern == nullptr) return hip_fail(h, hipErrorInvalidValue, "this build lacks the requested form of the int8 kernel");
  int rc = set_lds_once(h, kern, (size_t)I8Cfg::LDS_BYTES);
  if (rc) return rc;
  if ((rc = ensure_stats(h))) return rc;
  // diagonal noise: y / sqrt(s), 1 / sqrt(s), sum log s and a validity flag per regressor, once per call, in a side buffer of the
  // handle (16 bytes per observation: slices of at most 1 GiB)
  const int64_t per_reg = 2 * (int64_t)a.N * (int64_t)sizeof(double);
  const int grid = (int)h->cap_chunk(std::min<int64_t>(a.B, diag ? std::max<int64_t>(1, ((int64_t)1 << 30) / per_reg) : (1 << 20)));
  double *yt = nullptr, *rw = nullptr, *ld = nullptr, *rmx = nullptr;
  int32_t* bad = nullptr;
  // dense prior: logdet Lw and the status of its Cholesky per prior, from i8_prior_logdet_kernel (ONE prior when the batch shares it)
  const bool dense = a.prior_kind == BLR_PRIOR_DENSE;
  const bool shared_prior = a.strideLw == 0 || a.B == 1;
  double* pld = nullptr;
  int32_t* pinfo = nullptr;
  size_t o_prior = 0;
  if (diag) {
    const size_t o_rw = (((size_t)grid * a.N * sizeof(double)) + 255) & ~(size_t)255;
    o_prior = 2 * o_rw + 2 * (((size_t)grid * sizeof(double) + 255) & ~(size_t)255) + (((size_t)grid * sizeof(int32_t) + 255) & ~(size_t)255);
  }
  if (dense) {
    const size_t np = shared_prior ? 1 : (size_t)grid;
    if ((rc = h->i8side.reserve(h, o_prior + ((np * sizeof(double) + 255) & ~(size_t)255) + np * sizeof(int32_t)))) return rc;
    if ((rc = set_lds_once(h, i8_prior_logdet_kernel, kSmall8Lds))) return rc;
  }
  if (diag) {
    const size_t o_rw = (((size_t)grid * a.N * sizeof(double)) + 255) & ~(size_t)255;
    const size_t o_ld = 2 * o_rw, o_mx = o_ld + (((size_t)grid * sizeof(double) + 255) & ~(size_t)255);
    const size_t o_bad = o_mx + (((size_t)grid * sizeof(double) + 255) & ~(size_t)255);
    if (!dense && (rc = h->i8side.reserve(h, o_bad + (size_t)grid * sizeof(int32_t)))) return rc;
    yt = reinterpret_cast<double*>(h->i8side.p); rw = reinterpret_cast<double*>(h->i8side.p + o_rw);
    ld = reinterpret_cast<double*>(h->i8side.p + o_ld); rmx = reinterpret_cast<double*>(h->i8side.p + o_mx); bad = reinterpret_cast<int32_t*>(h->i8side.p + o_bad);
  }
  // Slices: one workgroup per regressor (batches beyond 2^20, or beyond the side buffer, in several launches).  A batch of more than
  // kI8ProbeMin = 4096 regressors (option I8_PROBE_MIN) starts with a PROBE slice of kI8Probe (one round of workgroups on the chip): every later slice reads how
  // many regressors of the slice before it the fast path had to hand back, and when that was more than a quarter its workgroups
  // leave their regressors to the fp64 kernel at once instead of streaming them twice (heavy-tailed inputs: blr_get_stat
  // "i8_handed_back").  The decision depends on the data of the previous slice only: same inputs, same bits.
  if (dense) {
    const size_t np = shared_prior ? 1 : (size_t)grid;
    pld = reinterpret_cast<double*>(h->i8side.p + o_prior);
    pinfo = reinterpret_cast<int32_t*>(h->i8side.p + o_prior + ((np * sizeof(double) + 255) & ~(size_t)255));
    if (shared_prior) {
      hipLaunchKernelGGL(i8_prior_logdet_kernel, dim3(1), dim3(kThreads), kSmall8Lds, h->stream, a.Lw, a.ldl, (int64_t)0, 1, pld, pinfo);
      HIP_TRY(h, hipGetLastError());
    }
  }
  int64_t b0 = 0;
  int prev_n = 0;
  h->last_chunks = 0;
  while (b0 < a.B) {
    PosteriorArgs<double> s = a;
    int64_t want = std::min<int64_t>(grid, a.B - b0);
    if (b0 == 0 && a.B > (h->opt.i8_probe_min > 0 ? h->opt.i8_probe_min : kI8ProbeMin) && !h->opt.no_i8_fallback) want = std::min<int64_t>(want, kI8Probe);
    const int nb = (int)want;
    s.B = nb;
    s.X += b0 * a.strideX; s.y += b0 * a.stridey; s.s += b0 * a.strides; s.mw += b0 * a.stridemw; s.Lw += b0 * a.strideLw;
    if (s.mw_post) s.mw_post += b0 * a.stride_mwpost;
    if (s.T_post) s.T_post += b0 * a.strideT;
    if (s.Lw_post) s.Lw_post += b0 * a.strideLp;
    if (s.logpdf) s.logpdf += b0;
    s.info += b0;
    s.i8_handed_tot = h->stats_dev;
    s.i8_call_base = b0 == 0 ? h->stats_dev + 2 : nullptr;
    s.i8_handed_slice = h->stats_dev + 8 + (h->i8_slices & 1u);         // zeroed by this slice's int8 launch, counted up by its retry launch
    s.i8_prev_handed = h->stats_dev + 8 + ((h->i8_slices & 1u) ^ 1u);   // final since the previous slice's retry launch
    s.i8_prev_n = h->opt.no_i8_fallback ? 0 : prev_n;
    ++h->i8_slices;
    if (diag) {
      s.i8_yt = yt; s.i8_rw = rw; s.i8_stride = a.N; s.i8_logdet = ld; s.i8_bad = bad; s.i8_rwmax = rmx;
      hipLaunchKernelGGL(i8_noise_prep_kernel, dim3(nb), dim3(kThreads), 0, h->stream, s.s, a.strides, s.y, a.stridey, (int)a.N, yt, rw, (int64_t)a.N, ld,
                         bad, rmx);
    }
    if (dense) {
      if (!shared_prior) {
        hipLaunchKernelGGL(i8_prior_logdet_kernel, dim3(std::min(nb, 2 * h->cus)), dim3(kThreads), kSmall8Lds, h->stream, s.Lw, a.ldl,
                           a.strideLw, nb, pld, pinfo);
        HIP_TRY(h, hipGetLastError());
      }
      s.i8_prior_logdet = pld; s.i8_prior_info = pinfo; s.i8_prior_stride = shared_prior ? 0 : 1;
    }
    if (alt) i8_kernel_launch_alt(diag, rowv, (unsigned)nb, h->stream, s);
    else if (diag) i8_kernel_launch_diag(rowv, (unsigned)nb, h->stream, s);
    else i8_kernel_launch_iso(rowv, (unsigned)nb, h->stream, s);
    HIP_TRY(h, hipGetLastError());
    s.retry_only = 1;
    if ((rc = launch_fused_small_mode<double, 8>(h, s))) return rc;
    h->i8_attempted += (unsigned long long)nb;
    prev_n = nb;
    b0 += nb;
    ++h->last_chunks;
  }
  h->route = !alt ? "fused_i8_kernel" : (groups == 7 ? "fused_i8_kernel (7 digit groups)" : "fused_i8_kernel (6 digit groups)");
  h->route_i8_B = a.B;
  return 0;
}

template <typename T>
int dispatch_fused_small(blr_handle* h, const PosteriorArgs<T>& a) {
  int NB = (a.D + 15) / 16;
  if constexpr (sizeof(T) == 8) {
    // (RowVecs: a feature's 32 observations of a k-step are 16 DMA lanes of 16 bytes: rows and regressors 16-byte aligned)
    const bool i8_layout = a.layout == BLR_LAYOUT_COLVECS
                               ? a.vec_ok
                               : (!h->opt.no_i8_rowvecs && ((uintptr_t)a.X & 15) == 0 && (a.ldx & 1) == 0 && (a.B == 1 || (a.strideX & 1) == 0));
    const bool i8_built = (a.noise_kind == BLR_NOISE_DIAGONAL ? i8_kernel_ptr_diag(a.layout == BLR_LAYOUT_ROWVECS) : i8_kernel_ptr_iso(a.layout == BLR_LAYOUT_ROWVECS)) != nullptr;
    if (i8_built && !h->opt.no_i8_gram && !h->opt.no_ldsdma && a.D == 128 && i8_layout &&
        (a.noise_kind == BLR_NOISE_ISOTROPIC || (a.noise_kind == BLR_NOISE_DIAGONAL && !h->opt.no_i8_diag)) &&
        (a.prior_kind == BLR_PRIOR_DIAGONAL || (a.prior_kind == BLR_PRIOR_UPPER_FACTOR && !h->opt.no_i8_factor) ||
         (a.prior_kind == BLR_PRIOR_DENSE && !h->opt.no_i8_dense)) && a.N - a.N % I8Cfg::KC >= kI8MinN && a.N - a.N % I8Cfg::KC <= kI8MaxN && a.ldx * 8 * I8Cfg::KC < ((int64_t)1 << 31))
      return launch_fused_i8(h, a);
  }
  if (!h->opt.no_wave_kernel && a.layout == BLR_LAYOUT_COLVECS && a.vec_ok && a.D == 16 * NB &&
      (3 * a.ldx + 64) * (int64_t)sizeof(T) < ((int64_t)1 << 31)) {
    if (NB == 4) return launch_fused_wave<T, 4>(h, a);
    if constexpr (sizeof(T) == 8) {
      if (NB == 2) return launch_fused_wave<T, 2>(h, a);
    }
  }
  switch (NB) {
    case 1: return launch_fused_small_mode<T, 1>(h, a);
    case 2: return launch_fused_small_mode<T, 2>(h, a);
    case 3: return launch_fused_small_mode<T, 3>(h, a);
    case 4: return launch_fused_small_mode<T, 4>(h, a);
    case 5: return launch_fused_small_mode<T, 5>(h, a);
    case 6: return launch_fused_small_mode<T, 6>(h, a);
    case 7: return launch_fused_small_mode<T, 7>(h, a);
    case 8: return launch_fused_small_mode<T, 8>(h, a);
    default: return bad_arg(h, 5, "D > 128 is not supported by this build");
  }
}

// ---- large-D path (D > 128): multi-kernel pipeline of blr_large.hpp ---------------------------------------------
constexpr int kChainBatchMaxWords = 128;  // = kChainBatchMax below

// In-place blocked (128) right-looking Cholesky of the lower triangle of M (nrows_total x DP, ld); rows beyond DP
// (the right-hand-side block of the augmented matrix) are carried through the TRSM and the trailing updates.
template <typename T, int ER>
int launch_panel(blr_handle* h, T* M, int64_t ld, int p, int nrows_total, int nbelow, int32_t* info_dev, int G, int64_t batch_stride,
                 int info_stride) {
  constexpr int NW = BLR_PANEL_WAVES;
  using CC = ChainCfg<T, NW, ER>;
  int rc;
  if ((rc = set_lds_once(h, panel_chain_kernel<T, NW, ER>, (size_t)CC::LDS_BYTES))) return rc;
  const int nwg = std::max(1, (nbelow + ER - 1) / ER);
  // arrival counters (one per factorisation of the launch): count up to nwg during the launch.  Two banks, used alternately
  // by the launches of this handle (= of its stream, in order); a launch clears the bank of its successor (blr_panel.hpp).
  // Forward progress of the wait inside the kernel: workgroup 0 waits for workgroups of ITS OWN launch only, every one of
  // which arrives after its loads without waiting for anybody -- so it holds for any dispatch order as long as each
  // workgroup is eventually scheduled, which a grid of at most one workgroup per CU (callers: G * nwg <= cus, or ER = 32
  // and D <= 8192) always is; beyond that the bounded spin reports -999 instead of a wrong factor.
  static_assert(kChainBatchMaxWords == kPanelArriveWords, "one arrival word per factorisation of a group");
  unsigned* const bank = h->ticket + 16 + kPanelArriveWords * (h->panel_launches & 1u);
  unsigned* const next = h->ticket + 16 + kPanelArriveWords * ((h->panel_launches & 1u) ^ 1u);
  ++h->panel_launches;
  hipLaunchKernelGGL((panel_chain_kernel<T, NW, ER>), dim3(nwg, G), dim3(64 * NW), CC::LDS_BYTES, h->stream, M, ld, p * kPB, nrows_total,
                     info_dev, bank, (unsigned)nwg, batch_stride, info_stride, next);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

constexpr int kChainBatchMax = kChainBatchMaxWords;  // factorisations that step through their panels in shared launches (one arrival word each per bank)

// Blocked Cholesky of G independent matrices M + g * batch_stride (status words info_dev + g * info_stride), panel by panel,
// every step ONE launch over all of them.
template <typename T>
int chol_large(blr_handle* h, T* M, int64_t ld, int DP, int nrows_total, int32_t* info_dev, int G = 1, int64_t batch_stride = 0,
               int info_stride = 0) {
  const int NC = DP / kPB;
  int rc;
  if (G < 1 || G > kChainBatchMax) return hip_fail(h, hipErrorInvalidValue, "chol_large: too many factorisations per launch");
  if ((rc = ensure_xchg(h, 0))) return rc;  // the handle's counter words (ticket[16 + g]: arrivals of panel_chain_kernel)
  if ((rc = set_lds_once(h, trail_update_kernel<T>, (size_t)TrailCfg<T>::LDS_BYTES))) return rc;
  for (int p = 0; p < NC; ++p) {
    // L_pp and X <- X L_pp^-T for the rows below.  Every workgroup factors L_pp and takes 16 or 32 of those rows along: the
    // fewer, the shorter the launch (the update waves are its bottleneck) -- as long as every workgroup has a CU to itself
    // (D <= 8192: at most 8128 rows below a block, 254 workgroups of 32)
    const int nbelow = nrows_total - (p + 1) * kPB;
    const int cus = h->cus;
    if ((int64_t)G * ((nbelow + 15) / 16) <= cus) rc = launch_panel<T, 16>(h, M, ld, p, nrows_total, nbelow, info_dev, G, batch_stride, info_stride);
    else rc = launch_panel<T, 32>(h, M, ld, p, nrows_total, nbelow, info_dev, G, batch_stride, info_stride);
    if (rc) return rc;
    const int m = NC - 1 - p;  // remaining column blocks
    if (m > 0) {
      const int ntri = 2 * m;                                   // 64-row sub-blocks of the remaining triangle
      const int nextra = (nrows_total - DP) / TrailCfg<T>::SB;  // rhs rows below the square part
      const int ntiles = ntri * (ntri + 1) / 2 + nextra * ntri;
      const int slots = h->cus * (TrailCfg<T>::LDS_BYTES <= 80 * 1024 ? 2 : 1);  // sub-tiles the chip holds at once
      const int gx = std::min(ntiles, std::max(1, slots / G));
      hipLaunchKernelGGL(trail_update_kernel<T>, dim3(gx, G), dim3(kThreads), TrailCfg<T>::LDS_BYTES, h->stream, M, ld,
                         p, ntri, (p + 1) * kPB, DP, (const int32_t*)info_dev, ntiles, batch_stride, info_stride);
      HIP_TRY(h, hipGetLastError());
    }
  }
  HIP_TRY(h, hipGetLastError());
  return 0;
}

// ---- the update of a group: plan (blr_large_plan.hpp: route, splits, workspace layout, group size -- no device needed), reserve,
// bind the workspace, run the stages.  What every stage sees: the call, the plan and the typed workspace pointers.  Every launch
// covers the whole group: regressor g from blockIdx.y / .z, its caller-side arrays by the batch strides and its workspace `wsb`
// bytes after its predecessor's (the pointers here are regressor reg0's).
template <typename T>
struct LargeRun {
  blr_handle* h;
  const PosteriorArgs<T>& a;
  const LargePlan& p;
  blr_handle::MultiSrc* ms;
  int64_t reg0;
  int G;
  const T *X, *y, *s, *mw, *Lw;
  T *Abar, *W, *Gpart, *mu, *rvec, *wvec, *Tfull;  // (mu: multi-output only; wvec: diagonal noise only)
  unsigned short* Xp;
  double *bpart, *qsp, *qpart, *lpart;
  unsigned* rowmax;  // behind the b partials: DPA words, then the planes pass's redo flag
  unsigned* scratch;  // LargeScratch
  double *logdetLw, *spare_logdet;
  int32_t *info_prior, *info_chol, *spare_info;
  unsigned* info_noise;
  int64_t wsb, wse;  // stride between the regressors' workspaces in bytes and in elements (a multiple of 256 bytes)
  int info_stride;   // ... and in status words
};
template <typename T>
LargeRun<T> bind_large(blr_handle* h, const PosteriorArgs<T>& a, const LargePlan& p, int64_t reg0, int G) {
  LargeRun<T> u{h, a, p, h->multi_src, reg0, G};
  u.X = a.X + reg0 * a.strideX; u.y = a.y + reg0 * a.stridey; u.s = a.s + reg0 * a.strides;
  u.mw = a.mw + reg0 * a.stridemw; u.Lw = a.Lw + reg0 * a.strideLw;
  char* const ws = h->ws.p;
  const LargeLayout& o = p.o;
  u.Abar = reinterpret_cast<T*>(ws + o.abar);
  u.W = reinterpret_cast<T*>(ws + o.w);
  u.Xp = reinterpret_cast<unsigned short*>(ws + o.xp);
  u.Gpart = reinterpret_cast<T*>(ws + o.gp);
  u.bpart = reinterpret_cast<double*>(ws + o.bp);
  u.rowmax = reinterpret_cast<unsigned*>(u.bpart + (int64_t)p.bslots * p.NCA * kPB);
  u.mu = u.ms ? reinterpret_cast<T*>(ws + o.mu) : nullptr;
  u.qsp = u.ms ? reinterpret_cast<double*>(ws + o.qs) : nullptr;
  u.rvec = reinterpret_cast<T*>(ws + o.r);
  u.wvec = a.noise_kind == NOISE_DIAGONAL ? reinterpret_cast<T*>(ws + o.wv) : nullptr;
  u.qpart = reinterpret_cast<double*>(ws + o.q);
  u.lpart = reinterpret_cast<double*>(ws + o.l);
  u.Tfull = reinterpret_cast<T*>(ws + o.m);
  char* const sc = ws + o.sc;
  u.scratch = reinterpret_cast<unsigned*>(sc);
  u.logdetLw = reinterpret_cast<double*>(sc + LargeScratch::logdet);
  u.info_prior = reinterpret_cast<int32_t*>(sc + LargeScratch::info_prior);
  u.info_chol = reinterpret_cast<int32_t*>(sc + LargeScratch::info_chol);
  u.info_noise = reinterpret_cast<unsigned*>(sc + LargeScratch::info_noise);
  u.spare_info = reinterpret_cast<int32_t*>(sc + LargeScratch::spare_info);
  u.spare_logdet = reinterpret_cast<double*>(sc + LargeScratch::spare_logdet);
  u.wsb = (int64_t)o.per;
  u.wse = (int64_t)(o.per / sizeof(T));
  u.info_stride = (int)(o.per / sizeof(int32_t));
  return u;
}

// ---- prior: SPD check + logdet (reference :78).  One launch clears the scratch words, sets the noise flag and zeroes the
// b partials; for a diagonal / factor prior it also checks the diagonal and seeds info_chol with the prior's status (a failed
// prior short-circuits the factorisation), for a dense one the blocked factorisation of W does that.
template <typename T>
int large_prior(const LargeRun<T>& u) {
  blr_handle* const h = u.h;
  const PosteriorArgs<T>& a = u.a;
  const LargePlan& p = u.p;
  const bool dense = a.prior_kind == PRIOR_DENSE;
  ScratchInit init;
  init.words16 = u.scratch;
  init.ones = u.info_noise;
  init.zeros = u.bpart;
  init.nzeros = (long long)p.bslots * p.NCA * kPB + p.DPA / 2 + 1;  // (+ the row maxima behind the b partials: DP words, + the redo flag)
  init.info_copy = dense ? nullptr : u.info_chol;
  const int gridp = (int)std::min<long long>(64, 1 + init.nzeros / (8 * kThreads));
  // (dense: the kernel's own look at Lw's diagonal is not the answer -- status and logdet go to spare scratch words)
  hipLaunchKernelGGL(prior_diag_kernel<T>, dim3(gridp, u.G), dim3(kThreads), 0, h->stream, u.Lw, a.ldl, a.prior_kind, a.D,
                     dense ? u.spare_logdet : u.logdetLw, dense ? u.spare_info : u.info_prior, init, a.strideLw, u.wsb);
  if (dense) {
    hipLaunchKernelGGL(prior_copy_kernel<T>, dim3(1024, u.G), dim3(kThreads), 0, h->stream, u.Lw, a.ldl, a.D, p.DP, u.W, (int64_t)p.DP, a.strideLw, u.wse);
    const int rc = chol_large<T>(h, u.W, p.DP, p.DP, p.DP, u.info_prior, u.G, u.wse, u.info_stride);
    if (rc) return rc;
    hipLaunchKernelGGL(logdet_kernel<T>, dim3(u.G), dim3(kThreads), 0, h->stream, (const T*)u.W, (int64_t)p.DP, a.D, u.logdetLw, u.wsb,
                       (const int32_t*)u.info_prior, u.info_chol);
  }
  return 0;
}

// ---- column statistics (reference :82-84)
template <typename T>
void large_colstats(const LargeRun<T>& u) {
  const PosteriorArgs<T>& a = u.a;
  ColstatsArgs<T> c{};
  c.X = u.X; c.ldx = a.ldx; c.y = u.y; c.s = u.s; c.mw = u.mw; c.r = u.rvec; c.w = u.wvec; c.qpart = u.qpart; c.lpart = u.lpart;
  c.noise_info = u.info_noise;
  c.layout = a.layout; c.noise_kind = a.noise_kind; c.D = a.D; c.N = a.N;
  c.grp_X = a.strideX; c.grp_y = a.stridey; c.grp_s = a.strides; c.grp_mw = a.stridemw; c.grp_ws = u.wsb;
  c.w_sqrt = u.p.planes ? 1 : 0;
  c.mu = u.mu;
  if (u.p.rff) {
    c.X = nullptr;
    c.rff_Xin = a.rff_Xin; c.rff_ldxin = a.rff_ldxin; c.rff_Omega = a.rff_Omega; c.rff_ldo = a.rff_ldo; c.rff_phase = a.rff_phase;
    c.rff_scale = a.rff_scale; c.rff_Din = a.rff_Din;
  }
  size_t lds = (((size_t)a.D * sizeof(T) + 15) & ~(size_t)15) + 64;
  hipLaunchKernelGGL(colstats_kernel<T>, dim3(kLargeParts, u.G), dim3(kThreads), lds, u.h->stream, c);
}

// what every launch of gram_tile_kernel in the update shares: the whole lower triangle of X diag(w) X' (+ the b partials)
template <typename T>
GramTileArgs<T> large_gram_args(const LargeRun<T>& u) {
  const PosteriorArgs<T>& a = u.a;
  GramTileArgs<T> g{};
  g.X = u.X; g.ldx = a.ldx; g.layout = a.layout;
  g.use_dma = u.p.x_ring ? (u.h->opt.no_gram_ring ? 2 : 1) : 0;  // (NO_GRAM_RING: A/B experiments only)
  g.bf3 = u.p.bf3 ? 1 : 0;  // (f32 + the LDS-DMA ring only: the bf16 x 3 code lives in the ring loop)
  g.s = u.s; g.noise_kind = a.noise_kind; g.r = u.rvec; g.wpre = u.wvec;
  g.D = a.D; g.n_begin = 0; g.n_end = a.N; g.nblocks = u.p.NC; g.bpart = u.bpart; g.mode_out = 0;
  g.grp_X = a.strideX; g.grp_s = a.strides; g.grp_ws = u.wsb;
  g.tile_i0 = 0; g.tile_j0 = 0; g.tri = 1;
  return g;
}
// The prior factor as pseudo-observations: one more partial per tile behind the nsplit data partials, from the f32 tile kernel on
// either Gram route.  (r == NULL: the launch writes no b partial, so bpart only has to be a valid pointer; the plain instantiation
// is chosen by its template argument, GramTileArgs::bf3 is read by nobody.)
template <typename T>
void large_prior_pseudo_split(const LargeRun<T>& u) {
  const LargePlan& p = u.p;
  GramTileArgs<T> g = large_gram_args(u);
  g.nsplit = 1; g.ntiles = p.ntiles; g.nsplit_diag = 0; g.nlong = 0;
  g.xcd_swizzle = 0;
  g.X = u.Lw; g.ldx = u.a.ldl; g.layout = 2; g.use_dma = 0; g.bf3 = 0; g.s = nullptr; g.r = nullptr; g.wpre = nullptr;
  g.grp_X = u.a.strideLw; g.grp_s = 0;
  g.n_begin = 0; g.n_end = u.a.D;
  g.Gpart = u.Gpart + (int64_t)p.nsplit * p.ntiles * kPB * kPB;
  hipLaunchKernelGGL(gram_tile_kernel<T>, dim3(p.ntiles, u.G), dim3(kThreads), LargeCfg<T>::LDS_BYTES, u.h->stream, g);
}

// ---- Gram (reference :86) by tiles: split-K partial tiles, then the prior factor as pseudo-observations
template <typename T>
void large_gram_tiles(const LargeRun<T>& u) {
  using LC = LargeCfg<T>;
  const LargePlan& p = u.p;
  GramTileArgs<T> g = large_gram_args(u);
  g.nsplit = p.nsplit; g.ntiles = p.ntiles; g.Gpart = u.Gpart;
  g.nsplit_diag = p.nsplit_diag; g.nlong = p.nlong;
  g.xcd_swizzle = (p.nsplit > 1 && !u.h->opt.no_xcd_swizzle) ? (p.nlong == 0 ? 1 : 2) : 0;  // (three kinds of work items: remapped inside a kind, the dispatch order of the kinds IS the plan)
  const int nwg = p.nsplit_diag ? (p.ntiles - p.NC) * p.nsplit - p.nlong + p.NC * p.nsplit_diag : p.ntiles * p.nsplit;
  if constexpr (sizeof(T) == 4) {
    if (g.bf3) hipLaunchKernelGGL((gram_tile_kernel<T, true>), dim3(nwg, u.G), dim3(kThreads), LC::LDS_BYTES, u.h->stream, g);
    else hipLaunchKernelGGL(gram_tile_kernel<T>, dim3(nwg, u.G), dim3(kThreads), LC::LDS_BYTES, u.h->stream, g);
  } else {
    hipLaunchKernelGGL(gram_tile_kernel<T>, dim3(nwg, u.G), dim3(kThreads), LC::LDS_BYTES, u.h->stream, g);
  }
  if (u.a.prior_kind == PRIOR_UPPER_FACTOR) large_prior_pseudo_split(u);
}

// ---- Gram by planes (fp32): the rows' largest entries, the operand planes (with the b partials), the Gram launch on them, then the
// prior factor as pseudo-observations
inline int large_gram_planes(const LargeRun<float>& u) {
  blr_handle* const h = u.h;
  const PosteriorArgs<float>& a = u.a;
  const LargePlan& p = u.p;
  const int G = u.G, NC = p.NC, NCA = p.NCA, nbchunks = p.nbchunks;
  const bool rff = p.rff;
  int rc;
  if ((rc = set_lds_once(h, gram_planes_kernel<2>, (size_t)PlanesCfg<2>::LDS))) return rc;
  if ((rc = set_lds_once(h, gram_planes_kernel<3>, (size_t)PlanesCfg<3>::LDS))) return rc;
  PlanesArgs pa{};
  pa.X = rff ? nullptr : u.X; pa.ldx = a.ldx;
  pa.Xin = a.rff_Xin; pa.ldxin = a.rff_ldxin; pa.Omega = a.rff_Omega; pa.ldo = a.rff_ldo; pa.phase = a.rff_phase; pa.scale = a.rff_scale; pa.Din = a.rff_Din;
  pa.wsq = u.wvec; pa.r = u.rvec; pa.Xp = u.Xp; pa.bpart = u.bpart; pa.rowmax = u.rowmax;
  pa.D = a.D; pa.N = a.N; pa.NC = NCA; pa.NKB = p.NKB; pa.nchunks = nbchunks;
  pa.grp_X = a.strideX; pa.grp_ws = u.wsb;
  if (u.ms) {
    pa.Y = static_cast<const float*>(u.ms->Y); pa.ldY = u.ms->ldY; pa.S = u.ms->S;
    pa.mu = u.mu; pa.qsp = u.qsp;
  }
  // a basis of up to 8 input dimensions: the raw inputs of a workgroup's whole column chunk are staged once (blr_planes.hpp, xs_chunk)
  pa.xs_chunk = (rff && a.rff_Din <= 8) ? 1 : 0;
  const size_t plds = planes_pass_lds(rff, pa.xs_chunk != 0, a.rff_Din);
  if (p.NP == 2) {  // the rows' power-of-two scales need (a bound of) the rows' largest entries first
    if (rff) {  // a basis: its bound
      hipLaunchKernelGGL(rowmax_kernel<true>, dim3(nbchunks, 1, G), dim3(kThreads), 0, h->stream, pa);
      hipLaunchKernelGGL((planes_kernel<2, true>), dim3(nbchunks, NC, G), dim3(kThreads), plds, h->stream, pa);
    } else if (h->opt.no_spec_rowmax) {  // the exact maxima: one more pass over X
      hipLaunchKernelGGL(rowmax_kernel<false>, dim3(nbchunks, NCA, G), dim3(kThreads), 0, h->stream, pa);
      hipLaunchKernelGGL((planes_kernel<2, false>), dim3(nbchunks, NCA, G), dim3(kThreads), plds, h->stream, pa);
    } else {
      // sampled maxima with head-room, the planes pass checks that every entry fits; the exact pass + the planes again only if one
      // did not (two launches that return at once otherwise: ~ 5 us against the 58 us of the exact pass at config 3)
      if ((rc = ensure_stats(h))) return rc;
      pa.redo = u.rowmax + p.DPA;
      pa.redo_total = h->stats_dev + 1;
      pa.sample_kb = 2;
      hipLaunchKernelGGL(rowmax_kernel<false>, dim3(nbchunks, NCA, G), dim3(kThreads), 0, h->stream, pa);
      hipLaunchKernelGGL((planes_kernel<2, false>), dim3(nbchunks, NCA, G), dim3(kThreads), plds, h->stream, pa);
      pa.sample_kb = 0;
      pa.redo_pass = 1;
      hipLaunchKernelGGL(rowmax_kernel<false>, dim3(nbchunks, NCA, G), dim3(kThreads), 0, h->stream, pa);
      hipLaunchKernelGGL((planes_kernel<2, false>), dim3(nbchunks, NCA, G), dim3(kThreads), plds, h->stream, pa);
    }
  } else {
    if (rff) hipLaunchKernelGGL((planes_kernel<3, true>), dim3(nbchunks, NC, G), dim3(kThreads), plds, h->stream, pa);
    else hipLaunchKernelGGL((planes_kernel<3, false>), dim3(nbchunks, NC, G), dim3(kThreads), plds, h->stream, pa);
  }
  HIP_TRY(h, hipGetLastError());  // (a failed planes launch leaves the last call's planes in the workspace: never a posterior from them)
  GramPlanesArgs ga{};
  ga.Xp = u.Xp; ga.NC = NCA; ga.NKB = p.NKB; ga.Gpart = u.Gpart; ga.ntiles = p.ntiles_g; ga.nsplit = p.nsplit;
  ga.s_iso = a.noise_kind == NOISE_DIAGONAL ? nullptr : u.s;
  ga.rowmax = u.rowmax;
  ga.xcd_swizzle = (p.nsplit > 1 && !h->opt.no_xcd_swizzle) ? 1 : 0;
  ga.grp_ws = u.wsb; ga.grp_s = a.strides;
  ga.ll = (p.NP == 2 && (int64_t)a.N < (int64_t)kPlanesLlFactor * p.DP) ? 1 : 0;
  const dim3 grid(p.ntiles_g * p.nsplit, G);
  if (p.planes4) {
    if ((rc = set_lds_once(h, gram_planes4_kernel, (size_t)Planes4Cfg::LDS))) return rc;
    hipLaunchKernelGGL(gram_planes4_kernel, grid, dim3(kThreads), (size_t)Planes4Cfg::LDS, h->stream, ga);
  } else if (p.NP == 2) hipLaunchKernelGGL(gram_planes_kernel<2>, grid, dim3(kPlanesThreads), (size_t)PlanesCfg<2>::LDS, h->stream, ga);
  else hipLaunchKernelGGL(gram_planes_kernel<3>, grid, dim3(kPlanesThreads), (size_t)PlanesCfg<3>::LDS, h->stream, ga);
  if (a.prior_kind == PRIOR_UPPER_FACTOR) large_prior_pseudo_split(u);  // (one more partial per tile, from the f32 kernel)
  return 0;
}

// ---- reduction of the partial tiles and b partials into Abar = [A; b'] (+ the prior; Lw_post for the caller)
template <typename T>
void large_reduce(const LargeRun<T>& u) {
  const PosteriorArgs<T>& a = u.a;
  const LargePlan& p = u.p;
  const int pf = a.prior_kind == PRIOR_UPPER_FACTOR ? 1 : 0;
  ReduceArgs<T> r{};
  r.bpart = u.bpart;
  r.Lw = u.Lw; r.ldl = a.ldl; r.prior_kind = a.prior_kind; r.D = a.D; r.DP = p.DP; r.Abar = u.Abar; r.lda = p.lda;
  r.Lw_post = a.Lw_post ? a.Lw_post + u.reg0 * a.strideLp : nullptr; r.ldlp = a.ldlp;
  r.grp_Lw = a.strideLw; r.grp_Lp = a.strideLp; r.grp_ws = u.wsb;
  // (planes path: the planes pass's b partials, one per column chunk, at stride NCA; multi-output: the residuals' row block is block NC)
  r.nsplit_b = p.nbchunks;
  r.nblocks = p.NCA;
  r.multi_block = u.ms ? p.NC : 0;
  r.Gpart = u.Gpart; r.nsplit_total = p.nsplit + pf; r.ntiles = p.ntiles_g;
  r.nsplit_diag = p.nsplit_diag; r.pseudo_split = pf; r.nlong = p.nlong;
  hipLaunchKernelGGL(gram_reduce_kernel<T>, dim3(p.ntiles_g + p.NC, 16, u.G), dim3(kThreads), 0, u.h->stream, r);
}

// ---- blocked Cholesky of Abar (rows DP.. = rhs) -> L, u  (reference :86, :57)
// (only the first 64 of the 128 padding rows ride along: row DP is b', the others are zero and nobody reads them back --
// half the right-hand-side sub-tiles of every trailing update, and c5's first trailing updates fit one round)
// (multi-output: rows DP + s are b_s' for the columns s < S of Y; more than 64 of them take all 128 rows along)
template <typename T>
int large_factor(const LargeRun<T>& u) {
  const LargePlan& p = u.p;
  blr_handle::MultiSrc* const ms = u.ms;
  const int rc = chol_large<T>(u.h, u.Abar, p.lda, p.DP, p.DP + ((ms && ms->S > TrailCfg<T>::SB) ? kPB : TrailCfg<T>::SB), u.info_chol, u.G,
                               u.wse, u.info_stride);
  if (rc) return rc;
  if (ms) {
    ms->Abar = u.Abar; ms->lda = p.lda; ms->Tfull = u.Tfull; ms->DP = p.DP;
    ms->qsp = u.qsp; ms->nq = p.nbchunks; ms->done = true;
  }
  return 0;
}

// ---- T = L' (for the caller and for the AXPY-form back substitution), then m, posterior mean, evidence: one launch each
// over the group (blockIdx.z / WaveSolveArgs::group)
template <typename T>
int large_solve(const LargeRun<T>& u) {
  const PosteriorArgs<T>& a = u.a;
  const LargePlan& p = u.p;
  const int G = u.G, DP = p.DP;
  // logpdf alone (no posterior mean, no factor wanted): the evidence is complete with the factorisation -- no transpose, no
  // back substitution, the launch below only assembles the scalars
  const bool evidence_only = a.mw_post == nullptr && a.T_post == nullptr;
  if (!evidence_only) {
    dim3 grid((DP + 31) / 32, (DP + 31) / 32, G);
    hipLaunchKernelGGL(transpose_out_kernel<T>, grid, dim3(kThreads), 0, u.h->stream, (const T*)u.Abar, p.lda, DP, u.Tfull,
                       (int64_t)DP, a.T_post ? a.T_post + u.reg0 * a.strideT : (T*)nullptr, a.ldt, a.D, u.wse, a.strideT,
                       (const int32_t*)u.info_prior, (const unsigned*)u.info_noise, (const int32_t*)u.info_chol, u.wsb);
  }
  WaveSolveArgs<T> b{};
  b.Tf = u.Tfull; b.ldtf = DP; b.D = a.D; b.DP = DP;
  if (evidence_only) { b.Tf = u.Abar; b.ldtf = p.lda; b.evidence_only = 1; }  // (diagonal of L = diagonal of T)
  b.rhs = u.Abar + DP; b.ldrhs = G > 1 ? u.wse : 0; b.rhs_inc = p.lda;  // u = row DP of the factored Abar
  b.add = u.mw; b.out = a.mw_post ? a.mw_post + u.reg0 * a.stride_mwpost : nullptr;
  b.ldout = G > 1 ? a.stride_mwpost : 0;
  b.qpart = u.qpart; b.lpart = u.lpart; b.nparts = kLargeParts;
  b.logdet_Lw_dev = u.logdetLw;
  b.noise_kind = a.noise_kind; b.s = u.s; b.N = a.N;
  b.logpdf = a.logpdf ? a.logpdf + u.reg0 : nullptr; b.info = a.info + u.reg0;
  b.chol_info = u.info_chol;
  b.prior_info = u.info_prior; b.noise_info = u.info_noise;
  if (G > 1) { b.group = G; b.ws_stride = u.wsb; b.add_stride = a.stridemw; b.s_stride = a.strides; }
  return launch_wave_solve<T>(u.h, b, p.NC, G);
}

// `G` regressors reg0 .. reg0 + G - 1 of the batch, each with its own copy of the workspace, in every launch of the update
// (regressor from blockIdx.y / .z): the ~2 dispatches per panel of the factorisation are latency, not throughput, and so are
// the small kernels around the Gram launch.  G = 1 is the single-regressor path.  *G_done: the regressors that ran (the
// workspace bound or a full device may make the group smaller).
template <typename T>
int posterior_large_group(blr_handle* h, const PosteriorArgs<T>& a, int64_t reg0, int G, int* G_done = nullptr) {
  const LargeShape shape{(int)sizeof(T), a.D, a.N, a.layout, a.noise_kind, a.prior_kind, aligned16(a.X + reg0 * a.strideX, a.ldx, (int64_t)0),
                         a.rff_Omega != nullptr, a.rff_Din, h->multi_src ? h->multi_src->S : 0, G};
  LargePlan p;
  const char* const refused = plan_large(shape, h->opt, h->cus, large_ws_cap(h->opt), h->gram_plans, p);
  if (p.route) { h->route_i8_B = 0; h->route = p.route; }
  if (refused) return hip_fail(h, hipErrorInvalidValue, refused);
  G = p.G;
  int rc;
  for (;;) {  // (a device too full for the whole group's workspace: smaller groups, down to one regressor at a time)
    rc = h->ws.reserve(h, p.o.per * (size_t)G, blr_handle::kWsFloor);
    if (rc == 0 || G == 1) break;
    (void)hipGetLastError();
    h->err.clear();
    G = (G + 1) / 2;
  }
  if (rc) return rc;
  if (G_done) *G_done = G;
  const LargeRun<T> u = bind_large<T>(h, a, p, reg0, G);

  if ((rc = large_prior(u))) return rc;
  large_colstats(u);
  if ((rc = set_lds_once(h, gram_tile_kernel<T>, (size_t)LargeCfg<T>::LDS_BYTES))) return rc;
  if constexpr (sizeof(T) == 4) {
    if ((rc = set_lds_once(h, gram_tile_kernel<T, true>, (size_t)LargeCfg<T>::LDS_BYTES))) return rc;
    if (p.planes) { if ((rc = large_gram_planes(u))) return rc; }
    else large_gram_tiles(u);
  } else {
    large_gram_tiles(u);
  }
  large_reduce(u);
  if ((rc = large_factor(u))) return rc;
  if ((rc = large_solve(u))) return rc;
  HIP_TRY(h, hipGetLastError());
  return 0;
}

template <typename T>
int dispatch_posterior(blr_handle* h, const PosteriorArgs<T>& a) {
  if (a.D <= kMaxSmallD) return dispatch_fused_small<T>(h, a);
  // regressors of a batch go through the blocked factorisation in groups (posterior_large_group); the regressors of a group
  // must see the same alignment of X (one split / staging decision per group)
  // (the more the better wherever measured -- D = 256 .. 4096, groups of up to 128, tools/chain_batch_scan.sh -- so the bound is
  // the workspace: kChainWorkspace)
  int gmax = kChainBatchMax;
  if (h->opt.chain_batch > 0) gmax = std::min(kChainBatchMax, h->opt.chain_batch);  // measurements only
  if ((a.strideX * (int64_t)sizeof(T)) % 16 != 0) gmax = 1;
  {  // even groups: 129 regressors run as 65 + 64, not 128 + 1
    const int64_t ngroups = std::max<int64_t>(1, (a.B + gmax - 1) / gmax);
    gmax = (int)((a.B + ngroups - 1) / ngroups);
  }
  for (int64_t reg = 0; reg < a.B;) {
    int done = 1;
    int rc = posterior_large_group<T>(h, a, reg, (int)std::min<int64_t>(gmax, a.B - reg), &done);
    if (rc) return rc;
    reg += done;
  }
  return 0;
}

// The argument checks of blr_posterior_batched_* (the positions are the documented ABI).  1: nothing to do (B == 0)
template <typename T>
int posterior_check(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X,
                      int64_t ldx, int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s,
                      int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw, int64_t ldl,
                      int64_t strideLw, T* mw_post, int64_t stride_mwpost, T* T_post, int64_t ldt, int64_t strideT,
                      T* Lw_post, int64_t ldlp, int64_t strideLp, double* logpdf, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1) return bad_arg(h, 5, "D < 1");
  if (D > kMaxLargeD) return bad_arg(h, 5, "D > 8192 is not supported by this build");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range");
  if (B == 0) return 1;
  if (N > 0 && !X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(N, 1)) return bad_arg(h, 8, "ldx too small");
  if (strideX < 0) return bad_arg(h, 9, "strideX < 0");
  if (N > 0 && !y) return bad_arg(h, 10, "y is NULL (reference :74 length check)");
  if (stridey < 0) return bad_arg(h, 11, "stridey < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 12, "noise_kind (dense Sigma_y is outside the GPU scope)");
  if (!s) return bad_arg(h, 13, "s is NULL");
  if (strides < 0) return bad_arg(h, 14, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 15, "prior_kind");
  if (!mw) return bad_arg(h, 16, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 17, "stridemw < 0");
  if (!Lw) return bad_arg(h, 18, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 19, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 20, "strideLw < 0");
  if (mw_post && B > 1 && stride_mwpost < D) return bad_arg(h, 22, "stride_mwpost < D");
  if (T_post && ldt < D) return bad_arg(h, 24, "ldt < D");
  if (T_post && B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 25, "strideT too small");
  if (Lw_post && ldlp < D) return bad_arg(h, 27, "ldlp < D");
  if (Lw_post && B > 1 && strideLp < (int64_t)mat_extent(D, D, ldlp)) return bad_arg(h, 28, "strideLp too small");
  if (!info) return bad_arg(h, 30, "info is NULL");
  return 0;
}

// The update on device pointers: `a` carries them with every dimension, leading dimension and stride (and the rff_* fields of a
// basis that the planes pass evaluates itself)
template <typename T>
int posterior_run(blr_handle* h, PosteriorArgs<T>& a) {
  a.vec_ok = (a.layout == BLR_LAYOUT_COLVECS && a.D % Mfma<T>::VEC == 0 && aligned16(a.X, a.ldx, a.strideX)) ? 1 : 0;
  if (a.N == 0) {  // no data: the kernel never dereferences X / y, but keep the pointers valid
    if (!a.X) a.X = a.mw;
    if (!a.y) a.y = a.mw;
  }
  return dispatch_posterior<T>(h, a);
}

template <typename T>
int posterior_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X,
                      int64_t ldx, int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s,
                      int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw, int64_t ldl,
                      int64_t strideLw, T* mw_post, int64_t stride_mwpost, T* T_post, int64_t ldt, int64_t strideT,
                      T* Lw_post, int64_t ldlp, int64_t strideLp, double* logpdf, int32_t* info) {
  int rc = posterior_check<T>(h, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides, prior_kind, mw, stridemw, Lw,
                              ldl, strideLw, mw_post, stride_mwpost, T_post, ldt, strideT, Lw_post, ldlp, strideLp, logpdf, info);
  if (rc) return rc < 0 ? rc : 0;
  HIP_TRY(h, hipSetDevice(h->device));
  PosteriorArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.stridey = stridey; a.strides = strides; a.stridemw = stridemw;
  a.ldl = ldl; a.strideLw = strideLw; a.stride_mwpost = stride_mwpost; a.ldt = ldt; a.strideT = strideT;
  a.ldlp = ldlp; a.strideLp = strideLp;
  a.layout = layout; a.noise_kind = noise_kind; a.prior_kind = prior_kind;
  a.D = (int)D; a.N = (int)N; a.B = (int)B;

  CallIO io(h, memspace);
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  const size_t s_one = noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1;
  if ((rc = io.in(X, extent(B, strideX, x_one), &a.X))) return rc;
  if ((rc = io.in(y, extent(B, stridey, (size_t)N), &a.y))) return rc;
  if ((rc = io.in(s, extent(B, strides, s_one), &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &a.Lw))) return rc;
  if ((rc = io.out(mw_post, extent(B, stride_mwpost, (size_t)D), &a.mw_post))) return rc;
  if ((rc = io.out(T_post, extent(B, strideT, mat_extent(D, D, ldt)), &a.T_post))) return rc;
  if ((rc = io.out(Lw_post, extent(B, strideLp, mat_extent(D, D, ldlp)), &a.Lw_post))) return rc;
  if ((rc = io.out(logpdf, (size_t)B, &a.logpdf))) return rc;
  if ((rc = io.out(info, (size_t)B, &a.info))) return rc;
  if ((rc = posterior_run<T>(h, a))) return rc;
  return io.finish();
}

template <typename T>
int posterior_single(blr_handle* h, int layout, int64_t D, int64_t N, const T* X, int64_t ldx, const T* y,
                     int noise_kind, const T* s, int prior_kind, const T* mw, const T* Lw, int64_t ldl, T* mw_post,
                     T* T_post, int64_t ldt, T* Lw_post, int64_t ldlp, double* logpdf) {
  int32_t info = 0;
  int rc = posterior_batched<T>(h, BLR_MEM_HOST, layout, 1, D, N, X, ldx, 0, y, 0, noise_kind, s, 0, prior_kind, mw, 0,
                                Lw, ldl, 0, mw_post, D, T_post, ldt, ldt * D, Lw_post, ldlp, ldlp * D, logpdf, &info);
  if (rc) {
    // re-number argument positions of the batched form onto the single form
    static const int map[31] = {0, 1, 0, 2, 0, 3, 4, 5, 6, 0, 7, 0, 8, 9, 0, 10, 11, 0, 12, 13, 0,
                                14, 0, 15, 16, 0, 17, 18, 0, 19, 0};
    if (rc < 0 && rc > -31 && map[-rc]) return -map[-rc];
    return rc;
  }
  return info;
}

// ---- factor of the prior precision for marginals / draws ----------------------------------------------
// Returns a device pointer to U (upper factor, ld = D, stride D*D) or to d (diagonal) per regressor.
template <typename T>
int prior_factor(blr_handle* h, int64_t B, int64_t D, int prior_kind, const T* Lw_dev, int64_t ldl, int64_t strideLw,
                 const T** U, int64_t* ldu, int64_t* strideU, int* kind_out, int32_t** info_dev) {
  *info_dev = nullptr;
  if (prior_kind != BLR_PRIOR_DENSE) {
    *U = Lw_dev; *ldu = ldl; *strideU = strideLw; *kind_out = prior_kind;
    return 0;
  }
  size_t need = (size_t)B * D * D * sizeof(T) + (size_t)B * sizeof(int32_t) + 64;
  int rc = h->ws.reserve(h, need, blr_handle::kWsFloor);
  if (rc) return rc;
  T* Uw = reinterpret_cast<T*>(h->ws.p);
  int32_t* inf = reinterpret_cast<int32_t*>(h->ws.p + (((size_t)B * D * D * sizeof(T) + 15) & ~(size_t)15));
  size_t lds = ((size_t)D * (D + 1) / 2 + D) * sizeof(T) + 16;
  auto kern = chol_small_kernel<T>;
  if (const int rc_lds = set_lds_once(h, kern, (size_t)((int)lds))) return rc_lds;
  hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(B, 1 << 20)), dim3(kThreads), lds, h->stream, Lw_dev, ldl,
                     strideLw, Uw, D, D * D, inf, (int)D, (int)B);
  HIP_TRY(h, hipGetLastError());
  *U = Uw; *ldu = D; *strideU = D * D; *kind_out = BLR_PRIOR_UPPER_FACTOR; *info_dev = inf;
  return 0;
}


// ---- large-D marginals with a factor or a dense prior: block forward substitution on LDS-resident tiles of 32 inputs ---------------
// (marg_blocksub_kernel: X is read once, nothing but the outputs is written).  A whole batch per launch (blockIdx.y = regressor;
// a dense prior's blocked Cholesky takes the batch through chol_large's groups).  Needs the tile in LDS (D <= 1152 in fp32, 512
// in fp64: the tile is DP = 128 ceil(D / 128) wide, and DP = 640 takes 172 032 bytes in fp64) and 16-byte loads along d from X and U.  Returns 1 when the call does not qualify (the caller takes the tall-matrix route).
template <typename T>
int marginals_large_group(blr_handle* h, int layout, int64_t B, int64_t D, int64_t N, const T* X, int64_t ldx, int64_t strideX,
                          int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw,
                          int64_t ldl, int64_t strideLw, T* mean, int64_t stridemean, T* var, int64_t stridevar, int32_t* info_dev) {
  using MB = MargBlockCfg<T>;
  using MG = MargGemmCfg<T>;
  constexpr int VEC = Mfma<T>::VEC;
  const int DP = (int)((D + kPB - 1) / kPB * kPB), NC = DP / kPB;
  const bool u_given = prior_kind == BLR_PRIOR_UPPER_FACTOR;
  auto vec_ok = [&](const T* p, int64_t ld, int64_t stride) {
    return ld % VEC == 0 && ((uintptr_t)p % 16) == 0 && (B == 1 || (stride * (int64_t)sizeof(T)) % 16 == 0);
  };
  if (!var || prior_kind == BLR_PRIOR_DIAGONAL || h->opt.no_marg_gemm || layout != BLR_LAYOUT_COLVECS || D % 16 != 0 || N < 1 ||
      MB::lds_bytes(DP) > MB::kMaxLds || !vec_ok(X, ldx, strideX) || (u_given && !vec_ok(Lw, ldl, strideLw)))
    return 1;
  int rc;
  if ((rc = set_lds_once(h, marg_image_kernel<T>, (size_t)TrsmCfg<T>::LDS_BYTES))) return rc;
  // Tile height: 32 inputs on eight waves, one workgroup per CU -- or, when such tiles leave CUs idle (short N), 16 inputs on four
  // waves, two workgroups per CU (twice the factor traffic per input: 1.02 against 0.77 ms at D = 1024, N = 65536, but 0.081
  // against 0.104 ms at N = 999; fp32 only: the fp64 instance does not fit the registers of two workgroups per CU)
  using MB16 = MargBlockCfg<T, 16>;
  const bool small_tiles = sizeof(T) == 4 && ((N + MB::RT - 1) / MB::RT) * B < h->cus;
  if ((rc = set_lds_once(h, marg_blocksub_kernel<T, 32>, (size_t)MB::kMaxLds))) return rc;
  if constexpr (sizeof(T) == 4) {
    if (small_tiles && (rc = set_lds_once(h, marg_blocksub_kernel<T, 16>, (size_t)MB16::lds_bytes(DP)))) return rc;
  }
  // regressors per launch: grid.y, the images (36 / 72 KB per diagonal block) within 256 MiB, a dense prior's two D x D copies
  // within 1 GiB and chol_large's group size
  const size_t mat = (((size_t)DP * DP * sizeof(T)) + 255) & ~(size_t)255;
  int64_t chunk = std::min<int64_t>(B, std::min<int64_t>(65535, ((int64_t)256 << 20) / ((int64_t)NC * MG::IMG_ELEMS * (int64_t)sizeof(T))));
  if (!u_given) chunk = std::min<int64_t>(chunk, std::min<int64_t>(kChainBatchMax, std::max<int64_t>(1, ((int64_t)1 << 30) / (int64_t)(2 * mat))));
  chunk = h->cap_chunk(chunk);
  h->count_chunks(B, chunk);
  if ((rc = h->aux.reserve(h, (size_t)chunk * NC * MG::IMG_ELEMS * sizeof(T)))) return rc;
  if (!u_given && (rc = h->ws.reserve(h, (size_t)chunk * 2 * mat + 256, blr_handle::kWsFloor))) return rc;
  T* const img = reinterpret_cast<T*>(h->aux.p);
  HIP_TRY(h, hipMemsetAsync(info_dev, 0, (size_t)B * sizeof(int32_t), h->stream));
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int nb = (int)std::min<int64_t>(chunk, B - b0);
    const T* U = Lw + b0 * strideLw;
    int64_t ldu = ldl, strideU = strideLw;
    int32_t* const inf = info_dev + b0;
    if (u_given) {  // a factor with a non-positive diagonal entry is not a Cholesky factor: LAPACK-style index
      hipLaunchKernelGGL(prior_diag_kernel<T>, dim3(1, nb), dim3(kThreads), 0, h->stream, U, ldl, (int)PRIOR_UPPER_FACTOR, (int)D,
                         (double*)nullptr, inf, ScratchInit(), strideLw, (int64_t)sizeof(int32_t));
    } else {  // dense precision: L = chol(Lw) (reference :41), then U = L' with the contraction index contiguous
      T* Lf = reinterpret_cast<T*>(h->ws.p);
      T* Ut = reinterpret_cast<T*>(h->ws.p + (size_t)chunk * mat);
      const int64_t mstride = (int64_t)(mat / sizeof(T));
      hipLaunchKernelGGL(prior_copy_kernel<T>, dim3(256, nb), dim3(kThreads), 0, h->stream, Lw + b0 * strideLw, ldl, (int)D, DP, Lf, (int64_t)DP,
                         strideLw, mstride);
      if ((rc = chol_large<T>(h, Lf, DP, DP, DP, inf, nb, mstride, 1))) return rc;  // (status words: one int32 apart)
      dim3 tg((DP + 31) / 32, (DP + 31) / 32, nb);
      hipLaunchKernelGGL(transpose_out_kernel<T>, tg, dim3(kThreads), 0, h->stream, (const T*)Lf, (int64_t)DP, DP, Ut, (int64_t)DP,
                         (T*)nullptr, (int64_t)0, 0, mstride);
      U = Ut;
      ldu = DP;
      strideU = mstride;
    }
    const int Df = u_given ? (int)D : DP;  // order of the factor the kernels see (a dense prior's is padded with a unit diagonal)
    hipLaunchKernelGGL(marg_image_kernel<T>, dim3((unsigned)(NC * nb), 2), dim3(kThreads), TrsmCfg<T>::LDS_BYTES, h->stream, U, ldu,
                       (int64_t)kPB * (ldu + 1), (int)kPB, img, (const int32_t*)inf, 0, Df, NC, strideU);
    MargBlockArgs<T> m{};
    m.X = X + b0 * strideX; m.ldx = ldx; m.U = U; m.ldu = ldu; m.img = img; m.mw = mw + b0 * stridemw; m.s = s + b0 * strides;
    m.noise_kind = noise_kind; m.mean = mean ? mean + b0 * stridemean : nullptr; m.var = var + b0 * stridevar; m.info = inf;
    m.D = Df; m.Dx = (int)D; m.DP = DP; m.N = (int)N;
    m.strideX = strideX; m.strideU = strideU; m.stridemw = stridemw; m.strides = strides; m.stridemean = stridemean; m.stridevar = stridevar;
    if constexpr (sizeof(T) == 4) {
      if (small_tiles) {
        const int64_t ntiles = (N + MB16::RT - 1) / MB16::RT;
        const int64_t gx = std::min<int64_t>(ntiles, std::max<int64_t>(1, (2 * h->cus + nb - 1) / nb));  // two workgroups per CU
        hipLaunchKernelGGL((marg_blocksub_kernel<T, 16>), dim3((unsigned)gx, (unsigned)nb), dim3(MB16::THREADS), (size_t)MB16::lds_bytes(DP),
                           h->stream, m);
        h->marg_block.launch(MB16::RT, ntiles, gx, nb);
      }
    }
    if (!small_tiles) {
      const int64_t ntiles = (N + MB::RT - 1) / MB::RT;
      const int64_t gx = std::min<int64_t>(ntiles, std::max<int64_t>(1, (h->cus + nb - 1) / nb));  // one workgroup per CU
      hipLaunchKernelGGL((marg_blocksub_kernel<T, 32>), dim3((unsigned)gx, (unsigned)nb), dim3(MB::THREADS), (size_t)MB::lds_bytes(DP),
                         h->stream, m);
      h->marg_block.launch(MB::RT, ntiles, gx, nb);
    }
  }
  HIP_TRY(h, hipGetLastError());
  return 0;
}

// ---- the tall-matrix panel sweep (kernels: blr_tall.hpp) ---------------------------------------------------------------------
// Ybar = [ F ; rows ] (column-major, ldy): `below` rows, a multiple of 128, under an already factored DP x DP block F.  One
// 128-column panel at a time every row x' becomes x'L^-T (forward) and then x'L^-T L^-1 = x'A^-1 (backward, which reads the UPPER
// triangle of F as T = L').  G matrices per launch (blockIdx.y): matrix g lies grp_ws bytes further and has status word info[g];
// 1 and 0 for a single matrix.
template <typename T>
struct TallSweep {
  using TC = TrsmCfg<T>;
  using LC = LargeCfg<T>;
  blr_handle* h;
  T* Ybar; int64_t ldy;
  int DP, below;
  const int32_t* info;
  int G; int64_t grp_ws;

  int NC() const { return DP / kPB; }
  dim3 row_blocks() const { return dim3((below + TC::RB - 1) / TC::RB, (unsigned)G); }
  int prepare() const {
    int rc;
    if ((rc = set_lds_once(h, trsm_block_kernel<T>, (size_t)TC::LDS_BYTES))) return rc;
    if ((rc = set_lds_once(h, trsm_back_block_kernel<T>, (size_t)TC::LDS_BYTES))) return rc;
    return set_lds_once(h, gram_tile_kernel<T>, (size_t)LC::LDS_BYTES);
  }
  // C(I, J) -= Y(I, p) F(J, p)' for every row block I below F and J = j0 .. j0 + ncolblocks - 1
  void trailing(int p, int j0, int ncolblocks) const {
    const int nyb = below / kPB;
    GramTileArgs<T> g{};
    g.X = Ybar + (int64_t)p * kPB * ldy; g.ldx = ldy; g.layout = LAYOUT_COLVECS; g.use_dma = 1;
    g.s = nullptr; g.noise_kind = NOISE_ISOTROPIC; g.r = nullptr;
    g.D = DP + below; g.n_begin = 0; g.n_end = kPB; g.nsplit = 1;
    g.tile_i0 = NC(); g.tile_j0 = j0; g.tri = 3; g.ntile_rows = nyb; g.ntiles = nyb * ncolblocks; g.nblocks = NC() + nyb;
    g.C = Ybar; g.ldc = ldy; g.mode_out = 1;
    g.grp_X = grp_ws / (int64_t)sizeof(T); g.grp_s = 0; g.grp_ws = grp_ws;
    hipLaunchKernelGGL(gram_tile_kernel<T>, dim3(g.ntiles, (unsigned)G), dim3(kThreads), LC::LDS_BYTES, h->stream, g);
  }
  // rows x' -> x'L^-T.  rs: the row sums of squares that ride along (block p of a row is final after panel p), without first / last
  void forward(RowSqArgs<T> rs) const {
    for (int p = 0; p < NC(); ++p) {
      rs.first = p == 0; rs.last = p == NC() - 1;
      hipLaunchKernelGGL(trsm_block_kernel<T>, row_blocks(), dim3(kThreads), TC::LDS_BYTES, h->stream, Ybar, ldy, p, DP, DP + below, info, rs,
                         grp_ws);
      if (p + 1 < NC()) trailing(p, p + 1, NC() - 1 - p);
    }
  }
  // rows x'L^-T -> x'L^-T L^-1 = x'A^-1
  void backward() const {
    for (int p = NC() - 1; p >= 0; --p) {
      hipLaunchKernelGGL(trsm_back_block_kernel<T>, row_blocks(), dim3(kThreads), TC::LDS_BYTES, h->stream, Ybar, ldy, p, DP, DP + below, info,
                         grp_ws);
      if (p > 0) trailing(p, 0, p);
    }
  }
};

// top block of a tall matrix for a factored or dense prior: L = U' (upper factor given) or chol(Lw) (dense precision, reference :41
// _cholesky(Lw)).  A factor with a non-positive diagonal entry is not a Cholesky factor: LAPACK-style index in *info_dev instead of
// Inf / NaN results with info = 0; the panel kernels return early on a non-zero status.
template <typename T>
int tall_top_block(blr_handle* h, int prior_kind, const T* Lw, int64_t ldl, int D, int DP, T* Ybar, int64_t ldy, int32_t* info_dev) {
  if (prior_kind == BLR_PRIOR_UPPER_FACTOR) {
    hipLaunchKernelGGL(prior_diag_kernel<T>, dim3(1), dim3(kThreads), 0, h->stream, Lw, ldl, (int)PRIOR_UPPER_FACTOR, D, (double*)nullptr,
                       info_dev);
    dim3 grid((DP + 31) / 32, (DP + 31) / 32);
    hipLaunchKernelGGL(factor_transpose_fill_kernel<T>, grid, dim3(kThreads), 0, h->stream, Lw, ldl, D, DP, Ybar, ldy);
    return 0;
  }
  hipLaunchKernelGGL(prior_copy_kernel<T>, dim3(1024), dim3(kThreads), 0, h->stream, Lw, ldl, D, DP, Ybar, ldy);
  return chol_large<T>(h, Ybar, ldy, DP, DP, info_dev);
}

// ---- large-D marginals: mean stream + (var) tall TRSM through the factorisation's panel machinery -------------------
template <typename T>
int marginals_large_one(blr_handle* h, int layout, int64_t D, int64_t N, const T* X, int64_t ldx, int noise_kind,
                        const T* s, int prior_kind, const T* mw, const T* Lw, int64_t ldl, T* mean, T* var,
                        int32_t* info_dev) {
  using SC = SmallCfg<T, 8>;
  const int DP = (int)((D + kPB - 1) / kPB * kPB);
  const int NP = (int)((N + kPB - 1) / kPB * kPB);
  const int64_t ldy = (int64_t)DP + NP;
  int rc;
  HIP_TRY(h, hipMemsetAsync(info_dev, 0, sizeof(int32_t), h->stream));
  const bool need_tall = var && prior_kind != BLR_PRIOR_DIAGONAL;
  T* Ybar = nullptr;
  if (need_tall) {
    const size_t bytes = (((size_t)ldy * DP * sizeof(T) + 255) & ~(size_t)255) + (size_t)NP * sizeof(double);
    if ((rc = h->ws.reserve(h, bytes + 256, blr_handle::kWsFloor))) return rc;
    Ybar = reinterpret_cast<T*>(h->ws.p);
  }
  {
    MeanFillArgs<T> m{};
    m.X = X; m.ldx = ldx; m.layout = layout; m.mw = mw; m.mean = mean; m.Ybar = Ybar; m.ldy = ldy; m.row0 = DP;
    m.D = (int)D; m.DP = DP; m.N = (int)N;
    constexpr int VEC = Mfma<T>::VEC;
    const bool stream_ok = mean && !Ybar && layout == BLR_LAYOUT_COLVECS && (D % VEC) == 0 && (ldx % VEC) == 0 &&
                           ((uintptr_t)X % 16) == 0;
    if (stream_ok) {  // mean only: a pure GEMV stream
      const size_t lds = ((size_t)D * sizeof(T) + 15) & ~(size_t)15;
      hipLaunchKernelGGL(mean_stream_kernel<T>, dim3(1024), dim3(kThreads), lds, h->stream, X, ldx, mw, mean, (int)D, (int)N);
    } else if (mean || Ybar) {
      hipLaunchKernelGGL(mean_fill_kernel<T>, dim3((unsigned)(NP / 64)), dim3(kThreads), 0, h->stream, m);
    }
  }
  if (var && prior_kind == BLR_PRIOR_DIAGONAL) {
    hipLaunchKernelGGL(var_diag_prior_kernel<T>, dim3(2048), dim3(kThreads), 0, h->stream, X, ldx, layout, Lw, (int)D, (int)N, s,
                       noise_kind, var);
  } else if (var) {
    if ((rc = tall_top_block<T>(h, prior_kind, Lw, ldl, (int)D, DP, Ybar, ldy, info_dev))) return rc;
    const TallSweep<T> sweep{h, Ybar, ldy, DP, NP, info_dev, 1, 0};
    if ((rc = sweep.prepare())) return rc;
    RowSqArgs<T> rs{};
    rs.acc = reinterpret_cast<double*>(h->ws.p + (((size_t)ldy * DP * sizeof(T) + 255) & ~(size_t)255));
    rs.var = var; rs.s = s; rs.noise_kind = noise_kind; rs.N = (int)N;
    sweep.forward(rs);
  }
  (void)sizeof(SC);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

// ---- the triangular inverses L^-T of a chunk of regressors as MFMA images (marg_image_kernel, blr_marginals.hpp) in the handle's
// side buffer: what MargProduct, marginals_multi_batched and loo_multi_batched run before their product kernels
template <typename T>
struct MargImages {
  using G = MargGemmCfg<T>;
  static constexpr int64_t kMaxChunk = ((int64_t)256 << 20) / (G::IMG_ELEMS * (int64_t)sizeof(T));  // images of a chunk within 256 MiB
  static int reserve(blr_handle* h, int64_t chunk) {
    int rc;
    if ((rc = h->aux.reserve(h, (size_t)chunk * G::IMG_ELEMS * sizeof(T)))) return rc;
    return set_lds_once(h, marg_image_kernel<T>, (size_t)TrsmCfg<T>::LDS_BYTES);
  }
  // nb regressors from reg0 on (the kernel indexes U, info and the images by reg0 + blockIdx.x): the chunk's first image lands at the
  // start of the buffer.  Returns the address the kernels index in the same way.
  static T* launch(blr_handle* h, const T* U, int64_t ldu, int64_t strideU, int D, const int32_t* info, int64_t reg0, int64_t nb) {
    T* const img = reinterpret_cast<T*>(h->aux.p) - reg0 * G::IMG_ELEMS;
    hipLaunchKernelGGL(marg_image_kernel<T>, dim3((unsigned)nb, 2), dim3(kThreads), TrsmCfg<T>::LDS_BYTES, h->stream, U, ldu, strideU, D, img, info,
                       (int)reg0);
    return img;
  }
};

// Workgroups per regressor of a kernel that walks tiles: every workgroup amortises its set-up (the image) over its tiles, about two
// workgroups per CU over the launch's nb regressors
inline int64_t tile_groups(const blr_handle* h, int64_t ntiles, int64_t nb) {
  return std::max<int64_t>(1, std::min<int64_t>(ntiles, (2 * (int64_t)h->cus + nb - 1) / nb));
}

// ---- D = 128 with a factor U (aligned ColVecs, or RowVecs): the triangular inverse once per regressor (marg_image_kernel), then a
// dependency-free product stream with the epilogue of A at the store (marginals_gemm_kernel<T, ROWV, A>, blr_marginals.hpp).
// A = MarginalArgs<T>: blr_marginals_batched_*; A = LooGemmArgs<T>: blr_loo_batched_*.  Regressors in chunks whose images fit 256 MiB.
template <typename T, typename A>
struct MargProduct {
  using G = MargGemmCfg<T>;
  static constexpr int64_t kMaxChunk = MargImages<T>::kMaxChunk;
  static bool takes(const blr_handle* h, int layout, int64_t D, int64_t N, const T* X, int64_t ldx, int64_t strideX) {
    const bool rowv = layout == BLR_LAYOUT_ROWVECS;  // (RowVecs: scalar loads, no alignment to ask for)
    return !h->opt.no_marg_gemm && D == kPB && N >= 64 &&
           (rowv || ((ldx % Mfma<T>::VEC) == 0 && ((uintptr_t)X % 16) == 0 && ((strideX * (int64_t)sizeof(T)) % 16) == 0));
  }
  static auto kernel(int layout) -> void (*)(A, const T*) {
    return layout == BLR_LAYOUT_ROWVECS ? marginals_gemm_kernel<T, true, A> : marginals_gemm_kernel<T, false, A>;
  }
  // the images of `chunk` regressors in the handle's side buffer, the two kernels' LDS limits
  static int prepare(blr_handle* h, int layout, int64_t chunk) {
    if (const int rc = MargImages<T>::reserve(h, chunk)) return rc;
    return set_lds_once(h, kernel(layout), (size_t)G::LDS_BYTES);
  }
  // regressors b0 .. b0 + nb - 1 (the kernels index regressor reg0 + blockIdx; the images of a chunk start at its first regressor)
  static void launch(blr_handle* h, A& a, const T* U, int64_t ldu, int64_t strideU, const int32_t* info, int64_t b0, int64_t nb) {
    T* const img = MargImages<T>::launch(h, U, ldu, strideU, (int)a.D, info, b0, nb);
    // two workgroups per CU, ONE round of them (tools/marg128_bench, 64 x 4096 inputs, stream kernel alone: 8 workgroups per
    // regressor 104.8 us, 16 -- two rounds -- 116.3, 32: 126.9; 256 regressors: 2 per regressor); every workgroup copies the
    // 74 KB image once: at least four tiles per wave
    const int64_t ntiles = ((int64_t)a.N + 15) / 16;
    const int64_t per_reg = tile_groups(h, (ntiles + 15) / 16, nb);
    a.reg0 = (int)b0;
    hipLaunchKernelGGL(kernel(a.layout), dim3((unsigned)per_reg, (unsigned)nb), dim3(kThreads), G::LDS_BYTES, h->stream, a, (const T*)img);
  }
};

template <typename T>
int marginals_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X, int64_t ldx,
                      int64_t strideX, int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw,
                      int64_t stridemw, const T* Lw, int64_t ldl, int64_t strideLw, T* mean, int64_t stridemean, T* var,
                      int64_t stridevar, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->marg_block = {};  // (set next to marg_blocksub_kernel's launches)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range for this build (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range");
  if (B == 0 || N == 0) return 0;
  if (!X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N) return bad_arg(h, 8, "ldx too small");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL) return bad_arg(h, 10, "noise_kind");
  if (var && !s) return bad_arg(h, 11, "s is NULL");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 13, "prior_kind");
  if (!mw) return bad_arg(h, 14, "mw is NULL");
  if (var && !Lw) return bad_arg(h, 16, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 17, "ldl < D");
  if (mean && B > 1 && stridemean < N) return bad_arg(h, 20, "stridemean < N");
  if (var && B > 1 && stridevar < N) return bad_arg(h, 22, "stridevar < N");
  if (!info) return bad_arg(h, 23, "info is NULL");
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  MarginalArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.strides = strides; a.stridemw = stridemw;
  a.stridemean = stridemean; a.stridevar = stridevar;
  a.layout = layout; a.noise_kind = noise_kind; a.D = (int)D; a.N = (int)N; a.B = (int)B;
  const T* Lw_dev = nullptr;
  int32_t* info_out_dev = nullptr;
  int rc;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  if ((rc = io.in(X, extent(B, strideX, x_one), &a.X))) return rc;
  if ((rc = io.in(s, extent(B, strides, noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1), &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &Lw_dev))) return rc;
  if ((rc = io.out(mean, extent(B, stridemean, (size_t)N), &a.mean))) return rc;
  if ((rc = io.out(var, extent(B, stridevar, (size_t)N), &a.var))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_out_dev))) return rc;
  if (D > kMaxSmallD) {  // large-D path: the whole batch on LDS-resident tiles if it qualifies, else one regressor at a time
    if (h->opt.chain_batch == 1 && B > 1) {  // measurements only (tools/group_scan.py): the same kernels, one regressor per set of launches
      rc = 0;
      for (int64_t reg = 0; rc == 0 && reg < B; ++reg)
        rc = marginals_large_group<T>(h, layout, 1, D, N, a.X + reg * strideX, ldx, strideX, noise_kind, a.s ? a.s + reg * strides : nullptr, strides,
                                      prior_kind, a.mw + reg * stridemw, stridemw, Lw_dev ? Lw_dev + reg * strideLw : nullptr, ldl, strideLw,
                                      a.mean ? a.mean + reg * stridemean : nullptr, stridemean, a.var ? a.var + reg * stridevar : nullptr, stridevar,
                                      info_out_dev + reg);
    } else {
      rc = marginals_large_group<T>(h, layout, B, D, N, a.X, ldx, strideX, noise_kind, a.s, strides, prior_kind, a.mw, stridemw, Lw_dev, ldl,
                                    strideLw, a.mean, stridemean, a.var, stridevar, info_out_dev);
    }
    if (rc < 0 || rc > 1) return rc;
    for (int64_t reg = 0; rc == 1 && reg < B; ++reg) {
      rc = marginals_large_one<T>(h, layout, D, N, a.X + reg * strideX, ldx, noise_kind, a.s ? a.s + reg * strides : nullptr,
                                  prior_kind, a.mw + reg * stridemw, Lw_dev ? Lw_dev + reg * strideLw : nullptr, ldl,
                                  a.mean ? a.mean + reg * stridemean : nullptr, a.var ? a.var + reg * stridevar : nullptr,
                                  info_out_dev + reg);
      if (rc) return rc;
      rc = 1;
    }
    return io.finish();
  }
  int32_t* chol_info = nullptr;
  int kind = prior_kind;
  if (var) {
    if ((rc = prior_factor<T>(h, B, D, prior_kind, Lw_dev, ldl, strideLw, &a.U, &a.ldu, &a.strideU, &kind, &chol_info)))
      return rc;
  } else {
    a.U = Lw_dev; a.ldu = ldl; a.strideU = strideLw;
  }
  a.prior_kind = kind;
  a.info = chol_info;
  if (chol_info) HIP_TRY(h, hipMemcpyAsync(info_out_dev, chol_info, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  else HIP_TRY(h, hipMemsetAsync(info_out_dev, 0, (size_t)B * sizeof(int32_t), h->stream));
  using MP = MargProduct<T, MarginalArgs<T>>;
  if (var && kind == BLR_PRIOR_UPPER_FACTOR && MP::takes(h, layout, D, N, a.X, ldx, strideX)) {
    const int64_t chunk = h->cap_chunk(std::min<int64_t>(std::min<int64_t>(B, 65535), MP::kMaxChunk));
    h->count_chunks(B, chunk);
    if ((rc = MP::prepare(h, layout, chunk))) return rc;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) MP::launch(h, a, a.U, a.ldu, a.strideU, a.info, b0, std::min<int64_t>(chunk, B - b0));
  } else {
    // inputs as rows of an LDS block; with a factor: Y = X'L^-T by the TRSM sweep (MFMA), fused mean / row sum of squares;
    // mean-only and diagonal-prior calls are pure streams through the same tile loop (smaller LDS image, 2 workgroups/CU)
    using TC = TrsmCfg<T>;
    auto kern = marginals_mfma_kernel<T>;
    const bool use_factor = var && kind == BLR_PRIOR_UPPER_FACTOR;
    const int xs_bytes = (TC::RB * TC::LDX * (int)sizeof(T) + 15) & ~15;
    const int lds = use_factor ? TC::LDS_BYTES + kPB * (int)sizeof(T) : xs_bytes + 2 * kPB * (int)sizeof(T) + 16;
    if (const int rc_lds = set_lds_once(h, kern, (size_t)(TC::LDS_BYTES + kPB * (int)sizeof(T)))) return rc_lds;
    // every workgroup amortises its set-up over several tiles: aim at ~2 rounds of the chip
    const int64_t ntiles = (N + TC::RB - 1) / TC::RB;
    const int64_t slots = use_factor ? 512 : 1024;
    const int64_t per_reg = std::max<int64_t>(1, std::min<int64_t>(ntiles, (slots + B - 1) / B));
    const int64_t chunk = h->cap_chunk(65535);  // grid.y <= 65535
    h->count_chunks(B, chunk);
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
      a.reg0 = (int)b0;
      dim3 grid((unsigned)per_reg, (unsigned)std::min<int64_t>(chunk, B - b0));
      hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, h->stream, a);
    }
  }
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- N-sharded single regressor: additive statistics of a column block, and the finish from their sum ----
template <typename T>
int gram_stats(blr_handle* h, int layout, int64_t D64, int64_t N64, const T* X, int64_t ldx, const T* y, int noise_kind,
               const T* s, const T* mw, T* stats, int64_t lds, double* scal) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 2, "unknown layout (reference :26-31)");
  if (D64 < 1 || D64 > kMaxLargeD) return bad_arg(h, 3, "D out of range for this build (1..8192)");
  if (N64 < 1 || N64 > (1 << 30)) return bad_arg(h, 4, "N out of range (>= 1)");
  const int D = (int)D64, N = (int)N64;
  const int DP = (D + kPB - 1) / kPB * kPB, NC = DP / kPB;
  if (!X) return bad_arg(h, 5, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N) return bad_arg(h, 6, "ldx too small");
  if (!y) return bad_arg(h, 7, "y is NULL");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL) return bad_arg(h, 8, "noise_kind");
  if (!s) return bad_arg(h, 9, "s is NULL");
  if (!mw) return bad_arg(h, 10, "mw is NULL");
  if (!stats) return bad_arg(h, 11, "stats is NULL");
  if (lds < DP + kPB) return bad_arg(h, 12, "lds < 128 ceil(D/128) + 128");
  if (!scal) return bad_arg(h, 13, "scal is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  using LC = LargeCfg<T>;
  const int ntiles = NC * (NC + 1) / 2;
  const int max_split = std::max(1, std::min(64, (N + LC::NSC - 1) / LC::NSC));
  int nsplit = 1;
  double best = 0.0;
  for (int sp = 1; sp <= max_split; ++sp) {
    const int wgs = ntiles * sp;
    const int rounds = (wgs + 511) / 512;
    const double eff = (double)wgs / (rounds * 512.0) - 0.002 * sp;
    if (eff > best) { best = eff; nsplit = sp; }
  }
  const int gridc = 1024;
  Carve carve;
  const size_t o_gp = carve((size_t)nsplit * ntiles * kPB * kPB * sizeof(T));
  const size_t o_bp = carve((size_t)nsplit * NC * kPB * sizeof(double));
  const size_t o_r = carve((size_t)N * sizeof(T));
  const size_t o_wv = carve(noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N * sizeof(T) : 0);  // 1 / s_n for the Gram launch
  const size_t o_q = carve((size_t)gridc * sizeof(double));
  const size_t o_l = carve((size_t)gridc * sizeof(double));
  int rc = h->ws.reserve(h, carve.off, blr_handle::kWsFloor);
  if (rc) return rc;
  char* ws = h->ws.p;
  T* Gpart = reinterpret_cast<T*>(ws + o_gp);
  double* bpart = reinterpret_cast<double*>(ws + o_bp);
  T* rvec = reinterpret_cast<T*>(ws + o_r);
  T* wvec = noise_kind == BLR_NOISE_DIAGONAL ? reinterpret_cast<T*>(ws + o_wv) : nullptr;
  double* qpart = reinterpret_cast<double*>(ws + o_q);
  double* lpart = reinterpret_cast<double*>(ws + o_l);
  HIP_TRY(h, hipMemsetAsync(bpart, 0, (size_t)nsplit * NC * kPB * sizeof(double), h->stream));
  {
    ColstatsArgs<T> c{};
    c.X = X; c.ldx = ldx; c.y = y; c.s = s; c.mw = mw; c.r = rvec; c.w = wvec; c.qpart = qpart; c.lpart = lpart;
    c.layout = layout; c.noise_kind = noise_kind; c.D = D; c.N = N;
    size_t ldsb = (((size_t)D * sizeof(T) + 15) & ~(size_t)15) + 64;
    hipLaunchKernelGGL(colstats_kernel<T>, dim3(gridc), dim3(kThreads), ldsb, h->stream, c);
    hipLaunchKernelGGL(stats_scalars_kernel<T>, dim3(1), dim3(kThreads), 0, h->stream, (const double*)qpart, (const double*)lpart, gridc,
                       noise_kind, s, N, scal);
  }
  if ((rc = set_lds_once(h, gram_tile_kernel<T>, (size_t)LC::LDS_BYTES))) return rc;
  {
    GramTileArgs<T> g{};
    g.X = X; g.ldx = ldx; g.layout = layout;
    g.use_dma = x_ring(layout, X, ldx) ? 1 : 0;
    g.s = s; g.noise_kind = noise_kind; g.r = rvec; g.wpre = wvec;
    g.D = D; g.n_begin = 0; g.n_end = N; g.nsplit = nsplit;
    g.tile_i0 = 0; g.tile_j0 = 0; g.tri = 1; g.ntiles = ntiles; g.nblocks = NC;
    g.Gpart = Gpart; g.bpart = bpart; g.mode_out = 0; g.xcd_swizzle = nsplit > 1 ? 1 : 0;
    hipLaunchKernelGGL(gram_tile_kernel<T>, dim3(ntiles * nsplit), dim3(kThreads), LC::LDS_BYTES, h->stream, g);
    ReduceArgs<T> r{};
    r.Gpart = Gpart; r.bpart = bpart; r.nsplit_total = nsplit; r.ntiles = ntiles; r.nblocks = NC;
    r.Lw = nullptr; r.ldl = 0; r.prior_kind = 3 /* none: the prior is added after the cross-rank sum */;
    r.D = D; r.DP = DP; r.Abar = stats; r.lda = lds; r.Lw_post = nullptr; r.ldlp = 0;
    hipLaunchKernelGGL(gram_reduce_kernel<T>, dim3(ntiles + NC, 16), dim3(kThreads), 0, h->stream, r);
  }
  HIP_TRY(h, hipGetLastError());
  if (!h->async) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

template <typename T>
int posterior_from_stats(blr_handle* h, int64_t D64, int64_t N_total, T* stats, int64_t lds, const double* scal, int prior_kind,
                         const T* mw, const T* Lw, int64_t ldl, T* mw_post, T* T_post, int64_t ldt, T* Lw_post, int64_t ldlp,
                         double* logpdf, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (D64 < 1 || D64 > kMaxLargeD) return bad_arg(h, 2, "D out of range for this build (1..8192)");
  if (N_total < 0 || N_total > ((int64_t)1 << 40)) return bad_arg(h, 3, "N_total out of range");
  const int D = (int)D64;
  const int DP = (D + kPB - 1) / kPB * kPB, NC = DP / kPB;
  if (!stats) return bad_arg(h, 4, "stats is NULL");
  if (lds < DP + kPB) return bad_arg(h, 5, "lds < 128 ceil(D/128) + 128");
  if (!scal) return bad_arg(h, 6, "scal is NULL");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 7, "prior_kind (dense or diagonal precision; pass a carried-forward factor as U'U)");
  if (!mw) return bad_arg(h, 8, "mw is NULL");
  if (!Lw) return bad_arg(h, 9, "Lw is NULL");
  if (prior_kind == BLR_PRIOR_DENSE && ldl < D) return bad_arg(h, 10, "ldl < D");
  if (T_post && ldt < D) return bad_arg(h, 13, "ldt < D");
  if (Lw_post && ldlp < D) return bad_arg(h, 15, "ldlp < D");
  if (!info) return bad_arg(h, 17, "info is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  Carve carve;
  const size_t o_w = carve(prior_kind == BLR_PRIOR_DENSE ? (size_t)DP * DP * sizeof(T) : 0);
  const size_t o_m = carve((size_t)DP * DP * sizeof(T));
  const size_t o_sc = carve(64);
  int rc = h->ws.reserve(h, carve.off, blr_handle::kWsFloor);
  if (rc) return rc;
  char* ws = h->ws.p;
  T* W = reinterpret_cast<T*>(ws + o_w);
  T* Tfull = reinterpret_cast<T*>(ws + o_m);
  double* logdetLw = reinterpret_cast<double*>(ws + o_sc + LargeScratch::logdet);
  int32_t* info_prior = reinterpret_cast<int32_t*>(ws + o_sc + LargeScratch::info_prior);
  int32_t* info_chol = reinterpret_cast<int32_t*>(ws + o_sc + LargeScratch::info_chol);
  HIP_TRY(h, hipMemsetAsync(ws + o_sc, 0, 64, h->stream));
  if (prior_kind == BLR_PRIOR_DENSE) {
    hipLaunchKernelGGL(prior_copy_kernel<T>, dim3(1024), dim3(kThreads), 0, h->stream, Lw, ldl, D, DP, W, (int64_t)DP);
    if ((rc = chol_large<T>(h, W, DP, DP, DP, info_prior))) return rc;
    hipLaunchKernelGGL(logdet_kernel<T>, dim3(1), dim3(kThreads), 0, h->stream, (const T*)W, (int64_t)DP, D, logdetLw);
  } else {
    hipLaunchKernelGGL(prior_diag_kernel<T>, dim3(1), dim3(kThreads), 0, h->stream, Lw, ldl, prior_kind, D, logdetLw, info_prior);
  }
  hipLaunchKernelGGL(stats_add_prior_kernel<T>, dim3(1024), dim3(kThreads), 0, h->stream, stats, lds, D, DP, Lw, ldl, prior_kind,
                     Lw_post, ldlp);
  HIP_TRY(h, hipMemcpyAsync(info_chol, info_prior, sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  if ((rc = chol_large<T>(h, stats, lds, DP, DP + TrailCfg<T>::SB, info_chol))) return rc;  // (the right-hand-side rows that ride along: see large_factor)
  {
    dim3 grid((DP + 31) / 32, (DP + 31) / 32);
    hipLaunchKernelGGL(transpose_out_kernel<T>, grid, dim3(kThreads), 0, h->stream, (const T*)stats, lds, DP, Tfull, (int64_t)DP,
                       T_post, ldt, D, (int64_t)0, (int64_t)0, (const int32_t*)nullptr, (const unsigned*)nullptr, (const int32_t*)info_chol,
                       (int64_t)0);  // (info_chol carries the prior's status too)
  }
  {
    WaveSolveArgs<T> b{};
    b.Tf = Tfull; b.ldtf = DP; b.D = D; b.DP = DP;
    b.rhs = stats + DP; b.ldrhs = 0; b.rhs_inc = lds;
    b.add = mw; b.out = mw_post; b.ldout = 0;
    b.qpart = scal; b.lpart = scal + 1; b.nparts = 1; b.logdet_Lw_dev = logdetLw;
    b.noise_kind = BLR_NOISE_DIAGONAL; b.s = mw /* unused */; b.N = (int)std::min<int64_t>(N_total, 0x7fffffff);
    b.logpdf = logpdf; b.info = info; b.chol_info = info_chol;
    b.n_total = (double)N_total;
    if ((rc = launch_wave_solve<T>(h, b, NC, 1))) return rc;
  }
  HIP_TRY(h, hipGetLastError());
  if (!h->async) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

// ---- gradient for D > 128: forward + backward panels over the tall matrix [F; X'; I], G regressors per launch ------------
// Regressor g of the group: caller's arrays at their element strides, the tall matrix and the per-observation vectors in ITS slice
// of the workspace (blockIdx.y of every launch; posterior_large_group's scheme).
struct GradGroupStrides {
  int64_t X, y, s, mwp, Tf, dX, dy, ds, dmw, Ai;
};
template <typename T>
size_t grad_large_ws_bytes(int64_t D, int64_t N, bool with_ainv, bool with_dmw) {
  const size_t DP = (size_t)((D + kPB - 1) / kPB * kPB), NP = (size_t)((N + kPB - 1) / kPB * kPB), DI = with_ainv ? DP : 0;
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  return al((DP + NP + DI) * DP * sizeof(T)) + al((NP + DI) * sizeof(double)) + 3 * al(NP * sizeof(T)) + al((NP + DI) * sizeof(T)) +
         al(with_dmw ? (NP / 64) * DP * sizeof(double) : 0);
}
template <typename T>
int logpdf_grad_large_group(blr_handle* h, int G, int layout, int64_t D, int64_t N, const T* X, int64_t ldx, const T* y, int noise_kind,
                            const T* s, const T* mwp, const T* Tfac, int64_t ldt, T* dX, int64_t lddx, T* dy, T* ds, T* dmw,
                            T* Ainv, int64_t ldai, int32_t* info_dev, const GradGroupStrides& gs) {
  const int DP = (int)((D + kPB - 1) / kPB * kPB);
  const int NP = (int)((N + kPB - 1) / kPB * kPB);
  const int DI = Ainv ? DP : 0;
  const int R = DP + NP + DI;
  const int64_t ldy = R;
  Carve carve;
  const size_t o_y = carve((size_t)ldy * DP * sizeof(T));
  const size_t o_sq = carve((size_t)(NP + DI) * sizeof(double));
  const size_t o_mu = carve((size_t)NP * sizeof(T));
  const size_t o_var = carve((size_t)(NP + DI) * sizeof(T));
  const size_t o_r = carve((size_t)NP * sizeof(T));
  const size_t o_w = carve((size_t)NP * sizeof(T));
  const size_t o_part = carve(dmw ? (size_t)(NP / 64) * DP * sizeof(double) : 0);
  const int64_t wsb = (int64_t)carve.off;  // one regressor's slice
  int rc = h->ws.reserve(h, carve.off * (size_t)G, blr_handle::kWsFloor);
  if (rc) return rc;
  T* Ybar = reinterpret_cast<T*>(h->ws.p + o_y);
  double* rowsq = reinterpret_cast<double*>(h->ws.p + o_sq);
  T* mu = reinterpret_cast<T*>(h->ws.p + o_mu);
  T* var = reinterpret_cast<T*>(h->ws.p + o_var);
  T* rvec = reinterpret_cast<T*>(h->ws.p + o_r);
  T* wvec = reinterpret_cast<T*>(h->ws.p + o_w);
  double* part = dmw ? reinterpret_cast<double*>(h->ws.p + o_part) : nullptr;
  const unsigned ug = (unsigned)G;

  {
    dim3 grid((DP + 31) / 32, (DP + 31) / 32, ug);
    hipLaunchKernelGGL(factor_sym_fill_kernel<T>, grid, dim3(kThreads), 0, h->stream, Tfac, ldt, (int)D, DP, Ybar, ldy, gs.Tf, wsb);
    MeanFillArgs<T> m{};
    m.X = X; m.ldx = ldx; m.layout = layout; m.mw = mwp; m.mean = mu; m.Ybar = Ybar; m.ldy = ldy; m.row0 = DP;
    m.D = (int)D; m.DP = DP; m.N = (int)N;
    m.grp_X = gs.X; m.grp_mw = gs.mwp; m.grp_ws = wsb;
    hipLaunchKernelGGL(mean_fill_kernel<T>, dim3((unsigned)(NP / 64), ug), dim3(kThreads), 0, h->stream, m);
    if (DI) hipLaunchKernelGGL(identity_rows_kernel<T>, dim3(G > 8 ? 128 : 1024, ug), dim3(kThreads), 0, h->stream, Ybar, ldy, DP + NP, DP, wsb);
  }
  const TallSweep<T> sweep{h, Ybar, ldy, DP, NP + DI, info_dev, G, wsb};
  if ((rc = sweep.prepare())) return rc;
  {
    RowSqArgs<T> rs{};
    rs.acc = rowsq; rs.var = var; rs.s = s; rs.noise_kind = noise_kind; rs.N = (int)N;
    rs.grp_ws = wsb; rs.grp_s = gs.s;
    sweep.forward(rs);
  }
  {
    GradObsGroup og{gs.y, gs.s, gs.dy, gs.ds, wsb};
    hipLaunchKernelGGL(grad_obs_kernel<T>, dim3((unsigned)((N + kThreads - 1) / kThreads), ug), dim3(kThreads), 0, h->stream, y,
                       (const T*)mu, (const T*)var, s, noise_kind, (int)N, rvec, wvec, dy, ds, og);
  }
  sweep.backward();
  if (dX || dmw) {
    GradOutArgs<T> o{};
    o.Ybar = Ybar; o.ldy = ldy; o.row0 = DP; o.X = X; o.ldx = ldx; o.layout = layout;
    o.rvec = rvec; o.wvec = wvec; o.mwp = mwp; o.dX = dX; o.lddx = lddx; o.dmw_part = part;
    o.D = (int)D; o.DP = DP; o.N = (int)N;
    o.grp_X = gs.X; o.grp_mwp = gs.mwp; o.grp_dX = gs.dX; o.grp_ws = wsb;
    hipLaunchKernelGGL(grad_out_large_kernel<T>, dim3((unsigned)(NP / 64), ug), dim3(kThreads), 0, h->stream, o);
    if (dmw)
      hipLaunchKernelGGL(grad_reduce_large_kernel<T>, dim3((unsigned)((D + kThreads - 1) / kThreads), ug), dim3(kThreads), 0, h->stream,
                         (const double*)part, NP / 64, DP, (int)D, dmw, wsb, gs.dmw);
  }
  if (Ainv)
    hipLaunchKernelGGL(ainv_copy_kernel<T>, dim3(G > 8 ? 128 : 1024, ug), dim3(kThreads), 0, h->stream, (const T*)Ybar, ldy, DP + NP, (int)D, Ainv, ldai,
                       wsb, gs.Ai);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

// ---- gradient of the log marginal likelihood (D <= 128): fused posterior, then the two-sweep gradient kernel -----------
template <typename T>
int logpdf_grad_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X, int64_t ldx,
                        int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s, int64_t strides,
                        int prior_kind, const T* mw, int64_t stridemw, const T* Lw, int64_t ldl, int64_t strideLw,
                        double* logpdf, T* dX, int64_t lddx, int64_t stridedX, T* dy, int64_t stridedy, T* ds,
                        int64_t strideds, T* dmw, int64_t stridedmw, T* mw_post, int64_t stride_mwpost, T* Ainv,
                        int64_t ldai, int64_t strideAi, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range for this build (1..8192)");
  if (N < 1 || N > (1 << 30)) return bad_arg(h, 6, "N out of range (>= 1)");
  if (B == 0) return 0;
  if (!X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N) return bad_arg(h, 8, "ldx too small");
  if (strideX < 0) return bad_arg(h, 9, "strideX < 0");
  if (!y) return bad_arg(h, 10, "y is NULL");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL) return bad_arg(h, 12, "noise_kind");
  if (!s) return bad_arg(h, 13, "s is NULL");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 15, "prior_kind");
  if (!mw) return bad_arg(h, 16, "mw is NULL");
  if (!Lw) return bad_arg(h, 18, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 19, "ldl < D");
  if (dX && (layout == BLR_LAYOUT_COLVECS ? lddx < D : lddx < N)) return bad_arg(h, 23, "lddx too small");
  if (dy && B > 1 && stridedy < N) return bad_arg(h, 26, "stridedy < N");
  if (ds && B > 1 && strideds < N) return bad_arg(h, 28, "strideds < N");
  if (dmw && B > 1 && stridedmw < D) return bad_arg(h, 30, "stridedmw < D");
  if (mw_post && B > 1 && stride_mwpost < D) return bad_arg(h, 32, "stride_mwpost < D");
  if (Ainv && ldai < D) return bad_arg(h, 34, "ldai < D");
  if (!info) return bad_arg(h, 36, "info is NULL");
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  PosteriorArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.stridey = stridey; a.strides = strides; a.stridemw = stridemw;
  a.ldl = ldl; a.strideLw = strideLw;
  a.layout = layout; a.noise_kind = noise_kind; a.prior_kind = prior_kind;
  a.D = (int)D; a.N = (int)N; a.B = (int)B;
  GradArgs<T> g{};
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t dx_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, lddx) : mat_extent(N, D, lddx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  const size_t s_one = noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1;
  int rc;
  T *dX_d = nullptr, *dy_d = nullptr, *ds_d = nullptr, *dmw_d = nullptr, *mwp_d = nullptr, *Ai_d = nullptr;
  double* lp_d = nullptr;
  int32_t* info_d = nullptr;
  if ((rc = io.in(X, extent(B, strideX, x_one), &a.X))) return rc;
  if ((rc = io.in(y, extent(B, stridey, (size_t)N), &a.y))) return rc;
  if ((rc = io.in(s, extent(B, strides, s_one), &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &a.Lw))) return rc;
  if ((rc = io.out(dX, extent(B, stridedX, dx_one), &dX_d))) return rc;
  if ((rc = io.out(dy, extent(B, stridedy, (size_t)N), &dy_d))) return rc;
  if ((rc = io.out(ds, extent(B, strideds, (size_t)N), &ds_d))) return rc;
  if ((rc = io.out(dmw, extent(B, stridedmw, (size_t)D), &dmw_d))) return rc;
  if ((rc = io.out(mw_post, extent(B, stride_mwpost, (size_t)D), &mwp_d))) return rc;
  if ((rc = io.out(Ainv, extent(B, strideAi, mat_extent(D, D, ldai)), &Ai_d))) return rc;
  if ((rc = io.out(logpdf, (size_t)B, &lp_d))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_d))) return rc;
  if (D > kMaxSmallD) {
    // large-D path: the regressors go through the update (posterior_large_group) and through the sweeps over the tall matrix in
    // groups that share every launch; factors and posterior means of a group in buffers of their own
    int gmax = kChainBatchMax;
    if (h->opt.chain_batch > 0) gmax = std::min(kChainBatchMax, h->opt.chain_batch);  // measurements only
    if ((strideX * (int64_t)sizeof(T)) % 16 != 0) gmax = 1;
    {
      size_t ws_cap = kChainWorkspace;
      if (h->opt.chain_ws_mb > 0) ws_cap = (size_t)h->opt.chain_ws_mb << 20;
      const size_t one_ws = grad_large_ws_bytes<T>(D, N, Ai_d != nullptr, dmw_d != nullptr) + (size_t)D * D * sizeof(T);
      gmax = (int)std::max<size_t>(1, std::min<size_t>((size_t)gmax, ws_cap / one_ws));
      const int64_t ngroups = std::max<int64_t>(1, (B + gmax - 1) / gmax);
      gmax = (int)((B + ngroups - 1) / ngroups);  // even groups
    }
    T* Tf = nullptr;
    T* mp = nullptr;
    if ((rc = io.tmp((size_t)gmax * D * D, &Tf))) return rc;
    if ((rc = io.tmp((size_t)gmax * D, &mp))) return rc;
    a.vec_ok = 0;
    for (int64_t reg = 0; reg < B;) {
      PosteriorArgs<T> one = a;
      // posterior_large_group indexes the batched arrays by the regressor's number: shift the outputs that are NOT batched here
      one.stride_mwpost = mwp_d ? stride_mwpost : D;
      one.mw_post = mwp_d ? mwp_d : mp - reg * one.stride_mwpost;
      one.ldt = D; one.strideT = D * D; one.T_post = Tf - reg * one.strideT;
      one.Lw_post = nullptr; one.ldlp = D; one.strideLp = 0;
      one.logpdf = lp_d; one.info = info_d;
      int done = 1;
      if ((rc = posterior_large_group<T>(h, one, reg, (int)std::min<int64_t>(gmax, B - reg), &done))) return rc;
      GradGroupStrides gs{strideX, stridey, strides, one.stride_mwpost, one.strideT, stridedX, stridedy, strideds, stridedmw, strideAi};
      if ((rc = logpdf_grad_large_group<T>(h, done, layout, D, N, a.X + reg * strideX, ldx, a.y + reg * stridey, noise_kind,
                                           a.s + reg * strides, one.mw_post + reg * one.stride_mwpost, Tf, D,
                                           dX_d ? dX_d + reg * stridedX : nullptr, lddx, dy_d ? dy_d + reg * stridedy : nullptr,
                                           ds_d ? ds_d + reg * strideds : nullptr, dmw_d ? dmw_d + reg * stridedmw : nullptr,
                                           Ai_d ? Ai_d + reg * strideAi : nullptr, ldai, info_d + reg, gs)))
        return rc;
      reg += done;
    }
    return io.finish();  // (drains the stream in either memspace: Tf / mp are temporaries of this call)
  }
  // workspace: factor T [B][D x D], posterior mean (if the caller does not want it), dmw partials
  using TC = TrsmCfg<T>;
  const int64_t ntiles = (N + TC::RB - 1) / TC::RB + (Ainv ? (D + TC::RB - 1) / TC::RB : 0);
  int64_t per_reg = std::max<int64_t>(1, std::min<int64_t>(ntiles, (512 + B - 1) / B));
  // D = 128, aligned ColVecs: both sweeps as products with the explicit triangular inverse (grad_gemm_kernel, blr_marginals.hpp):
  // one workgroup per CU, a wave per 16 inputs; A^-1 itself (if wanted) = M M' from the same images
  using GG = GradGemmCfg<T>;
  using MG = MargGemmCfg<T>;
  const bool rowv = layout == BLR_LAYOUT_ROWVECS;  // (RowVecs: scalar loads, no alignment to ask for)
  const bool gemm = !h->opt.no_grad_gemm && D == kPB && N >= 64 && B <= 65535 &&
                    (rowv || ((ldx % Mfma<T>::VEC) == 0 && ((uintptr_t)a.X % 16) == 0 && ((strideX * (int64_t)sizeof(T)) % 16) == 0)) &&
                    (size_t)B * 2 * MG::IMG_ELEMS * sizeof(T) <= ((size_t)1 << 30);
  if (gemm) per_reg = std::max<int64_t>(1, std::min<int64_t>(((N + 15) / 16 + 4 * GG::WAVES - 1) / (4 * GG::WAVES), ((int64_t)h->cus + B - 1) / B));
  Carve carve;
  const size_t o_T = carve((size_t)B * D * D * sizeof(T));
  const size_t o_mp = carve(mwp_d ? 0 : (size_t)B * D * sizeof(T));
  const size_t o_part = carve(dmw_d ? (size_t)B * per_reg * kPB * sizeof(double) : 0);
  const size_t o_img = carve(gemm ? (size_t)B * 2 * MG::IMG_ELEMS * sizeof(T) : 0);
  if ((rc = h->ws.reserve(h, carve.off, blr_handle::kWsFloor))) return rc;
  T* Tf = reinterpret_cast<T*>(h->ws.p + o_T);
  int64_t smp = stride_mwpost;
  if (!mwp_d) { mwp_d = reinterpret_cast<T*>(h->ws.p + o_mp); smp = D; }
  double* part = dmw_d ? reinterpret_cast<double*>(h->ws.p + o_part) : nullptr;

  a.mw_post = mwp_d; a.stride_mwpost = smp;
  a.T_post = Tf; a.ldt = D; a.strideT = D * D;
  a.Lw_post = nullptr; a.ldlp = D; a.strideLp = 0;
  a.logpdf = lp_d; a.info = info_d;
  a.vec_ok = (layout == BLR_LAYOUT_COLVECS && D % Mfma<T>::VEC == 0 && aligned16(a.X, ldx, strideX)) ? 1 : 0;
  if ((rc = dispatch_posterior<T>(h, a))) return rc;

  g.X = a.X; g.ldx = ldx; g.strideX = strideX; g.y = a.y; g.stridey = stridey; g.s = a.s; g.strides = strides;
  g.mwp = mwp_d; g.stridemwp = smp; g.U = Tf; g.ldu = D; g.strideU = D * D;
  g.dX = dX_d; g.lddx = lddx; g.stridedX = stridedX; g.dy = dy_d; g.stridedy = stridedy; g.ds = ds_d; g.strideds = strideds;
  g.dmw_part = part; g.Ainv = Ai_d; g.ldai = ldai; g.strideAi = strideAi; g.info = info_d;
  g.layout = layout; g.noise_kind = noise_kind; g.D = (int)D; g.N = (int)N; g.B = (int)B;
  if (gemm) {
    if ((rc = set_lds_once(h, marg_image_kernel<T>, (size_t)TC::LDS_BYTES))) return rc;
    void (*const gg_kern)(GradArgs<T>, const T*, const T*) = rowv ? grad_gemm_kernel<T, true> : grad_gemm_kernel<T, false>;
    if ((rc = set_lds_once(h, gg_kern, (size_t)GG::LDS_BYTES))) return rc;
    T* const img = reinterpret_cast<T*>(h->ws.p + o_img);
    T* const img2 = img + B * MG::IMG_ELEMS;
    hipLaunchKernelGGL(marg_image_kernel<T>, dim3((unsigned)B, 2), dim3(kThreads), TC::LDS_BYTES, h->stream, (const T*)Tf, D, D * D, (int)D, img,
                       (const int32_t*)info_d, 0, 0, 1, (int64_t)0, img2);
    g.reg0 = 0;
    hipLaunchKernelGGL(gg_kern, dim3((unsigned)per_reg, (unsigned)B), dim3(GG::THREADS), GG::LDS_BYTES, h->stream, g, (const T*)img,
                       (const T*)img2);
    if (dmw_d)
      hipLaunchKernelGGL(grad_reduce_kernel<T>, dim3((unsigned)B), dim3(kPB), 0, h->stream, (const double*)part, (int)per_reg,
                         dmw_d, stridedmw, (int)D, (const T*)mwp_d, smp, a.mw, a.Lw, GradPrior{prior_kind, ldl, strideLw, stridemw}, (const T*)Tf,
                         (const int32_t*)info_d);
  } else {
    auto kern = logpdf_grad_kernel<T>;
    const int lds = TC::LDS_BYTES + (kPB + 3 * TC::RB) * (int)sizeof(T);
    if (const int rc_lds = set_lds_once(h, kern, (size_t)(lds))) return rc_lds;
    const int64_t chunk = h->cap_chunk(65535);  // grid.y <= 65535
    h->count_chunks(B, chunk);
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
      g.reg0 = (int)b0;
      hipLaunchKernelGGL(kern, dim3((unsigned)per_reg, (unsigned)std::min<int64_t>(chunk, B - b0)), dim3(kThreads), lds, h->stream, g);
    }
    if (dmw_d)
      hipLaunchKernelGGL(grad_reduce_kernel<T>, dim3((unsigned)B), dim3(kPB), 0, h->stream, (const double*)part, (int)per_reg,
                         dmw_d, stridedmw, (int)D, (const T*)mwp_d, smp, a.mw, a.Lw, GradPrior{prior_kind, ldl, strideLw, stridemw}, (const T*)Tf,
                         (const int32_t*)info_d);
  }
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- shared-X multi-output evidence: logpdf(fx, Y::Matrix), optional per-column posterior means ----
template <typename T>
int logpdf_multi(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const T* X, int64_t ldx, const T* Y,
                 int64_t ldY, int noise_kind, const T* s, int prior_kind, const T* mw, const T* Lw, int64_t ldl, double* logpdf,
                 T* mw_post, int64_t ldmp, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 4, "D out of range for this build (1..8192)");
  if (N < 1 || N > (1 << 30)) return bad_arg(h, 5, "N out of range (>= 1)");
  if (S < 0 || S > 65536) return bad_arg(h, 6, "S out of range (0..65536)");
  if (S == 0) return 0;
  if (!X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N) return bad_arg(h, 8, "ldx too small");
  if (!Y) return bad_arg(h, 9, "Y is NULL");
  if (ldY < N) return bad_arg(h, 10, "ldY < N (reference :74 length check)");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL) return bad_arg(h, 11, "noise_kind");
  if (!s) return bad_arg(h, 12, "s is NULL");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 13, "prior_kind");
  if (!mw) return bad_arg(h, 14, "mw is NULL");
  if (!Lw) return bad_arg(h, 15, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 16, "ldl < D");
  if (!logpdf) return bad_arg(h, 17, "logpdf is NULL");
  if (mw_post && ldmp < D) return bad_arg(h, 19, "ldmp < D");
  if (!info) return bad_arg(h, 20, "info is NULL");
  HIP_TRY(h, hipSetDevice(h->device));

  using LC = LargeCfg<T>;
  CallIO io(h, memspace);
  int rc;
  const T *X_d = nullptr, *Y_d = nullptr, *s_d = nullptr, *mw_d = nullptr, *Lw_d = nullptr;
  double* lp_d = nullptr;
  T* mp_d = nullptr;
  int32_t* info_d = nullptr;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  if ((rc = io.in(X, x_one, &X_d))) return rc;
  if ((rc = io.in(Y, mat_extent(N, S, ldY), &Y_d))) return rc;
  if ((rc = io.in(s, noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1, &s_d))) return rc;
  if ((rc = io.in(mw, (size_t)D, &mw_d))) return rc;
  if ((rc = io.in(Lw, lw_one, &Lw_d))) return rc;
  if ((rc = io.out(logpdf, (size_t)S, &lp_d))) return rc;
  if ((rc = io.out(mw_post, mat_extent(D, S, ldmp), &mp_d))) return rc;
  if ((rc = io.out(info, (size_t)1, &info_d))) return rc;
  const int DP = (int)((D + kPB - 1) / kPB * kPB), NC = DP / kPB;
  // fp32, ColVecs, D > 128, up to 128 columns: the residuals of ALL columns ride through the update of column 0 as one more row block of
  // operand planes -- their b_s = X Sigma^-1 (y_s - mu) come out of the same Gram launch (NC + 1 more macro tiles), their u_s = L^-1 b_s
  // out of the same blocked factorisation (rows it carries along anyway), their q_s out of the planes pass.  No residual matrix, no
  // second product over X, no panel sweep of its own (round 6; until then: steps (2) - (5) below, 0.5 ms of a 1.09 ms call at config 3's
  // shape with 64 columns, 9.7 x the algorithmic bytes).
  if constexpr (sizeof(T) == 4) {
    if (D > kMaxSmallD && layout == BLR_LAYOUT_COLVECS && S <= kPB && prior_kind != BLR_PRIOR_UPPER_FACTOR && !h->opt.no_planes &&
        !h->opt.no_bf16x3 && !h->opt.no_fp16_planes && !h->opt.no_multi_planes) {
      void *vTf, *vlp0;
      {
        const size_t sz_tf = mp_d ? (((size_t)D * D * sizeof(T) + 255) & ~(size_t)255) : 0;
        if ((rc = h->aux.reserve(h, sz_tf + 256))) return rc;
        vTf = h->aux.p; vlp0 = h->aux.p + sz_tf;
      }
      T* Tf = static_cast<T*>(vTf);
      double* lp0 = static_cast<double*>(vlp0);
      blr_handle::MultiSrc ms{};
      ms.Y = Y_d; ms.ldY = ldY; ms.S = (int)S;
      PosteriorArgs<T> a{};
      a.X = X_d; a.ldx = ldx; a.strideX = 0; a.y = Y_d; a.stridey = 0; a.s = s_d; a.strides = 0; a.mw = mw_d; a.stridemw = 0;
      a.Lw = Lw_d; a.ldl = ldl; a.strideLw = 0;
      a.mw_post = nullptr; a.stride_mwpost = D; a.T_post = mp_d ? Tf : nullptr; a.ldt = D; a.strideT = D * D;  // (the means need T = L')
      a.Lw_post = nullptr; a.ldlp = D; a.strideLp = 0; a.logpdf = lp0; a.info = info_d;
      a.layout = layout; a.noise_kind = noise_kind; a.prior_kind = prior_kind; a.D = (int)D; a.N = (int)N; a.B = 1;
      a.vec_ok = (D % Mfma<T>::VEC == 0 && aligned16(X_d, ldx, 0)) ? 1 : 0;
      h->multi_src = &ms;
      rc = dispatch_posterior<T>(h, a);
      h->multi_src = nullptr;
      if (rc) return rc;
      if (!ms.done) return hip_fail(h, hipErrorInvalidValue, "multi-output rows were not taken along (internal)");
      hipLaunchKernelGGL(multi_rows_finish_kernel<T>, dim3((unsigned)S), dim3(kThreads), 0, h->stream, (const double*)lp0, (const double*)ms.qsp,
                         ms.nq, noise_kind == BLR_NOISE_ISOTROPIC ? s_d : (const T*)nullptr, (const T*)ms.Abar, ms.lda, ms.DP, (int)D, (int)S, lp_d);
      if (mp_d) {  // m_s = L^-T u_s, one wavefront of workgroups per column (as the weight draws of blr_sample_weights_*)
        WaveSolveArgs<T> b{};
        b.Tf = static_cast<const T*>(ms.Tfull); b.ldtf = ms.DP; b.D = (int)D; b.DP = ms.DP;
        b.rhs = static_cast<const T*>(ms.Abar) + ms.DP; b.ldrhs = 1; b.rhs_inc = ms.lda;
        b.add = mw_d; b.out = mp_d; b.ldout = ldmp;
        if ((rc = launch_wave_solve<T>(h, b, NC, S))) return rc;
      }
      HIP_TRY(h, hipGetLastError());
      return io.finish();
    }
  }
  const int SP = (int)((S + kPB - 1) / kPB * kPB);
  const int NP64 = (int)((N + 63) / 64);
  const int64_t ldy = (int64_t)DP + SP;
  const int ntile_rows = SP / kPB, ntiles = ntile_rows * NC;
  // split-K over N: fill the 512 workgroup slots
  const int max_split = std::max(1, std::min<int>(64, (int)((N + LC::NSC - 1) / LC::NSC)));
  const int nsplit = std::max(1, std::min(max_split, 512 / std::max(1, ntiles)));
  // eleven call-scoped temporaries, carved out of the handle's side buffer (it only grows: no hipMalloc / hipFree -- each of which
  // drains the device -- on a steady-state call; neither the update of step (1) nor the mean stream of step (2) uses that buffer)
  void *vTf, *vlp0, *vmu, *vR, *vq, *vG, *vY, *vsq, *vuu, *vzero, *vinfo2;
  const int64_t ldr = layout == BLR_LAYOUT_COLVECS ? SP : N;
  {
    const size_t sizes[11] = {(size_t)D * D * sizeof(T), sizeof(double), (size_t)N * sizeof(T), (size_t)SP * N * sizeof(T),
                              (size_t)NP64 * SP * sizeof(double), (size_t)nsplit * ntiles * kPB * kPB * sizeof(T),
                              (size_t)ldy * DP * sizeof(T), (size_t)SP * sizeof(double), (size_t)SP * sizeof(T), sizeof(T), sizeof(int32_t)};
    void** const outs[11] = {&vTf, &vlp0, &vmu, &vR, &vq, &vG, &vY, &vsq, &vuu, &vzero, &vinfo2};
    size_t total = 0;
    for (size_t b : sizes) total += (b + 255) & ~(size_t)255;
    if ((rc = h->aux.reserve(h, total))) return rc;
    size_t off = 0;
    for (int i = 0; i < 11; ++i) {
      *outs[i] = h->aux.p + off;
      off += (sizes[i] + 255) & ~(size_t)255;
    }
  }
  T* Tf = static_cast<T*>(vTf);
  double* lp0 = static_cast<double*>(vlp0);
  T* mu = static_cast<T*>(vmu);
  T* R = static_cast<T*>(vR);
  double* qpart = static_cast<double*>(vq);
  T* Gpart = static_cast<T*>(vG);
  T* Ybar = static_cast<T*>(vY);
  double* rowsq = static_cast<double*>(vsq);
  T* uu = static_cast<T*>(vuu);
  T* zero = static_cast<T*>(vzero);
  int32_t* info2 = static_cast<int32_t*>(vinfo2);
  HIP_TRY(h, hipMemsetAsync(zero, 0, sizeof(T), h->stream));
  if (layout == BLR_LAYOUT_COLVECS) HIP_TRY(h, hipMemsetAsync(R, 0, (size_t)SP * N * sizeof(T), h->stream));

  // (1) the ordinary fused update on column 0: factor T, logpdf_0, status
  {
    PosteriorArgs<T> a{};
    a.X = X_d; a.ldx = ldx; a.strideX = 0; a.y = Y_d; a.stridey = 0; a.s = s_d; a.strides = 0; a.mw = mw_d; a.stridemw = 0;
    a.Lw = Lw_d; a.ldl = ldl; a.strideLw = 0;
    a.mw_post = nullptr; a.stride_mwpost = D; a.T_post = Tf; a.ldt = D; a.strideT = D * D;
    a.Lw_post = nullptr; a.ldlp = D; a.strideLp = 0; a.logpdf = lp0; a.info = info_d;
    a.layout = layout; a.noise_kind = noise_kind; a.prior_kind = prior_kind; a.D = (int)D; a.N = (int)N; a.B = 1;
    a.vec_ok = (layout == BLR_LAYOUT_COLVECS && D % Mfma<T>::VEC == 0 && aligned16(X_d, ldx, 0)) ? 1 : 0;
    if ((rc = dispatch_posterior<T>(h, a))) return rc;
  }
  // (2) mu_n = x_n'mw: the mean-only marginal stream
  {
    const AsyncScope no_drain(h, true);
    rc = marginals_batched<T>(h, BLR_MEM_DEVICE, layout, 1, D, N, X_d, ldx, 0, noise_kind, s_d, 0, BLR_PRIOR_DIAGONAL, mw_d, 0,
                              nullptr, 1, 0, mu, N, nullptr, N, info2);
    if (rc) return rc;
  }
  // (3) residuals R = S (Y - mu 1') in X's layout, q partials
  {
    MultiPrepArgs<T> p{};
    p.Y = Y_d; p.ldY = ldY; p.mu = mu; p.s = s_d; p.noise_kind = noise_kind; p.R = R; p.ldr = ldr; p.layout = layout;
    p.qpart = qpart; p.N = (int)N; p.S = (int)S; p.SP = SP;
    hipLaunchKernelGGL(multi_prep_kernel<T>, dim3((unsigned)NP64), dim3(kThreads), 0, h->stream, p);
  }
  // (4) B' = R'X': split-K MFMA tiles, first operand R (rows s), second operand X (rows d)
  if ((rc = set_lds_once(h, gram_tile_kernel<T>, (size_t)LC::LDS_BYTES))) return rc;
  {
    GramTileArgs<T> g{};
    g.X = R; g.ldx = ldr; g.layout = layout; g.D = SP;
    g.XB = X_d; g.ldxb = ldx; g.DB = (int)D;
    g.use_dma = x_ring(layout, X_d, ldx) ? 1 : 0;
    g.s = nullptr; g.noise_kind = NOISE_ISOTROPIC; g.r = nullptr;
    g.n_begin = 0; g.n_end = (int)N; g.nsplit = nsplit;
    g.tile_i0 = 0; g.tile_j0 = 0; g.tri = 3; g.ntile_rows = ntile_rows; g.ntiles = ntiles; g.nblocks = NC;
    g.Gpart = Gpart; g.bpart = nullptr; g.mode_out = 0; g.xcd_swizzle = 0;
    hipLaunchKernelGGL(gram_tile_kernel<T>, dim3(ntiles * nsplit), dim3(kThreads), LC::LDS_BYTES, h->stream, g);
    hipLaunchKernelGGL(multi_reduce_kernel<T>, dim3(ntiles, 16), dim3(kThreads), 0, h->stream, (const T*)Gpart, nsplit, ntiles,
                       ntile_rows, Ybar, ldy, DP);
  }
  // (5) rows b_s' -> b_s'L^-T (|u_s|^2 rides along) -> (means only) b_s'A^-1
  {
    dim3 grid((DP + 31) / 32, (DP + 31) / 32);
    hipLaunchKernelGGL(factor_sym_fill_kernel<T>, grid, dim3(kThreads), 0, h->stream, (const T*)Tf, D, (int)D, DP, Ybar, ldy);
  }
  const TallSweep<T> sweep{h, Ybar, ldy, DP, SP, info_d, 1, 0};
  if ((rc = sweep.prepare())) return rc;
  {
    RowSqArgs<T> rs{};
    rs.acc = rowsq; rs.var = uu; rs.s = zero; rs.noise_kind = BLR_NOISE_ISOTROPIC; rs.N = (int)S;
    sweep.forward(rs);
  }
  hipLaunchKernelGGL(multi_finish_kernel<T>, dim3((unsigned)S), dim3(kThreads), 0, h->stream,
                     (const double*)lp0, (const double*)qpart, NP64, SP, (const T*)uu, (int)S, lp_d);
  if (mp_d) {
    sweep.backward();
    hipLaunchKernelGGL(multi_means_kernel<T>, dim3(1024), dim3(kThreads), 0, h->stream, (const T*)Ybar, ldy, DP, mw_d, (int)D, (int)S,
                       mp_d, ldmp);
  }
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// D > 128: W[:, s] = mw + U^-1 Z[:, s] with U = chol(Lw).U -- the wavefront back substitution of the posterior path with
// one grid column per draw (reference :46-52).  All pointers are device pointers.
template <typename T>
int sample_weights_large(blr_handle* h, int64_t D, int64_t S, int prior_kind, const T* mw, const T* Lw, int64_t ldl,
                         const T* Z, int64_t ldz, T* W, int64_t ldw) {
  if (prior_kind == BLR_PRIOR_DIAGONAL) {
    h->draw_route |= blr_handle::DRAW_W_DIAG;
    hipLaunchKernelGGL(diag_sample_kernel<T>, dim3(1024), dim3(kThreads), 0, h->stream, mw, Lw, Z, ldz, W, ldw, (int)D, S);
    HIP_TRY(h, hipGetLastError());
    return 0;
  }
  h->draw_route |= blr_handle::DRAW_W_LARGE;
  const int DP = (int)((D + kPB - 1) / kPB * kPB), NC = DP / kPB;
  const int64_t chunk = std::min<int64_t>(S, 1024);
  Carve carve;
  const size_t o_tf = carve((size_t)DP * DP * sizeof(T));
  const size_t o_wk = carve(prior_kind == BLR_PRIOR_DENSE ? (size_t)DP * DP * sizeof(T) : 0);
  const size_t o_info = carve(64);
  int rc = h->ws.reserve(h, carve.off, blr_handle::kWsFloor);
  if (rc) return rc;
  char* ws = h->ws.p;
  T* Tf = reinterpret_cast<T*>(ws + o_tf);
  int32_t* info_dev = reinterpret_cast<int32_t*>(ws + o_info);
  if (prior_kind == BLR_PRIOR_UPPER_FACTOR) {
    hipLaunchKernelGGL(upper_pad_kernel<T>, dim3(1024), dim3(kThreads), 0, h->stream, Lw, ldl, (int)D, DP, Tf, (int64_t)DP);
  } else {
    T* Wk = reinterpret_cast<T*>(ws + o_wk);
    HIP_TRY(h, hipMemsetAsync(info_dev, 0, 64, h->stream));
    hipLaunchKernelGGL(prior_copy_kernel<T>, dim3(1024), dim3(kThreads), 0, h->stream, Lw, ldl, (int)D, DP, Wk, (int64_t)DP);
    if ((rc = chol_large<T>(h, Wk, DP, DP, DP, info_dev))) return rc;
    dim3 grid((DP + 31) / 32, (DP + 31) / 32);
    hipLaunchKernelGGL(transpose_out_kernel<T>, grid, dim3(kThreads), 0, h->stream, (const T*)Wk, (int64_t)DP, DP, Tf,
                       (int64_t)DP, (T*)nullptr, (int64_t)0, 0);
    int32_t hinfo = 0;
    HIP_TRY(h, hipMemcpyAsync(&hinfo, info_dev, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (hinfo != 0) return hinfo;  // the prior precision is not positive definite
  }
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t ns = std::min(chunk, S - s0);
    WaveSolveArgs<T> b{};
    b.Tf = Tf; b.ldtf = DP; b.D = (int)D; b.DP = DP;
    b.rhs = Z + s0 * ldz; b.ldrhs = ldz; b.rhs_inc = 1;
    b.add = mw; b.out = W + s0 * ldw; b.ldout = ldw;
    if ((rc = launch_wave_solve<T>(h, b, NC, ns))) return rc;
  }
  HIP_TRY(h, hipGetLastError());
  return 0;
}

template <typename T>
int sample_weights_impl(blr_handle* h, CallIO& io, int64_t D, int64_t S, int prior_kind, const T* mw, const T* Lw,
                        int64_t ldl, const T* Z, int64_t ldz, T* W, int64_t ldw, T** W_dev_out) {  // (the caller's io.finish() ends the call)
  const T *mw_d = nullptr, *Lw_d = nullptr, *Z_d = nullptr;
  T* W_d = nullptr;
  int rc;
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  if ((rc = io.in(mw, (size_t)D, &mw_d))) return rc;
  if ((rc = io.in(Lw, lw_one, &Lw_d))) return rc;
  if ((rc = io.in(Z, mat_extent(D, S, ldz), &Z_d))) return rc;
  if ((rc = io.out(W, mat_extent(D, S, ldw), &W_d))) return rc;
  if (!W_d) {  // internal temporary (rand): dense D x S, in the handle's grow-only side buffer -- a hipMalloc / hipFree pair and
               // the drain in front of the free were most of a small call (64 draws at D = 128: 68 us, the kernels 20)
    if ((rc = h->aux.reserve(h, (size_t)D * S * sizeof(T)))) return rc;
    W_d = reinterpret_cast<T*>(h->aux.p);
    ldw = D;
  }
  if (D > kMaxSmallD) {
    if ((rc = sample_weights_large<T>(h, D, S, prior_kind, mw_d, Lw_d, ldl, Z_d, ldz, W_d, ldw))) return rc;
    if (W_dev_out) *W_dev_out = W_d;
    return 0;
  }
  const T* U;
  int64_t ldu, strideU;
  int kind;
  int32_t* chol_info;
  if ((rc = prior_factor<T>(h, 1, D, prior_kind, Lw_d, ldl, 0, &U, &ldu, &strideU, &kind, &chol_info))) return rc;
  int32_t hinfo = 0;
  if (chol_info) {
    HIP_TRY(h, hipMemcpyAsync(&hinfo, chol_info, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (hinfo != 0) return hinfo;
  }
  if (kind == BLR_PRIOR_DIAGONAL) {
    h->draw_route |= blr_handle::DRAW_W_DIAG;
    hipLaunchKernelGGL(diag_sample_kernel<T>, dim3(1024), dim3(kThreads), 0, h->stream, mw_d, U, Z_d, ldz, W_d, ldw, (int)D, S);
  } else {  // draws as rows of an LDS block, one backward MFMA sweep per tile of draws
    // (the stat repeats the predicate of the kernel's 16-byte loader of U; the kernel decides for itself)
    const bool uvec = D == kPB && (ldu % Mfma<T>::VEC) == 0 && ((uintptr_t)U % 16) == 0;
    h->draw_route |= blr_handle::DRAW_W_MFMA | (uvec ? blr_handle::DRAW_W_UVEC : 0);
    using TC = TrsmCfg<T>;
    const int lds = TC::LDS_BYTES + kPB * (int)sizeof(T);
    auto kern = sample_weights_mfma_kernel<T>;
    if (const int rc_lds = set_lds_once(h, kern, (size_t)(lds))) return rc_lds;
    const int64_t ntiles = (S + TC::RB - 1) / TC::RB;
    hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(ntiles, 512)), dim3(kThreads), lds, h->stream, mw_d, U, ldu, Z_d, ldz,
                       W_d, ldw, (int)D, S);
  }
  HIP_TRY(h, hipGetLastError());
  if (W_dev_out) *W_dev_out = W_d;
  return 0;
}

template <typename T>
int sample_weights(blr_handle* h, int memspace, int64_t D, int64_t S, int prior_kind, const T* mw, const T* Lw,
                   int64_t ldl, const T* Z, int64_t ldz, T* W, int64_t ldw) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->draw_route = 0;  // (the host code that picks each launch sets its bit)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 3, "D out of range for this build (1..8192)");
  if (S < 0) return bad_arg(h, 4, "S < 0");
  if (S == 0) return 0;
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 5, "prior_kind");
  if (!mw) return bad_arg(h, 6, "mw is NULL");
  if (!Lw) return bad_arg(h, 7, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 8, "ldl < D");
  if (!Z) return bad_arg(h, 9, "Z is NULL");
  if (ldz < D) return bad_arg(h, 10, "ldz < D");
  if (!W) return bad_arg(h, 11, "W is NULL");
  if (ldw < D) return bad_arg(h, 12, "ldw < D");
  HIP_TRY(h, hipSetDevice(h->device));
  CallIO io(h, memspace);
  const int rc = sample_weights_impl<T>(h, io, D, S, prior_kind, mw, Lw, ldl, Z, ldz, W, ldw, nullptr);
  return rc ? rc : io.finish();
}

// Y (N x S) = X'W (+ sqrt.(s) .* Z2 when Z2 != NULL): device pointers
template <typename T>
void launch_project(blr_handle* h, int layout, int64_t D, int64_t N, int64_t S, const T* X_d, int64_t ldx, const T* W_d, int64_t ldw,
                    const T* s_d, int noise_kind, const T* Z2_d, int64_t ldz2, T* Y_d, int64_t ldy) {
  constexpr int kVec = Mfma<T>::VEC;
  const bool no_mfma_proj = h->opt.no_mfma_project;  // A/B experiments only
  if (!no_mfma_proj && layout == BLR_LAYOUT_COLVECS && D % kVec == 0 && aligned16(X_d, ldx, 0) && aligned16(W_d, ldw, 0)) {
    // tall-skinny GEMM on the matrix cores
    h->draw_route |= blr_handle::DRAW_P_MFMA;
    using PC = ProjCfg<T>;
    dim3 grid((unsigned)((N + PC::TN - 1) / PC::TN), (unsigned)((S + PC::TS - 1) / PC::TS));
    hipLaunchKernelGGL(rand_project_mfma_kernel<T>, grid, dim3(kThreads), PC::LDS_BYTES, h->stream, X_d, ldx, W_d, ldw, s_d, noise_kind,
                       Z2_d, ldz2, Y_d, ldy, (int)D, (int)N, S);
  } else {
    h->draw_route |= blr_handle::DRAW_P_SCALAR;
    dim3 grid((unsigned)((N + 63) / 64), (unsigned)((S + 63) / 64));
    hipLaunchKernelGGL(rand_project_kernel<T>, grid, dim3(kThreads), 0, h->stream, X_d, ldx, layout, W_d, ldw, s_d, noise_kind, Z2_d,
                       ldz2, Y_d, ldy, (int)D, (int)N, S);
  }
}

// ---- Y = X'W for S given weight vectors: evaluation of function samples (reference sampling_functions.jl:16-18) ------------
template <typename T>
int apply_weights(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const T* X, int64_t ldx, const T* W,
                  int64_t ldw, T* Y, int64_t ldy) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->draw_route = 0;  // (the host code that picks each launch sets its bit)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (D < 1 || D > (1 << 30)) return bad_arg(h, 4, "D out of range");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 5, "N out of range");
  if (S < 0 || S > (1 << 30)) return bad_arg(h, 6, "S out of range");
  if (N == 0 || S == 0) return 0;
  if (!X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N) return bad_arg(h, 8, "ldx too small");
  if (!W) return bad_arg(h, 9, "W is NULL");
  if (ldw < D) return bad_arg(h, 10, "ldw < D");
  if (!Y) return bad_arg(h, 11, "Y is NULL");
  if (ldy < N) return bad_arg(h, 12, "ldy < N");
  HIP_TRY(h, hipSetDevice(h->device));
  CallIO io(h, memspace);
  const T *X_d = nullptr, *W_d = nullptr;
  T* Y_d = nullptr;
  int rc;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  if ((rc = io.in(X, x_one, &X_d))) return rc;
  if ((rc = io.in(W, mat_extent(D, S, ldw), &W_d))) return rc;
  if ((rc = io.out(Y, mat_extent(N, S, ldy), &Y_d))) return rc;
  launch_project<T>(h, layout, D, N, S, X_d, ldx, W_d, ldw, (const T*)nullptr, BLR_NOISE_ISOTROPIC, (const T*)nullptr, 0, Y_d, ldy);
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

template <typename T>
int rand_impl(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const T* X, int64_t ldx,
              int noise_kind, const T* s, int prior_kind, const T* mw, const T* Lw, int64_t ldl, const T* Z1,
              int64_t ldz1, const T* Z2, int64_t ldz2, T* Y, int64_t ldy) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->draw_route = 0;  // (the host code that picks each launch sets its bit)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 4, "D out of range for this build (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 5, "N out of range");
  if (S < 0) return bad_arg(h, 6, "S < 0");
  if (N == 0 || S == 0) return 0;
  if (!X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N) return bad_arg(h, 8, "ldx too small");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL) return bad_arg(h, 9, "noise_kind");
  if (!s) return bad_arg(h, 10, "s is NULL");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 11, "prior_kind");
  if (!mw) return bad_arg(h, 12, "mw is NULL");
  if (!Lw) return bad_arg(h, 13, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 14, "ldl < D");
  if (!Z1) return bad_arg(h, 15, "Z1 is NULL");
  if (ldz1 < D) return bad_arg(h, 16, "ldz1 < D");
  if (!Z2) return bad_arg(h, 17, "Z2 is NULL");
  if (ldz2 < N) return bad_arg(h, 18, "ldz2 < N");
  if (!Y) return bad_arg(h, 19, "Y is NULL");
  if (ldy < N) return bad_arg(h, 20, "ldy < N");
  HIP_TRY(h, hipSetDevice(h->device));
  CallIO io(h, memspace);
  T* W_dev = nullptr;
  // weights first (Z1 is the FIRST randn draw of reference :51), host staging handled inside
  int rc = sample_weights_impl<T>(h, io, D, S, prior_kind, mw, Lw, ldl, Z1, ldz1, (T*)nullptr, D, &W_dev);
  if (rc) return rc;
  const T *X_d = nullptr, *s_d = nullptr, *Z2_d = nullptr;
  T* Y_d = nullptr;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  if ((rc = io.in(X, x_one, &X_d))) return rc;
  if ((rc = io.in(s, noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1, &s_d))) return rc;
  if ((rc = io.in(Z2, mat_extent(N, S, ldz2), &Z2_d))) return rc;
  if ((rc = io.out(Y, mat_extent(N, S, ldy), &Y_d))) return rc;
  launch_project<T>(h, layout, D, N, S, X_d, ldx, (const T*)W_dev, (int64_t)D, s_d, noise_kind, Z2_d, ldz2, Y_d, ldy);
  HIP_TRY(h, hipGetLastError());
  // (W_dev lives in the handle's side buffer, which is only ever replaced behind a stream synchronisation)
  return io.finish();
}

// ---- draws from B regressors in one call (blr_rand_batched_*; reference :49-53 and sampling_functions.jl:27-49 under a map) ------
// D <= 128: [one batched Cholesky of a dense prior] + rand_batched_solve_kernel (+ one projection launch unless it is fused): the
// launch count does not depend on B, and nothing a launch computes for regressor b depends on B or on the other regressors.
// D > 128: one regressor at a time on sample_weights_large + launch_project (correct, not fast; synchronises for the status).
template <typename T>
int rand_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, const T* X, int64_t ldx,
                 int64_t strideX, int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw, int64_t stridemw,
                 const T* Lw, int64_t ldl, int64_t strideLw, const T* Z1, int64_t ldz1, int64_t strideZ1, const T* Z2, int64_t ldz2,
                 int64_t strideZ2, T* W, int64_t ldw, int64_t strideW, T* Y, int64_t ldy, int64_t strideY, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->draw_route = 0;  // (the host code that picks each launch sets its bit)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range for this build (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range");
  if (S < 0 || S > (1 << 30)) return bad_arg(h, 7, "S out of range");
  const bool proj = Y && N > 0;  // Y = NULL: weights only
  const bool noisy = proj && Z2;  // Z2 = NULL: noise-free function values, noise_kind and s ignored
  if (proj && !X) return bad_arg(h, 8, "X is NULL");
  if (proj && (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N)) return bad_arg(h, 9, "ldx too small");
  if (strideX < 0) return bad_arg(h, 10, "strideX < 0");
  if (noisy && noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL) return bad_arg(h, 11, "noise_kind");
  if (noisy && !s) return bad_arg(h, 12, "s is NULL");
  if (strides < 0) return bad_arg(h, 13, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 14, "prior_kind");
  if (!mw) return bad_arg(h, 15, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 16, "stridemw < 0");
  if (!Lw) return bad_arg(h, 17, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 18, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 19, "strideLw < 0");
  if (!Z1) return bad_arg(h, 20, "Z1 is NULL");
  if (ldz1 < D) return bad_arg(h, 21, "ldz1 < D");
  if (strideZ1 < 0) return bad_arg(h, 22, "strideZ1 < 0");
  if (noisy && ldz2 < N) return bad_arg(h, 24, "ldz2 < N");
  if (strideZ2 < 0) return bad_arg(h, 25, "strideZ2 < 0");
  if (W && ldw < D) return bad_arg(h, 27, "ldw < D");
  if (W && B > 1 && strideW < ldw * S) return bad_arg(h, 28, "strideW < ldw * S: the outputs of two regressors overlap");
  if (Y && ldy < N) return bad_arg(h, 30, "ldy < N");
  if (Y && B > 1 && strideY < ldy * S) return bad_arg(h, 31, "strideY < ldy * S: the outputs of two regressors overlap");
  if (!info) return bad_arg(h, 32, "info is NULL");
  if (B == 0 || S == 0) return 0;
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  const T *X_d = nullptr, *s_d = nullptr, *mw_d = nullptr, *Lw_d = nullptr, *Z1_d = nullptr, *Z2_d = nullptr;
  T *W_d = nullptr, *Y_d = nullptr;
  int32_t* info_d = nullptr;
  int rc;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  // (X without a projection and s without noise are not staged: a count of 0)
  if ((rc = io.in(X, proj ? extent(B, strideX, x_one) : 0, &X_d))) return rc;
  if ((rc = io.in(s, noisy ? extent(B, strides, noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1) : 0, &s_d))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &mw_d))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &Lw_d))) return rc;
  if ((rc = io.in(Z1, extent(B, strideZ1, mat_extent(D, S, ldz1)), &Z1_d))) return rc;
  if ((rc = io.in(noisy ? Z2 : (const T*)nullptr, extent(B, strideZ2, mat_extent(N, S, ldz2)), &Z2_d))) return rc;
  if ((rc = io.out(W, extent(B, strideW, mat_extent(D, S, ldw)), &W_d))) return rc;
  if ((rc = io.out(proj ? Y : (T*)nullptr, extent(B, strideY, mat_extent(N, S, ldy)), &Y_d))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_d))) return rc;

  if (D > kMaxSmallD) {
    std::vector<int32_t> hinfo((size_t)B, 0);
    if (prior_kind != BLR_PRIOR_DENSE) {
      hipLaunchKernelGGL(rand_batched_status_kernel<T>, dim3((unsigned)std::min<int64_t>((B + kWaves - 1) / kWaves, 1 << 16)),
                         dim3(kThreads), 0, h->stream, Lw_d, ldl, strideLw, prior_kind == BLR_PRIOR_DIAGONAL ? 1 : 0, (int)D, B, info_d);
      HIP_TRY(h, hipGetLastError());
      HIP_TRY(h, hipMemcpyAsync(hinfo.data(), info_d, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    T* Wtmp = nullptr;
    if (!W_d) {
      if ((rc = h->aux.reserve(h, (size_t)D * S * sizeof(T)))) return rc;
      Wtmp = reinterpret_cast<T*>(h->aux.p);
    }
    for (int64_t b = 0; b < B; ++b) {
      if (hinfo[b]) continue;
      T* Wb = W_d ? W_d + b * strideW : Wtmp;
      const int64_t ldwb = W_d ? ldw : D;
      rc = sample_weights_large<T>(h, D, S, prior_kind, mw_d + b * stridemw, Lw_d + b * strideLw, ldl, Z1_d + b * strideZ1, ldz1, Wb, ldwb);
      if (rc < 0) return rc;
      if (rc > 0) { hinfo[b] = rc; continue; }  // a dense prior that is not positive definite: nothing was written
      if (proj)
        launch_project<T>(h, layout, D, N, S, X_d + b * strideX, ldx, (const T*)Wb, ldwb, noisy ? s_d + b * strides : nullptr, noise_kind,
                          Z2_d ? Z2_d + b * strideZ2 : nullptr, ldz2, Y_d + b * strideY, ldy);
      HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipMemcpyAsync(info_d, hinfo.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // (hinfo is a host temporary)
    return io.finish();
  }

  RandBatchedArgs<T> a{};
  a.layout = layout; a.noise_kind = noise_kind; a.D = (int)D; a.N = (int)N; a.S = S; a.B = B;
  a.X = X_d; a.ldx = ldx; a.strideX = strideX;
  a.s = s_d; a.strides = strides;
  a.mw = mw_d; a.stridemw = stridemw;
  a.Z1 = Z1_d; a.ldz1 = ldz1; a.strideZ1 = strideZ1;
  a.Z2 = Z2_d; a.ldz2 = ldz2; a.strideZ2 = strideZ2;
  a.W = W_d; a.ldw = ldw; a.strideW = strideW;
  a.Y = Y_d; a.ldy = ldy; a.strideY = strideY;
  a.info = info_d;
  int kind = prior_kind;
  int32_t* chol_info = nullptr;
  if ((rc = prior_factor<T>(h, B, D, prior_kind, Lw_d, ldl, strideLw, &a.U, &a.ldu, &a.strideU, &kind, &chol_info))) return rc;
  a.prior_kind = kind;
  a.chol_info = chol_info;
  // the route depends on N, S, D, the layout and the alignment of X -- never on B
  const bool fuse = proj && N * S <= 512;
  const int ns = S == 1 ? 1 : 4;
  a.nsb = (S + ns - 1) / ns;
  if (proj && !fuse) {  // the weights for the projection launch: ld rounded to 16 bytes, so its operand loads are aligned
    a.ldwt = (D + 3) & ~(int64_t)3;
    a.strideWt = a.ldwt * S;
    if ((rc = h->aux.reserve(h, (size_t)B * a.strideWt * sizeof(T)))) return rc;
    a.Wt = reinterpret_cast<T*>(h->aux.p);
  }
  const bool mfma = !h->opt.no_mfma_project && layout == BLR_LAYOUT_COLVECS && D % Mfma<T>::VEC == 0 && aligned16(X_d, ldx, strideX);
  const int tn = mfma ? ProjCfg<T>::TN : 64, ts = mfma ? ProjCfg<T>::TS : 64;
  const int ntn = (int)((N + tn - 1) / tn);
  const int64_t nts = (S + ts - 1) / ts;
  if (proj && !fuse && nts > 65535) return bad_arg(h, 7, "S too large for the projection grid");
  const unsigned blocks = (unsigned)std::min<int64_t>((B * a.nsb + kWaves - 1) / kWaves, 1 << 20);
  void (*solve)(RandBatchedArgs<T>);
  if (ns == 1) solve = fuse ? rand_batched_solve_kernel<T, 1, true> : rand_batched_solve_kernel<T, 1, false>;
  else         solve = fuse ? rand_batched_solve_kernel<T, 4, true> : rand_batched_solve_kernel<T, 4, false>;
  h->draw_route |= (ns == 1 ? blr_handle::DRAW_W_BATCHED_NS1 : blr_handle::DRAW_W_BATCHED_NS4) | (fuse ? blr_handle::DRAW_P_FUSED : 0);
  hipLaunchKernelGGL(solve, dim3(blocks), dim3(kThreads), 0, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  if (proj && !fuse) {
    const int64_t per_launch = h->cap_chunk(std::max<int64_t>(1, ((int64_t)1 << 24) / ntn));
    h->count_chunks(B, per_launch);
    h->draw_route |= mfma ? blr_handle::DRAW_P_MFMA : blr_handle::DRAW_P_SCALAR;
    for (int64_t b0 = 0; b0 < B; b0 += per_launch) {
      const int64_t nreg = std::min<int64_t>(per_launch, B - b0);
      const dim3 grid((unsigned)(nreg * ntn), (unsigned)nts);
      if (mfma)
        hipLaunchKernelGGL(rand_batched_project_mfma_kernel<T>, grid, dim3(kThreads), ProjCfg<T>::LDS_BYTES, h->stream, a, ntn, b0, nreg);
      else
        hipLaunchKernelGGL(rand_batched_project_kernel<T>, grid, dim3(kThreads), 0, h->stream, a, ntn, b0, nreg);
      HIP_TRY(h, hipGetLastError());
    }
  }
  return io.finish();
}

// ---- draws from a batched multi-output state: S column posteriors per regressor share one factor, R draws each
// (blr_rand_multi_batched_*; blr_rand_multi.hpp) ---------------------------------------------------------------------
// D <= 128: [one batched Cholesky of a dense prior] + per chunk of regressors rand_cols_solve_kernel (status, factor in LDS, 16 draw
// columns per pass) + rand_cols_project_kernel (X read once whatever S R is): the launch count depends on B only through the chunks.
// D > 128: column by column through rand_batched (correct, not fast; synchronises).
template <typename T>
int rand_multi_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, int64_t R, const T* X,
                       int64_t ldx, int64_t strideX, int noise_kind, const T* s, int64_t strides, int prior_kind, const T* M, int64_t ldm,
                       int64_t strideM, const T* Lw, int64_t ldl, int64_t strideLw, const T* Z1, int64_t ldz1, int64_t strideZ1,
                       const T* Z2, int64_t ldz2, int64_t strideZ2, T* W, int64_t ldw, int64_t strideW, T* Y, int64_t ldy,
                       int64_t strideY, int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range");
  if (S < 0 || S > (1 << 20)) return bad_arg(h, 7, "S out of range (0..2^20)");
  if (R < 0 || R > (1 << 20) || S * R > (1 << 20)) return bad_arg(h, 8, "R out of range (S*R <= 2^20)");
  const int64_t SR = S * R;
  const bool proj = Y && N > 0;   // Y = NULL: weights only
  const bool noisy = proj && Z2;  // Z2 = NULL: noise-free function values, noise_kind and s ignored
  if (proj && !X) return bad_arg(h, 9, "X is NULL");
  if (proj && (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N)) return bad_arg(h, 10, "ldx too small");
  if (strideX < 0) return bad_arg(h, 11, "strideX < 0");
  if (noisy && noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 12, "noise_kind (isotropic or diagonal; dense Sigma_y is not supported for batched draws)");
  if (noisy && !s) return bad_arg(h, 13, "s is NULL");
  if (strides < 0) return bad_arg(h, 14, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 15, "prior_kind");
  if (!M) return bad_arg(h, 16, "M is NULL");
  if (ldm < D) return bad_arg(h, 17, "ldm < D");
  if (strideM < 0) return bad_arg(h, 18, "strideM < 0");
  if (!Lw) return bad_arg(h, 19, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 20, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 21, "strideLw < 0");
  if (!Z1) return bad_arg(h, 22, "Z1 is NULL");
  if (ldz1 < D) return bad_arg(h, 23, "ldz1 < D");
  if (strideZ1 < 0) return bad_arg(h, 24, "strideZ1 < 0");
  if (noisy && ldz2 < N) return bad_arg(h, 26, "ldz2 < N");
  if (strideZ2 < 0) return bad_arg(h, 27, "strideZ2 < 0");
  if (W && ldw < D) return bad_arg(h, 29, "ldw < D");
  if (W && B > 1 && strideW < ldw * SR) return bad_arg(h, 30, "strideW < ldw * S * R: the outputs of two regressors overlap");
  if (Y && ldy < N) return bad_arg(h, 32, "ldy < N");
  if (Y && B > 1 && strideY < ldy * SR) return bad_arg(h, 33, "strideY < ldy * S * R: the outputs of two regressors overlap");
  if (!info) return bad_arg(h, 34, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  if (B == 0 || SR == 0 || (!W && !Y)) return 0;
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  const T *X_d = nullptr, *s_d = nullptr, *M_d = nullptr, *Lw_d = nullptr, *Z1_d = nullptr, *Z2_d = nullptr;
  T *W_d = nullptr, *Y_d = nullptr;
  int32_t* info_d = nullptr;
  int rc;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  // (X without a projection and s without noise are not staged: a count of 0)
  if ((rc = io.in(X, proj ? extent(B, strideX, x_one) : 0, &X_d))) return rc;
  if ((rc = io.in(s, noisy ? extent(B, strides, noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1) : 0, &s_d))) return rc;
  if ((rc = io.in(M, extent(B, strideM, mat_extent(D, S, ldm)), &M_d))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &Lw_d))) return rc;
  if ((rc = io.in(Z1, extent(B, strideZ1, mat_extent(D, SR, ldz1)), &Z1_d))) return rc;
  if ((rc = io.in(noisy ? Z2 : (const T*)nullptr, extent(B, strideZ2, mat_extent(N, SR, ldz2)), &Z2_d))) return rc;
  if ((rc = io.out(W, extent(B, strideW, mat_extent(D, SR, ldw)), &W_d))) return rc;
  if ((rc = io.out(proj ? Y : (T*)nullptr, extent(B, strideY, mat_extent(N, SR, ldy)), &Y_d))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_d))) return rc;

  if (D > kMaxSmallD) {
    // correct, not fast: the R draws of column c are one call of the single-column route with mw = M[:, c]; every such call forms the
    // same status (a failed regressor's outputs stay untouched in each of them); the route synchronises
    const AsyncScope drain(h, false);
    for (int64_t c = 0; c < S; ++c) {
      rc = rand_batched<T>(h, BLR_MEM_DEVICE, layout, B, D, N, R, X_d, ldx, strideX, noise_kind, s_d, strides, prior_kind, M_d + c * ldm,
                           strideM, Lw_d, ldl, strideLw, Z1_d + c * R * ldz1, ldz1, strideZ1, Z2_d ? Z2_d + c * R * ldz2 : (const T*)nullptr,
                           ldz2, strideZ2, W_d ? W_d + c * R * ldw : (T*)nullptr, ldw, strideW, Y_d ? Y_d + c * R * ldy : (T*)nullptr, ldy,
                           strideY, info_d);
      if (rc) return rc;  // (device pointers and in-range sizes: a HIP failure, not an argument index of the inner call)
    }
    h->last_chunks = 1;
    return io.finish();
  }

  RandColsArgs<T> a{};
  a.noise_kind = noise_kind; a.D = (int)D; a.N = (int)N; a.R = (int)R; a.SR = (int)SR;
  a.ldx = ldx; a.strideX = strideX; a.strides = strides; a.ldm = ldm; a.strideM = strideM;
  a.ldz1 = ldz1; a.strideZ1 = strideZ1; a.ldz2 = ldz2; a.strideZ2 = strideZ2;
  a.ldw = ldw; a.strideW = strideW; a.ldy = ldy; a.strideY = strideY;
  int kind = prior_kind;
  int32_t* chol_info = nullptr;
  if ((rc = prior_factor<T>(h, B, D, prior_kind, Lw_d, ldl, strideLw, &a.U, &a.ldu, &a.strideU, &kind, &chol_info))) return rc;
  a.prior_kind = kind;
  a.chol_info = chol_info;
  // regressors per launch: grid.y, and the fragment images of the weights within 256 MiB (at least one regressor)
  const size_t img_one = rand_cols_image_elems((int)D, SR);
  int64_t chunk = std::min<int64_t>(B, 65535);
  if (proj) chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / (img_one * sizeof(T)))));
  chunk = h->cap_chunk(chunk);
  h->count_chunks(B, chunk);
  const size_t lds_s = rand_cols_solve_lds_bytes(sizeof(T), (int)D, kind == BLR_PRIOR_DIAGONAL);
  const size_t lds_p = rand_cols_project_lds_bytes(sizeof(T), (int)D);
  void (*const project)(RandColsArgs<T>) = layout == BLR_LAYOUT_ROWVECS ? rand_cols_project_kernel<T, LAYOUT_ROWVECS> : rand_cols_project_kernel<T, LAYOUT_COLVECS>;
  if (lds_s && (rc = set_lds_once(h, rand_cols_solve_kernel<T>, lds_s))) return rc;
  if (proj && (rc = set_lds_once(h, project, lds_p))) return rc;
  if (proj && (rc = h->aux.reserve(h, (size_t)chunk * img_one * sizeof(T)))) return rc;
  const int64_t passes = (SR + kRandColsPerPass - 1) / kRandColsPerPass;
  const int64_t ntiles = (N + kMargTile - 1) / kMargTile;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, B - b0);
    const int64_t ngroups = tile_groups(h, ntiles, nb);  // (the projection's)
    a.X = X_d; a.s = s_d; a.M = M_d; a.Z1 = Z1_d; a.Z2 = Z2_d; a.W = W_d; a.Y = Y_d; a.info = info_d;
    a.Wf = proj ? reinterpret_cast<T*>(h->aux.p) : nullptr;
    a.ngroups = (int)ngroups; a.reg0 = (int)b0; a.nreg = (int)nb;
    hipLaunchKernelGGL(rand_cols_solve_kernel<T>, dim3((unsigned)passes, (unsigned)nb), dim3(kThreads), lds_s, h->stream, a);
    if (proj) hipLaunchKernelGGL(project, dim3((unsigned)(ngroups * nb)), dim3(kThreads), lds_p, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}


template <typename T>
int rff_features(blr_handle* h, int memspace, int64_t Din, int64_t D, int64_t N, const T* Xin, int64_t ldxin,
                 const T* Omega, int64_t ldo, const T* phase, T scale, T* Phi, int64_t ldphi) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (Din < 1) return bad_arg(h, 3, "Din < 1");
  if (D < 1) return bad_arg(h, 4, "D < 1");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 5, "N out of range");
  if (N == 0) return 0;
  if (!Xin) return bad_arg(h, 6, "Xin is NULL");
  if ((N + 15) / 16 > 65535) return bad_arg(h, 5, "N > 1048560 inputs per feature-map call (launch geometry)");
  if (ldxin < Din) return bad_arg(h, 7, "ldxin < Din");
  if (!Omega) return bad_arg(h, 8, "Omega is NULL");
  if (ldo < Din) return bad_arg(h, 9, "ldo < Din");
  if (!phase) return bad_arg(h, 10, "phase is NULL");
  if (!Phi) return bad_arg(h, 12, "Phi is NULL");
  if (ldphi < D) return bad_arg(h, 13, "ldphi < D");
  HIP_TRY(h, hipSetDevice(h->device));
  CallIO io(h, memspace);
  const T *Xd = nullptr, *Od = nullptr, *Pd = nullptr;
  T* Fd = nullptr;
  int rc;
  if ((rc = io.in(Xin, mat_extent(Din, N, ldxin), &Xd))) return rc;
  if ((rc = io.in(Omega, mat_extent(Din, D, ldo), &Od))) return rc;
  if ((rc = io.in(phase, (size_t)D, &Pd))) return rc;
  if ((rc = io.out(Phi, mat_extent(D, N, ldphi), &Fd))) return rc;
  dim3 grid((unsigned)((D + kThreads - 1) / kThreads), (unsigned)((N + 31) / 32));  // 32 columns per workgroup (rff_features_kernel NT)
  hipLaunchKernelGGL(rff_features_kernel<T>, grid, dim3(kThreads), 0, h->stream, Xd, ldxin, Od, ldo, Pd, scale, (int)Din,
                     (int)D, (int)N, Fd, ldphi);
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

template <typename T>
int posterior_rff(blr_handle* h, int memspace, int64_t Din, int64_t D, int64_t N, const T* Xin, int64_t ldxin,
                  const T* Omega, int64_t ldo, const T* phase, T scale, const T* y, int noise_kind, const T* s,
                  int prior_kind, const T* mw, const T* Lw, int64_t ldl, T* mw_post, T* T_post, int64_t ldt, T* Lw_post,
                  int64_t ldlp, double* logpdf, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (Din < 1) return bad_arg(h, 3, "Din < 1");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 4, "D out of range");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 5, "N out of range");
  if (N > 0 && !Xin) return bad_arg(h, 6, "Xin is NULL");
  if (ldxin < Din) return bad_arg(h, 7, "ldxin < Din");
  if (!Omega) return bad_arg(h, 8, "Omega is NULL");
  if (ldo < Din) return bad_arg(h, 9, "ldo < Din");
  if (!phase) return bad_arg(h, 10, "phase is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  // fp32 at D > 128, D_in <= kRffFusedMaxDin: the basis is never materialised -- the planes pass of the large-D pipeline evaluates phi
  // once per element and writes the bf16 planes of the Gram operands directly (blr_planes.hpp; reference
  // src/basis_function_regression.jl:41 builds phi(x)).  A wider input materialises the features below (the planes Gram still runs on them).
  const bool fused = sizeof(T) == 4 && D > kMaxSmallD && N > 0 && Din <= kRffFusedMaxDin && !h->opt.no_planes && !h->opt.no_bf16x3;
  if (memspace == BLR_MEM_HOST) {
    if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL) return bad_arg(h, 13, "noise_kind");
    if (!y && N > 0) return bad_arg(h, 12, "y is NULL");
    if (!s) return bad_arg(h, 14, "s is NULL");
    if (!mw) return bad_arg(h, 16, "mw is NULL");
    if (!Lw) return bad_arg(h, 17, "Lw is NULL");
    if (!info) return bad_arg(h, 25, "info is NULL");
  }
  CallIO io(h, memspace);
  int rc;
  const T *Xd = nullptr, *Od = nullptr, *Pd = nullptr;
  PosteriorArgs<T> a{};
  a.strideX = 0; a.stridey = 0; a.strides = 0; a.stridemw = 0; a.ldl = ldl; a.strideLw = 0;
  a.stride_mwpost = D; a.ldt = ldt; a.strideT = ldt * D; a.ldlp = ldlp; a.strideLp = ldlp * D;
  a.layout = BLR_LAYOUT_COLVECS; a.noise_kind = noise_kind; a.prior_kind = prior_kind;
  a.D = (int)D; a.N = (int)N; a.B = 1;
  if ((rc = io.in(Xin, mat_extent(Din, N, ldxin), &Xd))) return rc;
  if ((rc = io.in(Omega, mat_extent(Din, D, ldo), &Od))) return rc;
  if ((rc = io.in(phase, (size_t)D, &Pd))) return rc;
  if ((rc = io.in(y, (size_t)N, &a.y))) return rc;
  if ((rc = io.in(s, noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1, &a.s))) return rc;
  if ((rc = io.in(mw, (size_t)D, &a.mw))) return rc;
  if ((rc = io.in(Lw, prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl), &a.Lw))) return rc;
  if ((rc = io.out(mw_post, (size_t)D, &a.mw_post))) return rc;
  if ((rc = io.out(T_post, mat_extent(D, D, ldt), &a.T_post))) return rc;
  if ((rc = io.out(Lw_post, mat_extent(D, D, ldlp), &a.Lw_post))) return rc;
  if ((rc = io.out(logpdf, 1, &a.logpdf))) return rc;
  if ((rc = io.out(info, 1, &a.info))) return rc;
  if (fused) {
    // (X: any non-NULL device pointer -- with a basis source attached nothing dereferences it; ldx = D passes the argument checks)
    a.X = Xd; a.ldx = D;
    a.rff_Xin = Xd; a.rff_ldxin = ldxin; a.rff_Omega = Od; a.rff_ldo = ldo; a.rff_phase = Pd; a.rff_scale = scale; a.rff_Din = (int)Din;
  } else {
    a.ldx = (D + 3) / 4 * 4;  // keeps every feature column 16-byte aligned for the LDS-DMA loader
    if ((rc = h->feat.reserve(h, (size_t)a.ldx * (size_t)std::max<int64_t>(N, 1) * sizeof(T)))) return rc;
    a.X = reinterpret_cast<T*>(h->feat.p);
  }
  // the rest of the arguments: the checks of the batched update on the device pointers, with its positions
  rc = posterior_check<T>(h, BLR_MEM_DEVICE, a.layout, 1, D, N, a.X, a.ldx, 0, a.y, 0, noise_kind, a.s, 0, prior_kind, a.mw, 0, a.Lw, ldl, 0,
                          a.mw_post, D, a.T_post, ldt, a.strideT, a.Lw_post, ldlp, a.strideLp, a.logpdf, a.info);
  if (rc) return rc;
  if (!fused && N > 0) {
    dim3 grid((unsigned)((D + kThreads - 1) / kThreads), (unsigned)((N + 31) / 32));  // 32 columns per workgroup (rff_features_kernel NT)
    hipLaunchKernelGGL(rff_features_kernel<T>, grid, dim3(kThreads), 0, h->stream, Xd, ldxin, Od, ldo, Pd, scale,
                       (int)Din, (int)D, (int)N, reinterpret_cast<T*>(h->feat.p), a.ldx);
    HIP_TRY(h, hipGetLastError());
  }
  if ((rc = posterior_run<T>(h, a))) return rc;
  return io.finish();
}


// ================================================================================================================
// Dense Sigma_y and full predictive covariance: see blr_dense.hpp for the scheme
// ================================================================================================================
constexpr int64_t kMaxDenseN = 16384;  // N x N work matrices: 2 GiB in fp64 at this size

// x_n' mw for D <= 128 (one thread per input; the mean of mean_and_cov -- N <= 16384, not a hot path)
template <typename T>
__global__ __launch_bounds__(kThreads) void mean_small_kernel(const T* __restrict__ X, int64_t ldx, int layout, const T* __restrict__ mw, int D,
                                                              int N, T* __restrict__ mean) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  double acc = 0.0;
  for (int d = 0; d < D; ++d)
    acc += (double)((layout == LAYOUT_COLVECS) ? X[(int64_t)n * ldx + d] : X[(int64_t)d * ldx + n]) * (double)mw[d];
  mean[n] = (T)acc;
}

// Sigma_y = L L' in the top NP x NP block of M (lower, unit padding), R extra rows carried through; info_dev: status
template <typename T>
int chol_noise(blr_handle* h, const T* Sy_dev, int64_t ldsy, int N, int NP, int R, T* M, int64_t ld, int32_t* info_dev) {
  HIP_TRY(h, hipMemsetAsync(info_dev, 0, sizeof(int32_t), h->stream));
  hipLaunchKernelGGL(prior_copy_kernel<T>, dim3(2048), dim3(kThreads), 0, h->stream, Sy_dev, ldsy, N, NP, M, ld);
  return chol_large<T>(h, M, ld, NP, NP + R, info_dev);
}

template <typename T>
int posterior_dense_noise(blr_handle* h, int memspace, int layout, int64_t D64, int64_t N64, const T* X, int64_t ldx, const T* y,
                          const T* Sy, int64_t ldsy, int prior_kind, const T* mw, const T* Lw, int64_t ldl, T* mw_post, T* T_post,
                          int64_t ldt, T* Lw_post, int64_t ldlp, double* logpdf, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (D64 < 1 || D64 > kMaxLargeD) return bad_arg(h, 4, "D out of range for this build (1..8192)");
  if (N64 < 1 || N64 > kMaxDenseN) return bad_arg(h, 5, "N out of range for a dense noise covariance (1..16384)");
  if (!X) return bad_arg(h, 6, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D64 : ldx < N64) return bad_arg(h, 7, "ldx too small");
  if (!y) return bad_arg(h, 8, "y is NULL (reference :74 length check)");
  if (!Sy) return bad_arg(h, 9, "Sy is NULL");
  if (ldsy < N64) return bad_arg(h, 10, "ldsy < N");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 11, "prior_kind");
  if (!mw) return bad_arg(h, 12, "mw is NULL");
  if (!Lw) return bad_arg(h, 13, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D64) return bad_arg(h, 14, "ldl < D");
  if (T_post && ldt < D64) return bad_arg(h, 17, "ldt < D");
  if (Lw_post && ldlp < D64) return bad_arg(h, 19, "ldlp < D");
  if (!info) return bad_arg(h, 21, "info is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  const int D = (int)D64, N = (int)N64;
  const int NP = (N + kPB - 1) / kPB * kPB;
  const int R = (D + 1 + kPB - 1) / kPB * kPB;  // X rows + the y row, padded to whole TRSM row blocks
  const int64_t ld = (int64_t)NP + R;
  CallIO io(h, memspace);
  int rc;
  const T *X_d = nullptr, *y_d = nullptr, *Sy_d = nullptr, *mw_d = nullptr, *Lw_d = nullptr;
  T *mwp_d = nullptr, *Tp_d = nullptr, *Lp_d = nullptr;
  double* lp_d = nullptr;
  int32_t* info_d = nullptr;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  if ((rc = io.in(X, x_one, &X_d))) return rc;
  if ((rc = io.in(y, (size_t)N, &y_d))) return rc;
  if ((rc = io.in(Sy, mat_extent(N, N, ldsy), &Sy_d))) return rc;
  if ((rc = io.in(mw, (size_t)D, &mw_d))) return rc;
  if ((rc = io.in(Lw, lw_one, &Lw_d))) return rc;
  if ((rc = io.out(mw_post, (size_t)D, &mwp_d))) return rc;
  if ((rc = io.out(T_post, mat_extent(D, D, ldt), &Tp_d))) return rc;
  if ((rc = io.out(Lw_post, mat_extent(D, D, ldlp), &Lp_d))) return rc;
  if ((rc = io.out(logpdf, (size_t)1, &lp_d))) return rc;
  if ((rc = io.out(info, (size_t)1, &info_d))) return rc;
  T *M = nullptr, *ytil = nullptr, *one = nullptr;
  double* logdet = nullptr;
  int32_t* noise_info = nullptr;
  if ((rc = io.tmp((size_t)ld * NP, &M))) return rc;
  if ((rc = io.tmp((size_t)N, &ytil))) return rc;
  if ((rc = io.tmp(1, &one))) return rc;
  if ((rc = io.tmp(1, &logdet))) return rc;
  if ((rc = io.tmp(1, &noise_info))) return rc;
  double* lp_tmp = lp_d;
  if (!lp_tmp && (rc = io.tmp(1, &lp_tmp))) return rc;
  const T one_h = T(1);
  HIP_TRY(h, hipMemcpyAsync(one, &one_h, sizeof(T), hipMemcpyHostToDevice, h->stream));
  // [Sigma_y; X; y'] -> [L; X L^-T; (L^-1 y)']   (reference :79, :81 outer solve, :82)
  hipLaunchKernelGGL(whiten_fill_kernel<T>, dim3(2048), dim3(kThreads), 0, h->stream, X_d, ldx, layout, y_d, D, N, NP, R, M, ld, NP);
  if ((rc = chol_noise<T>(h, Sy_d, ldsy, N, NP, R, M, ld, noise_info))) return rc;
  hipLaunchKernelGGL(logdet_kernel<T>, dim3(1), dim3(kThreads), 0, h->stream, (const T*)M, ld, N, logdet);
  hipLaunchKernelGGL(row_extract_kernel<T>, dim3(256), dim3(kThreads), 0, h->stream, (const T*)M, ld, NP + D, N, ytil);
  // the whitened problem: ColVecs X~ = rows NP .. NP+D of M (leading dimension ld), y~, unit isotropic noise
  PosteriorArgs<T> a{};
  a.X = M + NP; a.ldx = ld; a.strideX = 0; a.y = ytil; a.stridey = 0; a.s = one; a.strides = 0;
  a.mw = mw_d; a.stridemw = 0; a.Lw = Lw_d; a.ldl = ldl; a.strideLw = 0;
  a.mw_post = mwp_d; a.stride_mwpost = D; a.T_post = Tp_d; a.ldt = ldt; a.strideT = 0; a.Lw_post = Lp_d; a.ldlp = ldlp; a.strideLp = 0;
  a.logpdf = lp_tmp; a.info = info_d;
  a.layout = BLR_LAYOUT_COLVECS; a.noise_kind = BLR_NOISE_ISOTROPIC; a.prior_kind = prior_kind;
  a.D = D; a.N = N; a.B = 1;
  a.vec_ok = (D % Mfma<T>::VEC == 0 && aligned16(a.X, ld, (int64_t)0)) ? 1 : 0;
  // status precedence of the reference: the prior is factored first (:78), then Sigma_y (:79), then the posterior (:86).  The
  // inner update cannot tell a prior failure from a posterior one once the whitened data are garbage, so the prior's status
  // comes from an update on ZERO observations (A = Lw: D^3 / 3 flops, nothing next to the N^3 / 3 of the whitening)
  int32_t* prior_info = nullptr;
  if ((rc = io.tmp(1, &prior_info))) return rc;
  {
    PosteriorArgs<T> p0 = a;
    p0.N = 0; p0.mw_post = nullptr; p0.T_post = nullptr; p0.Lw_post = nullptr; p0.logpdf = nullptr; p0.info = prior_info;
    if ((rc = dispatch_posterior<T>(h, p0))) return rc;
  }
  if ((rc = dispatch_posterior<T>(h, a))) return rc;
  hipLaunchKernelGGL(dense_finish_kernel, dim3(1), dim3(64), 0, h->stream, lp_tmp, info_d, (const double*)logdet, (const int32_t*)noise_info,
                     (const int32_t*)prior_info);
  HIP_TRY(h, hipGetLastError());
  return io.finish();  // (drains the stream in either memspace: the temporaries are freed on return)
}

// Y = X' Lw^-T (N rows x D columns, column-major with leading dimension ldy, rows [DP, DP + NP) of Ybar) for a factored or
// dense prior: the tall-matrix panel sweep of the marginal path, keeping Y instead of folding it into row sums.
template <typename T>
int tall_solve_rows(blr_handle* h, int layout, int D, int N, const T* X, int64_t ldx, int prior_kind, const T* Lw, int64_t ldl,
                    T* Ybar, int64_t ldy, int DP, int NP, int32_t* info_dev) {
  int rc;
  HIP_TRY(h, hipMemsetAsync(info_dev, 0, sizeof(int32_t), h->stream));
  {
    MeanFillArgs<T> m{};
    m.X = X; m.ldx = ldx; m.layout = layout; m.mw = nullptr; m.mean = nullptr; m.Ybar = Ybar; m.ldy = ldy; m.row0 = DP;
    m.D = D; m.DP = DP; m.N = N;
    hipLaunchKernelGGL(mean_fill_kernel<T>, dim3((unsigned)(NP / 64)), dim3(kThreads), 0, h->stream, m);
  }
  if ((rc = tall_top_block<T>(h, prior_kind, Lw, ldl, D, DP, Ybar, ldy, info_dev))) return rc;
  const TallSweep<T> sweep{h, Ybar, ldy, DP, NP, info_dev, 1, 0};
  if ((rc = sweep.prepare())) return rc;
  sweep.forward(RowSqArgs<T>{});
  HIP_TRY(h, hipGetLastError());
  return 0;
}

// The temporaries of one N x N covariance at padded sizes (mean_and_cov_core): the tall matrix, the Gram tiles, a scalar
template <typename T>
struct CovTemps {
  T *Ybar = nullptr, *Gpart = nullptr;
  double* scratch = nullptr;
  int reserve(CallIO& io, int D, int N) {
    const int DP = (D + kPB - 1) / kPB * kPB, NP = (N + kPB - 1) / kPB * kPB;
    const int nb = NP / kPB, ntiles = nb * (nb + 1) / 2;
    int rc;
    if ((rc = io.tmp((size_t)((int64_t)DP + NP) * DP, &Ybar))) return rc;
    if ((rc = io.tmp((size_t)ntiles * kPB * kPB, &Gpart))) return rc;
    return io.tmp(1, &scratch);
  }
};

// mean and covariance of ONE regressor on device operands: what blr_mean_and_cov_* launches, and the D > 128 route of
// blr_mean_and_cov_batched_* one regressor after the other.  Enqueues only.
template <typename T>
int mean_and_cov_core(blr_handle* h, const CovTemps<T>& t, int layout, int D, int N, const T* X_d, int64_t ldx, int noise_kind, const T* s_d,
                      int64_t lds, int prior_kind, const T* mw_d, const T* Lw_d, int64_t ldl, T* mean_d, T* C_d, int64_t ldc, int32_t* info_d) {
  const int DP = (D + kPB - 1) / kPB * kPB, NP = (N + kPB - 1) / kPB * kPB;
  const int64_t ldy = (int64_t)DP + NP;
  const int nb = NP / kPB, ntiles = nb * (nb + 1) / 2;
  T *const Ybar = t.Ybar, *const Gpart = t.Gpart;
  double* const scratch = t.scratch;
  const T* const mean = mean_d;
  int rc;
  // ---- Y = alpha' = X' Uw^-1   (reference :36 alpha = Uw' \ X)
  if (prior_kind == BLR_PRIOR_DIAGONAL) {
    hipLaunchKernelGGL(prior_diag_kernel<T>, dim3(1), dim3(kThreads), 0, h->stream, Lw_d, (int64_t)1, prior_kind, D, scratch, info_d);
    hipLaunchKernelGGL(diag_prior_rows_kernel<T>, dim3(2048), dim3(kThreads), 0, h->stream, X_d, ldx, layout, Lw_d, D, N, NP, DP, Ybar + DP, ldy);
  } else {
    if ((rc = tall_solve_rows<T>(h, layout, D, N, X_d, ldx, prior_kind, Lw_d, ldl, Ybar, ldy, DP, NP, info_d))) return rc;
  }
  // ---- Y Y' by the Gram kernel with the roles swapped: NP "rows", D "observations" (columns of Y are contiguous)
  {
    using LC = LargeCfg<T>;
    if ((rc = set_lds_once(h, gram_tile_kernel<T>, (size_t)LC::LDS_BYTES))) return rc;
    GramTileArgs<T> g{};
    g.X = Ybar + DP; g.ldx = ldy; g.layout = LAYOUT_COLVECS; g.use_dma = 1;
    g.s = nullptr; g.noise_kind = NOISE_ISOTROPIC; g.r = nullptr;
    g.D = NP; g.n_begin = 0; g.n_end = DP; g.nsplit = 1;
    g.tile_i0 = 0; g.tile_j0 = 0; g.tri = 1; g.ntiles = ntiles; g.nblocks = nb;
    g.Gpart = Gpart; g.bpart = nullptr; g.mode_out = 0; g.xcd_swizzle = 0;
    hipLaunchKernelGGL(gram_tile_kernel<T>, dim3(ntiles), dim3(kThreads), LC::LDS_BYTES, h->stream, g);
    hipLaunchKernelGGL(cov_assemble_kernel<T>, dim3(ntiles, 16), dim3(kThreads), 0, h->stream, (const T*)Gpart, ntiles, N, noise_kind, s_d,
                       lds, C_d, ldc);
  }
  // ---- mean = X' mw   (reference :33)
  if (mean)
    hipLaunchKernelGGL(mean_small_kernel<T>, dim3((unsigned)((N + 255) / 256)), dim3(kThreads), 0, h->stream, X_d, ldx, layout, mw_d, D, N, mean_d);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

template <typename T>
int mean_and_cov(blr_handle* h, int memspace, int layout, int64_t D64, int64_t N64, const T* X, int64_t ldx, int noise_kind, const T* s,
                 int64_t lds, int prior_kind, const T* mw, const T* Lw, int64_t ldl, T* mean, T* C, int64_t ldc, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (D64 < 1 || D64 > kMaxLargeD) return bad_arg(h, 4, "D out of range for this build (1..8192)");
  if (N64 < 1 || N64 > kMaxDenseN) return bad_arg(h, 5, "N out of range for an N x N covariance (1..16384)");
  if (!X) return bad_arg(h, 6, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D64 : ldx < N64) return bad_arg(h, 7, "ldx too small");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL && noise_kind != BLR_NOISE_DENSE) return bad_arg(h, 8, "noise_kind");
  if (!s) return bad_arg(h, 9, "s is NULL");
  if (noise_kind == BLR_NOISE_DENSE && lds < N64) return bad_arg(h, 10, "lds < N");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 11, "prior_kind");
  if (mean && !mw) return bad_arg(h, 12, "mw is NULL");
  if (!Lw) return bad_arg(h, 13, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D64) return bad_arg(h, 14, "ldl < D");
  if (!C) return bad_arg(h, 16, "C is NULL");
  if (ldc < N64) return bad_arg(h, 17, "ldc < N");
  if (!info) return bad_arg(h, 18, "info is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  const int D = (int)D64, N = (int)N64;
  CallIO io(h, memspace);
  int rc;
  const T *X_d = nullptr, *s_d = nullptr, *mw_d = nullptr, *Lw_d = nullptr;
  T *mean_d = nullptr, *C_d = nullptr;
  int32_t* info_d = nullptr;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  const size_t s_one = noise_kind == BLR_NOISE_DENSE ? mat_extent(N, N, lds) : (noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1);
  if ((rc = io.in(X, x_one, &X_d))) return rc;
  if ((rc = io.in(s, s_one, &s_d))) return rc;
  if ((rc = io.in(mw, (size_t)D, &mw_d))) return rc;
  if ((rc = io.in(Lw, lw_one, &Lw_d))) return rc;
  if ((rc = io.out(mean, (size_t)N, &mean_d))) return rc;
  if ((rc = io.out(C, mat_extent(N, N, ldc), &C_d))) return rc;
  if ((rc = io.out(info, (size_t)1, &info_d))) return rc;
  CovTemps<T> t;
  if ((rc = t.reserve(io, D, N))) return rc;
  if ((rc = mean_and_cov_core<T>(h, t, layout, D, N, X_d, ldx, noise_kind, s_d, lds, prior_kind, mw_d, Lw_d, ldl, mean_d, C_d, ldc, info_d))) return rc;
  return io.finish();  // (drains the stream in either memspace: the temporaries are freed on return)
}

// rand with a dense noise covariance: Y = X'(mw + Uw \ Z1) + Us' Z2   (reference :49-53).  Returns info (> 0: Sigma_y or Lw
// not positive definite).
template <typename T>
int rand_dense_noise(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const T* X, int64_t ldx, const T* Sy,
                     int64_t ldsy, int prior_kind, const T* mw, const T* Lw, int64_t ldl, const T* Z1, int64_t ldz1, const T* Z2,
                     int64_t ldz2, T* Y, int64_t ldy) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (N < 1 || N > kMaxDenseN) return bad_arg(h, 5, "N out of range for a dense noise covariance (1..16384)");
  if (!Sy) return bad_arg(h, 9, "Sy is NULL");
  if (ldsy < N) return bad_arg(h, 10, "ldsy < N");
  if (S < 0) return bad_arg(h, 6, "S < 0");
  if (S == 0) return 0;
  // X' W with the noise term switched off (sigma^2 = 0), through the ordinary entry point (validates everything else)
  const T zero = T(0);
  CallIO io(h, memspace);
  int rc;
  const T* zero_d = &zero;
  if (memspace == BLR_MEM_DEVICE) {
    T* z = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = io.tmp(1, &z))) return rc;
    HIP_TRY(h, hipMemsetAsync(z, 0, sizeof(T), h->stream));
    zero_d = z;
  }
  rc = rand_impl<T>(h, memspace, layout, D, N, S, X, ldx, BLR_NOISE_ISOTROPIC, zero_d, prior_kind, mw, Lw, ldl, Z1, ldz1, Z2, ldz2, Y, ldy);
  if (rc) return rc;
  // + L Z2 with L L' = Sigma_y
  const int NP = (int)((N + kPB - 1) / kPB * kPB);
  const T *Sy_d = nullptr, *Z2_d = nullptr;
  T* Y_d = nullptr;
  if ((rc = io.in(Sy, mat_extent(N, N, ldsy), &Sy_d))) return rc;
  if ((rc = io.in(Z2, mat_extent(N, S, ldz2), &Z2_d))) return rc;
  if ((rc = io.out(Y, mat_extent(N, S, ldy), &Y_d))) return rc;  // copies the X'W part back in
  T* M = nullptr;
  int32_t* ninfo = nullptr;
  if ((rc = io.tmp((size_t)NP * NP, &M))) return rc;
  if ((rc = io.tmp(1, &ninfo))) return rc;
  if ((rc = chol_noise<T>(h, Sy_d, ldsy, (int)N, NP, 0, M, (int64_t)NP, ninfo))) return rc;
  dim3 grid((unsigned)((N + 63) / 64), (unsigned)((S + 15) / 16));
  hipLaunchKernelGGL(lower_mult_add_kernel<T>, grid, dim3(kThreads), 0, h->stream, (const T*)M, (int64_t)NP, (int)N, Z2_d, ldz2, Y_d, ldy, S);
  HIP_TRY(h, hipGetLastError());
  int32_t hinfo = 0;
  HIP_TRY(h, hipMemcpyAsync(&hinfo, ninfo, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if ((rc = io.finish())) return rc;  // (drains the stream in either memspace: hinfo, the temporaries)
  return hinfo;
}

// ---- rank-k update / downdate of a resident state (blr_update.hpp, blr_downdate.hpp) -----------------------------------------
// What blr_update_factor_* (on its sweep route) and blr_downdate_factor_* share behind their own checks of the shape: the checks
// of the operands (positions 7 .. 21; `noise_msg`: the entry point's words for a noise kind it does not take), the device and
// the kernels' argument record ...
template <typename T>
int sweep_begin(blr_handle* h, SweepArgs<T>& a, int layout, int64_t B, int64_t D, int64_t k, const T* X, int64_t ldx, int64_t strideX,
                const T* y, int64_t stridey, int noise_kind, const char* noise_msg, const T* s, int64_t strides, T* mw, int64_t stridemw,
                T* Tf, int64_t ldt, int64_t strideT, int32_t* info) {
  if (k > 0 && !X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(k, 1)) return bad_arg(h, 8, "ldx too small");
  if (strideX < 0) return bad_arg(h, 9, "strideX < 0");
  if (k > 0 && !y) return bad_arg(h, 10, "y is NULL (reference :74 length check)");
  if (stridey < 0) return bad_arg(h, 11, "stridey < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL) return bad_arg(h, 12, noise_msg);
  if (!s) return bad_arg(h, 13, "s is NULL");
  if (strides < 0) return bad_arg(h, 14, "strides < 0");
  if (!mw) return bad_arg(h, 15, "mw is NULL");
  if (B > 1 && stridemw < D) return bad_arg(h, 16, "stridemw < D");
  if (!Tf) return bad_arg(h, 17, "T is NULL");
  if (ldt < D) return bad_arg(h, 18, "ldt < D");
  if (B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 19, "strideT too small");
  if (!info) return bad_arg(h, 21, "info is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  a.ldx = ldx; a.strideX = strideX; a.layout = layout; a.stridey = stridey; a.strides = strides; a.noise_kind = noise_kind;
  a.stridemw = stridemw; a.ldt = ldt; a.strideT = strideT; a.D = (int)D; a.k = (int)k;
  return 0;
}
// ... and the operands staged through `io` (the state is updated in place), with the k = 0 pointer fix-up
template <typename T>
int sweep_stage(CallIO& io, SweepArgs<T>& a, int64_t B, const T* X, const T* y, const T* s, T* mw, T* Tf, double* logpdf, int32_t* info) {
  const int64_t D = a.D, k = a.k;
  const size_t x_one = a.layout == BLR_LAYOUT_COLVECS ? mat_extent(D, k, a.ldx) : mat_extent(k, D, a.ldx);
  const size_t s_one = a.noise_kind == BLR_NOISE_DIAGONAL ? (size_t)k : 1;
  int rc;
  if ((rc = io.in(X, extent(B, a.strideX, x_one), &a.X))) return rc;
  if ((rc = io.in(y, extent(B, a.stridey, (size_t)k), &a.y))) return rc;
  if ((rc = io.in(s, extent(B, a.strides, s_one), &a.s))) return rc;
  if ((rc = io.out(mw, extent(B, a.stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.out(Tf, extent(B, a.strideT, mat_extent(D, D, a.ldt)), &a.Tf))) return rc;
  if ((rc = io.out(logpdf, (size_t)B, &a.logpdf))) return rc;
  if ((rc = io.out(info, (size_t)B, &a.info))) return rc;
  if (k == 0) { if (!a.X) a.X = a.mw; if (!a.y) a.y = a.mw; }
  return 0;
}

template <typename T>
int update_factor(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, const T* X, int64_t ldx,
                  int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s, int64_t strides, T* mw,
                  int64_t stridemw, T* Tf, int64_t ldt, int64_t strideT, double* logpdf, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  // Route (measured, tools/update_bench.py): a sweep costs ~40 us per observation at D = 128 (a serial chain
  // of D rotations), the in-place re-factorisation ~90 us per CALL whatever k is (45 us at D = 64, where batches run on the
  // one-wave-per-regressor kernel at 27 M updates/s) -- the sweep wins for a single new observation, except in large
  // batches at D <= 64.  A blocked (Householder) sweep that eliminates up to 16 rows in one chain of D reflections was built
  // and measured in round 3: 92 / 115 / 144 / 205 us at k = 1 / 3 / 8 / 16 against 90 us -- the k + 1-term dot products and
  // three reciprocal chains per step cost more than the rotations they replace -- and was not kept.
  // BLR_MI355X_SWEEP=always / never overrides (tests exercise both routes on the same inputs).
  const int mode = h->opt.sweep;
  const bool can_sweep = D >= 1 && D <= kSweepMaxD && k >= 0 && k <= kSweepMaxK;
  bool sweep = can_sweep && k <= 1 && (D > 64 || B < 256);
  if (mode == 1) sweep = can_sweep;
  if (mode == 2) sweep = false;
  if (!sweep) {
    // k-independent cost: the SAME state re-factored in place, the old factor entering as D pseudo-observations
    // (reads of T and mw complete before the first write in both the fused and the large-D path)
    if (!mw) return bad_arg(h, 15, "mw is NULL");
    if (!Tf) return bad_arg(h, 17, "T is NULL");
    return posterior_batched<T>(h, memspace, layout, B, D, k, X, ldx, strideX, y, stridey, noise_kind, s, strides,
                                BLR_PRIOR_UPPER_FACTOR, mw, stridemw, Tf, ldt, strideT, mw, stridemw, Tf, ldt, strideT,
                                (T*)nullptr, 0, 0, logpdf, info);
  }
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (B == 0) return 0;
  SweepArgs<T> a{};
  int rc = sweep_begin<T>(h, a, layout, B, D, k, X, ldx, strideX, y, stridey, noise_kind, "noise_kind", s, strides, mw, stridemw, Tf, ldt,
                          strideT, info);
  if (rc) return rc;
  const int lds = sweep_lds_bytes<T>((int)D);
  if ((rc = set_lds_once(h, rank1_sweep_kernel<T>, (size_t)(lds)))) return rc;
  CallIO io(h, memspace);
  if ((rc = sweep_stage<T>(io, a, B, X, y, s, mw, Tf, logpdf, info))) return rc;
  hipLaunchKernelGGL(rank1_sweep_kernel<T>, dim3((unsigned)B), dim3(kThreads), lds, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- rank-k downdate of a resident state (blr_downdate.hpp) -----------------------------------------------------------
constexpr size_t kDowndateWorkspace = (size_t)2 << 30;  // bound of the global route's per-chunk workspace (at least one regressor)

template <typename T>
int downdate_launch(blr_handle* h, const SweepArgs<T>& a0, int64_t B) {
  const int D = a0.D;
  if (D <= kDowndateLdsMaxD && !h->opt.no_downdate_lds) {
    const int lds = downdate_lds_bytes<T>(D);
    if (const int rc_lds = set_lds_once(h, downdate_lds_kernel<T>, (size_t)lds)) return rc_lds;
    hipLaunchKernelGGL(downdate_lds_kernel<T>, dim3((unsigned)B), dim3(kThreads), lds, h->stream, a0);
    HIP_TRY(h, hipGetLastError());
    return 0;
  }
  // global route: chunks of regressors, each with a row-major copy of its factor and the per-observation vectors
  const size_t item = sizeof(T), vec = ((size_t)D * item + 255) & ~(size_t)255, mat = ((size_t)D * D * item + 255) & ~(size_t)255;
  const size_t per = mat + 3 * vec + 4 * sizeof(double) + sizeof(int);
  const int64_t chunk = h->cap_chunk(std::max<int64_t>(1, std::min<int64_t>(B, (int64_t)(kDowndateWorkspace / per))));
  h->count_chunks(B, chunk);
  const size_t off_v = (size_t)chunk * mat, off_sc = off_v + 3 * (size_t)chunk * vec, off_st = off_sc + (size_t)chunk * 4 * sizeof(double);
  int rc = h->ws.reserve(h, off_st + (size_t)chunk * sizeof(int) + 256, blr_handle::kWsFloor);
  if (rc) return rc;
  char* base = h->ws.p;
  DowndateWs<T> w{};
  w.W = reinterpret_cast<T*>(base);
  w.strideW = (int64_t)(mat / item);
  w.stridev = (int64_t)(vec / item);
  w.u = reinterpret_cast<T*>(base + off_v);
  w.cs = w.u + chunk * w.stridev;
  w.sn = w.cs + chunk * w.stridev;
  w.sc = reinterpret_cast<double*>(base + off_sc);
  w.st = reinterpret_cast<int*>(base + off_st);
  const int nt = (D + kDdTile - 1) / kDdTile;
  const int solve_lds = downdate_g_solve_lds<T>(D), finish_lds = downdate_g_finish_lds<T>(D);
  if (const int rc_lds = set_lds_once(h, downdate_g_solve_kernel<T>, (size_t)solve_lds)) return rc_lds;
  if (const int rc_lds = set_lds_once(h, downdate_g_finish_kernel<T>, (size_t)finish_lds)) return rc_lds;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const unsigned nb = (unsigned)std::min<int64_t>(chunk, B - b0);
    SweepArgs<T> a = a0;
    a.X += b0 * a.strideX; a.y += b0 * a.stridey; a.s += b0 * a.strides;
    a.mw += b0 * a.stridemw; a.Tf += b0 * a.strideT;
    if (a.logpdf) a.logpdf += b0;
    a.info += b0;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(downdate_g_copy_kernel<T, true>), dim3(nb, (unsigned)(nt * nt)), dim3(kThreads), 0, h->stream, a, w);
    hipLaunchKernelGGL(downdate_g_prep_kernel<T>, dim3(nb), dim3(kThreads), 0, h->stream, a, w);
    for (int i = 0; i < a.k; ++i) {
      hipLaunchKernelGGL(downdate_g_solve_kernel<T>, dim3(nb), dim3(kThreads), solve_lds, h->stream, a, w, i);
      hipLaunchKernelGGL(downdate_g_apply_kernel<T>, dim3(nb, (unsigned)((D + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, a, w);
    }
    hipLaunchKernelGGL(downdate_g_finish_kernel<T>, dim3(nb), dim3(kThreads), finish_lds, h->stream, a, w);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(downdate_g_copy_kernel<T, false>), dim3(nb, (unsigned)(nt * nt)), dim3(kThreads), 0, h->stream, a, w);
    HIP_TRY(h, hipGetLastError());
  }
  return 0;
}

template <typename T>
int downdate_factor(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, const T* X, int64_t ldx,
                    int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s, int64_t strides, T* mw,
                    int64_t stridemw, T* Tf, int64_t ldt, int64_t strideT, double* logpdf, int32_t* info) {
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > 8192) return bad_arg(h, 5, "D out of range (1..8192)");
  if (k < 0 || k > (1 << 30)) return bad_arg(h, 6, "k out of range (0..2^30)");
  if (B == 0) return 0;
  SweepArgs<T> a{};
  int rc = sweep_begin<T>(h, a, layout, B, D, k, X, ldx, strideX, y, stridey, noise_kind, "noise_kind (dense noise is not downdated)", s,
                          strides, mw, stridemw, Tf, ldt, strideT, info);
  if (rc) return rc;
  CallIO io(h, memspace);
  if ((rc = sweep_stage<T>(io, a, B, X, y, s, mw, Tf, logpdf, info))) return rc;
  if ((rc = downdate_launch<T>(h, a, B))) return rc;
  return io.finish();
}

// ---- exact leave-one-out predictives of a state's observations (blr_loo.hpp) -------------------------------------------------
constexpr size_t kLooWorkspace = (size_t)256 << 20;  // bound of the per-chunk intermediates (at least one regressor)

// ---- what the held-out entry points share behind their own argument checks (blr_loo_*, blr_kfold_*) ----
// Status of every state: loo_check_kernel, at most 65535 regressors per launch (grid.x; the empty totals' launches too).  Returns that
// chunk; the caller asks for the launches' error.
template <typename T>
int64_t heldout_status(blr_handle* h, int64_t B, int64_t D, int64_t N, const T* Tf, int64_t ldt, int64_t strideT, const T* s, int64_t strides,
                       int noise_kind, int32_t* info) {
  const int64_t ychunk = h->cap_chunk(65535);
  for (int64_t b0 = 0; b0 < B; b0 += ychunk)
    hipLaunchKernelGGL(loo_check_kernel<T>, dim3((unsigned)std::min<int64_t>(ychunk, B - b0)), dim3(kThreads), 0, h->stream, Tf + b0 * strideT,
                       ldt, strideT, (int)D, s + b0 * strides, strides, noise_kind, (int)N, info + b0);
  return ychunk;
}
// One operand of a held-out call: the caller's pointer, its leading dimension and stride per regressor, where the staged pointer goes
template <typename P>
struct HeldoutOp { P* p; int64_t ld, stride; P** dev; };
// The inputs staged through `io`: X, the N x S targets, s (no ld), the D x S mean(s) and T (a single column: S = 1, Y.ld = N,
// M.ld = D).  At N = 0 nothing of X, the targets and s is read ...
template <typename T>
int heldout_stage_in(CallIO& io, int layout, int noise_kind, int64_t B, int64_t D, int64_t N, int64_t S, HeldoutOp<const T> X, HeldoutOp<const T> Y,
                     HeldoutOp<const T> s, HeldoutOp<const T> M, HeldoutOp<const T> Tf) {
  const size_t x_one = N == 0 ? 0 : (layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, X.ld) : mat_extent(N, D, X.ld));
  const size_t s_one = N == 0 ? 0 : (noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1);
  int rc;
  if ((rc = io.in(X.p, x_one ? extent(B, X.stride, x_one) : 0, X.dev))) return rc;
  if ((rc = io.in(Y.p, N ? extent(B, Y.stride, mat_extent(N, S, Y.ld)) : 0, Y.dev))) return rc;
  if ((rc = io.in(s.p, s_one ? extent(B, s.stride, s_one) : 0, s.dev))) return rc;
  if ((rc = io.in(M.p, extent(B, M.stride, mat_extent(D, S, M.ld)), M.dev))) return rc;
  return io.in(Tf.p, extent(B, Tf.stride, mat_extent(D, D, Tf.ld)), Tf.dev);
}
// ... and the outputs: the N x S means, the N variances (no ld), the n_ll x S log densities, the S totals (no ld) and info (a single
// column: S = 1, mean.ld = N, ll.ld = n_ll, total.stride = 1)
template <typename T>
int heldout_stage_out(CallIO& io, int64_t B, int64_t N, int64_t S, int64_t n_ll, HeldoutOp<T> mean, HeldoutOp<T> var, HeldoutOp<double> ll,
                      HeldoutOp<double> total, int32_t* info, int32_t** info_d) {
  int rc;
  if ((rc = io.out(mean.p, N ? extent(B, mean.stride, mat_extent(N, S, mean.ld)) : 0, mean.dev))) return rc;
  if ((rc = io.out(var.p, N ? extent(B, var.stride, (size_t)N) : 0, var.dev))) return rc;
  if ((rc = io.out(ll.p, N ? extent(B, ll.stride, mat_extent(n_ll, S, ll.ld)) : 0, ll.dev))) return rc;
  if ((rc = io.out(total.p, extent(B, total.stride, (size_t)S), total.dev))) return rc;
  return io.out(info, (size_t)B, info_d);
}
// The totals need the log densities somewhere: wanted without them, the log densities go to workspace, S rows of n doubles per
// regressor, a row rounded up to `pad` bytes.
struct LogpdfSpill {
  const bool on;
  const int64_t ld;  // doubles per row
  const size_t per;  // bytes per regressor (0: no spill)
  LogpdfSpill(const double* total, const double* ll, int64_t n, int64_t S = 1, size_t pad = 256)
      : on(total && !ll), ld((int64_t)(((size_t)n * sizeof(double) + pad - 1) / pad * pad / sizeof(double))), per(on ? (size_t)S * ld * sizeof(double) : 0) {}
  // a chunk's rows at `base`, indexed by the global regressor as the outputs are (b0: the chunk's first)
  double* rows(char* base, int64_t b0) const { return reinterpret_cast<double*>(base) - b0 * (int64_t)(per / sizeof(double)); }
};
// Totals of regressors b0 .. b0 + nb - 1 over their n log densities (ll NULL, n = 0: empty sums): single-column states ...
inline void heldout_totals(blr_handle* h, int64_t b0, int64_t nb, const double* ll, int64_t stride_ll, int64_t n, double* total, const int32_t* info) {
  hipLaunchKernelGGL(loo_total_kernel, dim3((unsigned)nb), dim3(kThreads), 0, h->stream, ll, stride_ll, (int)n, total, info, (int)b0);
}
// ... and states of S columns
inline void heldout_cols_totals(blr_handle* h, int64_t b0, int64_t nb, int64_t S, const double* ll, int64_t ld_ll, int64_t stride_ll, int64_t n,
                                double* total, int64_t stride_t, const int32_t* info) {
  hipLaunchKernelGGL(loo_cols_total_kernel, dim3((unsigned)S, (unsigned)nb), dim3(kThreads), 0, h->stream, ll, ld_ll, stride_ll, (int)n, total,
                     stride_t, info, (int)b0);
}
// N = 0: empty sums, for the regressors whose state passed the check (cols: the totals are [S] per regressor, stride_t apart)
inline int heldout_empty_totals(blr_handle* h, int64_t B, int64_t ychunk, bool cols, int64_t S, double* total, int64_t stride_t, const int32_t* info) {
  for (int64_t b0 = 0; total && b0 < B; b0 += ychunk) {
    const int64_t nb = std::min<int64_t>(ychunk, B - b0);
    if (cols) heldout_cols_totals(h, b0, nb, S, nullptr, 0, 0, 0, total, stride_t, info);
    else heldout_totals(h, b0, nb, nullptr, 0, 0, total, info);
  }
  HIP_TRY(h, hipGetLastError());
  return 0;
}
// Regressors per launch: grid.y; the images if the route builds them; the rows of Z (z_one elements a regressor, 0: none) within
// 256 MiB; `per` bytes a regressor of the other intermediates (0: none) within kLooWorkspace -- at least one regressor
template <typename T>
int64_t whitened_chunk(const blr_handle* h, int64_t B, bool images, size_t z_one, size_t per) {
  int64_t chunk = std::min<int64_t>(B, 65535);
  if (images) chunk = std::min<int64_t>(chunk, MargImages<T>::kMaxChunk);
  if (z_one) chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / (z_one * sizeof(T)))));
  if (per) chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(kLooWorkspace / per)));
  return h->cap_chunk(chunk);
}
// The composed large-D route: a chunk's LATENT variance (the noise is the zero word at `zero`), with the mean if wanted, by whichever
// route blr_marginals_batched_* takes -- nested: no drain between the halves, its message dropped
template <typename T>
int heldout_latent_marginals(blr_handle* h, int layout, int64_t nb, int64_t D, int64_t N, const T* X, int64_t ldx, int64_t strideX, const T* zero,
                             const T* mw, int64_t stridemw, const T* Tf, int64_t ldt, int64_t strideT, T* mean, T* var, int64_t ldw, int32_t* inf) {
  int rc;
  {
    const AsyncScope no_drain(h, true);
    rc = marginals_batched<T>(h, BLR_MEM_DEVICE, layout, nb, D, N, X, ldx, strideX, BLR_NOISE_ISOTROPIC, zero, 0, BLR_PRIOR_UPPER_FACTOR, mw,
                              stridemw, Tf, ldt, strideT, mean, mean ? ldw : 0, var, ldw, inf);
  }
  if (!rc) h->err.clear();
  return rc;
}

// device operands; l carries y, s, the three outputs and info (global regressor indexing)
template <typename T>
int loo_launch(blr_handle* h, int layout, int64_t B, int64_t D, int64_t N, const T* X, int64_t ldx, int64_t strideX, LooArgs<T> l,
               const T* mw, int64_t stridemw, const T* Tf, int64_t ldt, int64_t strideT, double* total) {
  using MP = MargProduct<T, LooGemmArgs<T>>;
  int rc;
  if ((rc = ensure_stats(h))) return rc;
  l.degenerate = h->stats_dev + 3;
  int32_t* const info = const_cast<int32_t*>(l.info);
  const int64_t ychunk = heldout_status<T>(h, B, D, N, Tf, ldt, strideT, l.s, l.strides, l.noise_kind, info);
  HIP_TRY(h, hipGetLastError());
  // the route follows from the shape, as the marginals' does: the fused product stream at D = 128
  const bool fused = MP::takes(h, layout, D, N, X, ldx, strideX);
  const LogpdfSpill spill(total, l.ll, N);
  const size_t item = sizeof(T), row = ((size_t)N * item + 255) & ~(size_t)255;
  const size_t per = (fused ? 0 : 2 * row) + spill.per + sizeof(int32_t);
  int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(B, 65535), (int64_t)(kLooWorkspace / per)));
  if (fused) chunk = std::min<int64_t>(chunk, MP::kMaxChunk);
  chunk = h->cap_chunk(chunk);
  const size_t off_var = (size_t)chunk * row, off_ll = fused ? 0 : 2 * (size_t)chunk * row;
  const size_t off_zero = off_ll + (size_t)chunk * spill.per, off_inf = off_zero + 256;
  if (N > 0 && (rc = h->loo_ws.reserve(h, off_inf + (size_t)chunk * sizeof(int32_t) + 256))) return rc;
  char* const ws = h->loo_ws.p;
  const int64_t ldw = (int64_t)(row / item);
  if (N > 0 && !fused) HIP_TRY(h, hipMemsetAsync(ws + off_zero, 0, sizeof(T), h->stream));  // the composed route's zero noise
  if (N > 0 && fused && (rc = MP::prepare(h, layout, chunk))) return rc;
  for (int64_t b0 = 0; N > 0 && b0 < B; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, B - b0);
    LooArgs<T> lc = l;
    if (spill.on) { lc.ll = spill.rows(ws + off_ll, b0); lc.stride_ll = spill.ld; }
    if (fused) {
      LooGemmArgs<T> a{};
      a.X = X; a.ldx = ldx; a.strideX = strideX; a.s = l.s; a.strides = l.strides; a.mw = mw; a.stridemw = stridemw;
      a.info = l.info; a.layout = layout; a.noise_kind = l.noise_kind; a.prior_kind = BLR_PRIOR_UPPER_FACTOR;
      a.D = (int)D; a.N = (int)N; a.B = (int)B;
      a.l = lc;
      MP::launch(h, a, Tf, ldt, strideT, l.info, b0, nb);
    } else {
      // mean and LATENT variance (zero noise) by whichever marginal route the shape takes, then the epilogue
      T* const mean = reinterpret_cast<T*>(ws);
      T* const var = reinterpret_cast<T*>(ws + off_var);
      rc = heldout_latent_marginals<T>(h, layout, nb, D, N, X + b0 * strideX, ldx, strideX, reinterpret_cast<const T*>(ws + off_zero),
                                       mw + b0 * stridemw, stridemw, Tf + b0 * strideT, ldt, strideT, mean, var, ldw,
                                       reinterpret_cast<int32_t*>(ws + off_inf));
      if (rc) return rc;
      const int64_t gx = std::max<int64_t>(1, std::min<int64_t>((N + kThreads - 1) / kThreads, (4 * (int64_t)h->cus + nb - 1) / nb));
      hipLaunchKernelGGL(loo_finish_kernel<T>, dim3((unsigned)gx, (unsigned)nb), dim3(kThreads), 0, h->stream, lc, (const T*)mean,
                         (const T*)var, ldw, (int)b0);
    }
    if (total) heldout_totals(h, b0, nb, lc.ll, lc.stride_ll, N, total, l.info);
    HIP_TRY(h, hipGetLastError());
  }
  h->count_chunks(B, N > 0 ? chunk : ychunk);  // (after the loop: the composed route's marginals count their own)
  return N == 0 && total ? heldout_empty_totals(h, B, ychunk, false, 1, total, 1, l.info) : 0;
}

template <typename T>
int loo_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X, int64_t ldx, int64_t strideX,
                const T* y, int64_t stridey, int noise_kind, const T* s, int64_t strides, const T* mw, int64_t stridemw, const T* Tf,
                int64_t ldt, int64_t strideT, T* loo_mean, int64_t stride_lm, T* loo_var, int64_t stride_lv, double* loo_logpdf,
                int64_t stride_ll, double* loo_total, int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range (0..2^30)");
  if (N > 0 && !X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(N, 1)) return bad_arg(h, 8, "ldx too small");
  if (strideX < 0) return bad_arg(h, 9, "strideX < 0");
  if (N > 0 && !y) return bad_arg(h, 10, "y is NULL (reference :74 length check)");
  if (stridey < 0) return bad_arg(h, 11, "stridey < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 12, "noise_kind (dense noise has no single-observation LOO: that is a block LOO)");
  if (N > 0 && !s) return bad_arg(h, 13, "s is NULL");
  if (strides < 0) return bad_arg(h, 14, "strides < 0");
  if (!mw) return bad_arg(h, 15, "mw is NULL");
  if (B > 1 && stridemw < D) return bad_arg(h, 16, "stridemw < D");
  if (!Tf) return bad_arg(h, 17, "T is NULL");
  if (ldt < D) return bad_arg(h, 18, "ldt < D");
  if (B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 19, "strideT too small");
  if (loo_mean && B > 1 && stride_lm < N) return bad_arg(h, 21, "stride_lm < N");
  if (loo_var && B > 1 && stride_lv < N) return bad_arg(h, 23, "stride_lv < N");
  if (loo_logpdf && B > 1 && stride_ll < N) return bad_arg(h, 25, "stride_ll < N");
  if (!info) return bad_arg(h, 27, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  if (B == 0) return 0;
  HIP_TRY(h, hipSetDevice(h->device));
  LooArgs<T> l{};
  l.stridey = stridey; l.strides = strides; l.noise_kind = noise_kind; l.stride_lm = stride_lm; l.stride_lv = stride_lv;
  l.stride_ll = stride_ll; l.N = (int)N;
  CallIO io(h, memspace);
  int rc;
  const T *dX = nullptr, *dmw = nullptr, *dT = nullptr;
  double* dtot = nullptr;
  int32_t* dinfo = nullptr;
  if ((rc = heldout_stage_in<T>(io, layout, noise_kind, B, D, N, 1, {X, ldx, strideX, &dX}, {y, N, stridey, &l.y}, {s, 0, strides, &l.s},
                                {mw, D, stridemw, &dmw}, {Tf, ldt, strideT, &dT}))) return rc;
  if ((rc = heldout_stage_out<T>(io, B, N, 1, N, {loo_mean, N, stride_lm, &l.lm}, {loo_var, 0, stride_lv, &l.lv}, {loo_logpdf, N, stride_ll, &l.ll},
                                 {loo_total, 0, 1, &dtot}, info, &dinfo))) return rc;
  l.info = dinfo;
  if ((rc = loo_launch<T>(h, layout, B, D, N, dX, ldx, strideX, l, dmw, stridemw, dT, ldt, strideT, dtot))) return rc;
  return io.finish();
}

// ---- evidence over a grid of (prior scale, noise scale) settings (blr_grid.hpp) --------------------------------------------------
template <typename T, int NB, int MODE>
int launch_grid_stats(blr_handle* h, const GridArgs<T>& a) {
  using C = SmallCfg<T, NB>;
  auto kern = grid_stats_kernel<T, NB, MODE>;
  if (const int rc_lds = set_lds_once(h, kern, (size_t)C::LDS_BYTES)) return rc_lds;
  hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)a.B * a.S)), dim3(kThreads), C::LDS_BYTES, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

// grid_prior_kernel<T, nb> over p.B regressors (it reads the prior's fields of p and writes prior_info / prior_logdet): the one place
// that launches it, for blr_logpdf_grid_* (nb known at compile time: NB = nb) and blr_logpdf_grid_ragged_* (nb at run time)
template <typename T, int NB = 1>
int grid_prior_enqueue(blr_handle* h, int nb, const GridArgs<T>& p) {
  if constexpr (NB < 8) if (nb != NB) return grid_prior_enqueue<T, NB + 1>(h, nb, p);
  using C = SmallCfg<T, NB>;
  if (const int rc = set_lds_once(h, grid_prior_kernel<T, NB>, (size_t)C::LDS_BYTES)) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(grid_prior_kernel<T, NB>), dim3((unsigned)p.B), dim3(kThreads), C::LDS_BYTES, h->stream, p);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

// device operands, D <= 128: prior, statistics (+ reduce), settings, argmax, refit -- the same launches whatever B and G are
template <typename T, int NB>
int grid_small_nb(blr_handle* h, GridArgs<T> a, bool vec_ok) {
  using C = SmallCfg<T, NB>;
  constexpr int SZ = grid_stat_elems<T, NB>();
  int rc;
  Carve carve;
  const size_t nblk = (size_t)a.B * a.S;
  const size_t o_st = carve(nblk * SZ * sizeof(T)), o_sc = carve(nblk * 2 * sizeof(double)), o_bad = carve(nblk * sizeof(int32_t));
  const size_t o_pl = carve((size_t)a.B * sizeof(double)), o_pi = carve((size_t)a.B * sizeof(int32_t)), o_best = carve((size_t)a.B * sizeof(int64_t));
  if ((rc = h->loo_ws.reserve(h, carve.off))) return rc;
  char* const ws = h->loo_ws.p;
  a.stats = reinterpret_cast<T*>(ws + o_st); a.scal = reinterpret_cast<double*>(ws + o_sc); a.bad = reinterpret_cast<int32_t*>(ws + o_bad);
  a.prior_logdet = reinterpret_cast<double*>(ws + o_pl); a.prior_info = reinterpret_cast<int32_t*>(ws + o_pi);
  a.best = reinterpret_cast<int64_t*>(ws + o_best);
  if ((rc = set_lds_once(h, grid_eval_kernel<T, NB>, (size_t)C::LDS_BYTES))) return rc;
  if ((rc = grid_prior_enqueue<T, NB>(h, NB, a))) return rc;  // (every launch is checked before the ones that read its output are enqueued)
  if (a.layout == BLR_LAYOUT_ROWVECS) rc = launch_grid_stats<T, NB, 1>(h, a);
  else if (vec_ok) rc = launch_grid_stats<T, NB, 4>(h, a);
  else rc = launch_grid_stats<T, NB, 0>(h, a);
  if (rc) return rc;
  if (a.S > 1) {
    hipLaunchKernelGGL(grid_reduce_kernel<T>, dim3((unsigned)a.B, 8), dim3(kThreads), 0, h->stream, a, SZ);
    HIP_TRY(h, hipGetLastError());
  }
  a.refit = 0;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(grid_eval_kernel<T, NB>), dim3((unsigned)((int64_t)a.B * a.G)), dim3(kThreads), C::LDS_BYTES, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(grid_argmax_kernel, dim3((unsigned)((a.B + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream,
                     (const double*)a.logpdf, a.stride_lp, a.G, a.B, a.best, a.best_out);
  HIP_TRY(h, hipGetLastError());
  if (a.mw_best || a.T_best) {
    a.refit = 1;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(grid_eval_kernel<T, NB>), dim3((unsigned)a.B), dim3(kThreads), C::LDS_BYTES, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  return 0;
}

// D > 128: correct, not fast.  Per setting the scaled operands (grid_scale_kernel) go through the existing pipeline, all B regressors
// at once; then the argmax, and one more pass per regressor that has a winner.  Synchronises.
template <typename T>
int grid_large(blr_handle* h, GridArgs<T> a) {
  int rc;
  const int64_t B = a.B, D = a.D, N = a.N;
  const int64_t s_one = a.noise_kind == BLR_NOISE_DIAGONAL ? std::max<int64_t>(N, 1) : 1;
  const int64_t lw_one = a.prior_kind == BLR_PRIOR_DENSE ? D * D : D;
  Carve carve;
  const size_t o_s = carve((size_t)B * s_one * sizeof(T)), o_l = carve((size_t)B * lw_one * sizeof(T));
  const size_t o_lp = carve((size_t)B * sizeof(double)), o_in = carve((size_t)B * sizeof(int32_t)), o_best = carve((size_t)B * sizeof(int64_t));
  if ((rc = h->loo_ws.reserve(h, carve.off))) return rc;
  char* const ws = h->loo_ws.p;
  T* const s_g = reinterpret_cast<T*>(ws + o_s);
  T* const Lw_g = reinterpret_cast<T*>(ws + o_l);
  double* const lp_g = reinterpret_cast<double*>(ws + o_lp);
  int32_t* const in_g = reinterpret_cast<int32_t*>(ws + o_in);
  a.best = reinterpret_cast<int64_t*>(ws + o_best);
  const int64_t ldl_g = a.prior_kind == BLR_PRIOR_DENSE ? D : 0;
  for (int g = 0; g < a.G; ++g) {
    const int64_t chunk = h->cap_chunk(65535);  // grid.y <= 65535
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
      const int64_t nb = std::min<int64_t>(chunk, B - b0);
      hipLaunchKernelGGL(grid_scale_kernel<T>, dim3(64, (unsigned)nb), dim3(kThreads), 0, h->stream, a, b0, g, s_g + b0 * s_one, s_one,
                         Lw_g + b0 * lw_one, lw_one);
    }
    HIP_TRY(h, hipGetLastError());
    {
      const AsyncScope no_drain(h, true);
      rc = posterior_batched<T>(h, BLR_MEM_DEVICE, a.layout, B, D, N, a.X, a.ldx, a.strideX, a.y, a.stridey, a.noise_kind, s_g, s_one,
                                a.prior_kind, a.mw, a.stridemw, Lw_g, ldl_g, lw_one, (T*)nullptr, 0, (T*)nullptr, 0, 0, (T*)nullptr, 0, 0,
                                lp_g, in_g);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(grid_scatter_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream,
                       (const double*)lp_g, (const int32_t*)in_g, (int)B, g, a.logpdf, a.stride_lp, a.info, a.stride_info);
  }
  h->count_chunks(B, h->cap_chunk(65535));  // (the scaling launches; the nested updates counted their own)
  hipLaunchKernelGGL(grid_argmax_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream,
                     (const double*)a.logpdf, a.stride_lp, a.G, a.B, a.best, a.best_out);
  HIP_TRY(h, hipGetLastError());
  if (a.mw_best || a.T_best) {
    std::vector<int64_t> best((size_t)B);
    HIP_TRY(h, hipMemcpyAsync(best.data(), a.best, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int64_t b = 0; b < B; ++b) {
      if (best[(size_t)b] < 0) continue;  // nothing succeeded: mw_best / T_best stay as they are
      hipLaunchKernelGGL(grid_scale_kernel<T>, dim3(64, 1), dim3(kThreads), 0, h->stream, a, b, (int)best[(size_t)b], s_g, s_one, Lw_g, lw_one);
      const AsyncScope no_drain(h, true);
      rc = posterior_batched<T>(h, BLR_MEM_DEVICE, a.layout, 1, D, N, a.X + b * a.strideX, a.ldx, 0, a.y + b * a.stridey, 0, a.noise_kind,
                                s_g, 0, a.prior_kind, a.mw + b * a.stridemw, 0, Lw_g, ldl_g, 0,
                                a.mw_best ? a.mw_best + b * a.stride_mwbest : (T*)nullptr, 0, a.T_best ? a.T_best + b * a.strideT : (T*)nullptr,
                                a.ldt, 0, (T*)nullptr, 0, 0, lp_g, in_g);
      if (rc) return rc;
    }
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->err.clear();
  return 0;
}

template <typename T>
int grid_launch(blr_handle* h, const GridArgs<T>& a) {
  if (a.D > kMaxSmallD) return grid_large<T>(h, a);
  const bool vec_ok = a.layout == BLR_LAYOUT_COLVECS && a.D % Mfma<T>::VEC == 0 && aligned16(a.X, a.ldx, a.strideX);
  switch ((a.D + 15) / 16) {
    case 1: return grid_small_nb<T, 1>(h, a, vec_ok);
    case 2: return grid_small_nb<T, 2>(h, a, vec_ok);
    case 3: return grid_small_nb<T, 3>(h, a, vec_ok);
    case 4: return grid_small_nb<T, 4>(h, a, vec_ok);
    case 5: return grid_small_nb<T, 5>(h, a, vec_ok);
    case 6: return grid_small_nb<T, 6>(h, a, vec_ok);
    case 7: return grid_small_nb<T, 7>(h, a, vec_ok);
    default: return grid_small_nb<T, 8>(h, a, vec_ok);
  }
}

template <typename T>
int logpdf_grid(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X, int64_t ldx, int64_t strideX,
                const T* y, int64_t stridey, int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw, int64_t stridemw,
                const T* Lw, int64_t ldl, int64_t strideLw, int64_t G, const T* alpha, int64_t stride_alpha, const T* tau,
                int64_t stride_tau, double* logpdf, int64_t stride_lp, int64_t* best, T* mw_best, int64_t stride_mwbest, T* T_best,
                int64_t ldt, int64_t strideT, int32_t* info, int64_t stride_info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range (0..2^30)");
  if (N > 0 && !X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(N, 1)) return bad_arg(h, 8, "ldx too small");
  if (strideX < 0) return bad_arg(h, 9, "strideX < 0");
  if (N > 0 && !y) return bad_arg(h, 10, "y is NULL (reference :74 length check)");
  if (stridey < 0) return bad_arg(h, 11, "stridey < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 12, "noise_kind (the grid scales an isotropic or diagonal base noise; dense Sigma_y is not supported)");
  if (!s) return bad_arg(h, 13, "s is NULL");
  if (strides < 0) return bad_arg(h, 14, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 15, "prior_kind (dense or diagonal precision; pass a carried-forward factor as U'U)");
  if (!mw) return bad_arg(h, 16, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 17, "stridemw < 0");
  if (!Lw) return bad_arg(h, 18, "Lw is NULL");
  if (prior_kind == BLR_PRIOR_DENSE && ldl < D) return bad_arg(h, 19, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 20, "strideLw < 0");
  if (G < 0 || G > (1 << 20)) return bad_arg(h, 21, "G out of range (0..2^20)");
  if (alpha && stride_alpha != 0 && stride_alpha < G) return bad_arg(h, 23, "stride_alpha (0 = one grid for every regressor, else >= G)");
  if (tau && stride_tau != 0 && stride_tau < G) return bad_arg(h, 25, "stride_tau (0 = one grid for every regressor, else >= G)");
  if (G > 0 && !logpdf) return bad_arg(h, 26, "logpdf is NULL");
  if (stride_lp < G) return bad_arg(h, 27, "stride_lp < G");
  if (mw_best && B > 1 && stride_mwbest < D) return bad_arg(h, 30, "stride_mwbest < D");
  if (T_best && ldt < D) return bad_arg(h, 32, "ldt < D");
  if (T_best && B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 33, "strideT too small");
  if (G > 0 && !info) return bad_arg(h, 34, "info is NULL");
  if (stride_info < G) return bad_arg(h, 35, "stride_info < G");
  int S = 1, chunk = 64;
  if (D <= kMaxSmallD) grid_splits(N, &S, &chunk);
  // one workgroup of 256 threads per (regressor, setting) / (regressor, column block): a launch takes fewer than 2^32 threads
  if (B * std::max<int64_t>(G, S) >= ((int64_t)1 << 24)) return bad_arg(h, 21, "B * max(G, 8) too large (< 2^24)");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  if (B == 0 || G == 0) return 0;
  HIP_TRY(h, hipSetDevice(h->device));
  GridArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.stridey = stridey; a.strides = strides; a.stridemw = stridemw; a.ldl = ldl; a.strideLw = strideLw;
  a.stride_alpha = stride_alpha; a.stride_tau = stride_tau; a.stride_lp = stride_lp; a.stride_info = stride_info;
  a.stride_mwbest = stride_mwbest; a.ldt = ldt; a.strideT = strideT;
  a.layout = layout; a.noise_kind = noise_kind; a.prior_kind = prior_kind;
  a.D = (int)D; a.N = (int)N; a.B = (int)B; a.G = (int)G; a.S = S; a.chunk = chunk;
  CallIO io(h, memspace);
  const size_t x_one = N == 0 ? 0 : (layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx));
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  const size_t s_one = noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1;
  int rc;
  if ((rc = io.in(X, x_one ? extent(B, strideX, x_one) : 0, &a.X))) return rc;
  if ((rc = io.in(y, N ? extent(B, stridey, (size_t)N) : 0, &a.y))) return rc;
  if ((rc = io.in(s, std::max<size_t>(extent(B, strides, s_one), 1), &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &a.Lw))) return rc;
  if ((rc = io.in(alpha, extent(B, stride_alpha, (size_t)G), &a.alpha))) return rc;
  if ((rc = io.in(tau, extent(B, stride_tau, (size_t)G), &a.tau))) return rc;
  if ((rc = io.out(logpdf, extent(B, stride_lp, (size_t)G), &a.logpdf))) return rc;
  if ((rc = io.out(info, extent(B, stride_info, (size_t)G), &a.info))) return rc;
  if ((rc = io.out(best, (size_t)B, &a.best_out))) return rc;
  if ((rc = io.out(mw_best, extent(B, stride_mwbest, (size_t)D), &a.mw_best))) return rc;
  if ((rc = io.out(T_best, extent(B, strideT, mat_extent(D, D, ldt)), &a.T_best))) return rc;
  if (N == 0) { if (!a.X) a.X = a.mw; if (!a.y) a.y = a.mw; }
  if ((rc = grid_launch<T>(h, a))) return rc;
  return io.finish();
}

// ---- regressors with unequal observation counts (blr_ragged.hpp) ---------------------------------------------------
inline const void* ragged_kernel_ptr(double, int NB, int mode) { return ragged_kernel_ptr_f64(NB, mode); }
inline const void* ragged_kernel_ptr(float, int NB, int mode) { return ragged_kernel_ptr_f32(NB, mode); }
inline size_t ragged_kernel_lds(double, int NB) { return ragged_kernel_lds_f64(NB); }
inline size_t ragged_kernel_lds(float, int NB) { return ragged_kernel_lds_f32(NB); }
inline void ragged_kernel_launch(int NB, int mode, unsigned grid, hipStream_t st, const RaggedArgs<double>& a) { ragged_kernel_launch_f64(NB, mode, grid, st, a); }
inline void ragged_kernel_launch(int NB, int mode, unsigned grid, hipStream_t st, const RaggedArgs<float>& a) { ragged_kernel_launch_f32(NB, mode, grid, st, a); }

// ---- what the packed entry points share: blr_posterior_ragged_*, blr_marginals_ragged_*, blr_loo_ragged_*, blr_kfold_ragged_* ------
// offsets: what blr_posterior_ragged_* asks of it
inline int ragged_offsets_check(blr_handle* h, int64_t B, const int64_t* offsets) {
  if (B > 0 && !offsets) return bad_arg(h, 6, "offsets is NULL (a host array of B + 1 entries)");
  if (B > 0 && offsets[0] < 0) return bad_arg(h, 6, "offsets[0] < 0");
  for (int64_t b = 0; b < B; ++b) {
    if (offsets[b + 1] < offsets[b]) return bad_arg(h, 6, "offsets must be non-decreasing");
    if (offsets[b + 1] - offsets[b] > (1 << 30)) return bad_arg(h, 6, "a regressor with more than 2^30 observations");
  }
  return 0;
}

// The shape of a packed call, filled by ragged_front
struct RaggedFront {
  int64_t total = 0;                       // columns of the packed arrays
  bool any = false;                        // some regressor has an observation
  bool colv = false, diag = false;         // layout, noise kind
  size_t x_all = 0, n_all = 0, s_all = 0;  // elements of X, of a packed vector, of s (diagonal: n_all; isotropic: B entries at strides)
};
inline int no_check() { return 0; }
// The checks every packed entry point starts with, in the order of the arguments: memspace (2), layout, B, D, offsets (6), `mid` --
// what blr_kfold_ragged_* checks next --, then X and ldx at positions xpos and xpos + 1.  The noise kind and strides are the entry
// point's to check: `diag` and `s_all` mean something once it has.
template <typename T, typename Mid = int (*)()>
int ragged_front(blr_handle* h, RaggedFront& f, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, const T* X, int64_t ldx,
                 int noise_kind, int64_t strides, int xpos = 7, Mid mid = no_check, int64_t maxD = kMaxLargeD,
                 const char* d_text = "D out of range (1..8192)") {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > maxD) return bad_arg(h, 5, d_text);
  if (const int rc = ragged_offsets_check(h, B, offsets)) return rc;
  if (const int rc = mid()) return rc;
  f.total = B > 0 ? offsets[B] : 0;
  f.any = B > 0 && offsets[B] > offsets[0];
  f.colv = layout == BLR_LAYOUT_COLVECS;
  f.diag = noise_kind == BLR_NOISE_DIAGONAL;
  if (f.any && !X) return bad_arg(h, xpos, "X is NULL");
  if (f.colv ? ldx < D : ldx < std::max<int64_t>(f.total, 1)) return bad_arg(h, xpos + 1, "ldx too small");
  f.x_all = !f.any ? 0 : (f.colv ? mat_extent(D, f.total, ldx) : mat_extent(f.total, D, ldx));
  f.n_all = f.any ? (size_t)f.total : 0;
  f.s_all = f.diag ? f.n_all : (strides < 0 ? 0 : extent(B, strides, 1));
  return 0;
}

// The host tables of a packed call go one behind the other into the handle's metadata buffer; dev[k]: where spans[k] lies on the
// device.  The copy is ordered behind the work in flight and the stream is drained: the host image belongs to the handle and the
// next call rewrites it.
struct MetaSpan { const void* p; size_t bytes; };
template <size_t K>
int ragged_meta_upload(blr_handle* h, const MetaSpan (&spans)[K], const char* (&dev)[K]) {
  size_t bytes = 0;
  for (const MetaSpan& s : spans) bytes += s.bytes;
  h->ragged_host.resize((bytes + 7) / 8);
  char* const img = reinterpret_cast<char*>(h->ragged_host.data());
  size_t at = 0;
  for (const MetaSpan& s : spans) {
    if (s.bytes) std::memcpy(img + at, s.p, s.bytes);
    at += s.bytes;
  }
  if (const int rc = h->ragged_meta.reserve(h, bytes, (size_t)1 << 16)) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->ragged_meta.p, img, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  at = 0;
  for (size_t k = 0; k < K; ++k) {
    dev[k] = h->ragged_meta.p + at;
    at += spans[k].bytes;
  }
  return 0;
}
inline size_t ragged_table_bytes(int64_t B) { return (size_t)(B + 1) * sizeof(int64_t); }  // offsets and its kin

// D > 128: correct, not fast -- one regressor after the other through the equal-count entry point, `one(b, o, n)`: its call with
// B = 1 on the device operands of regressor b, whose n observations start at o.  Stops at the first failure (device pointers and
// in-range sizes: a HIP failure, not an argument index of the inner call); the call synchronises.
template <typename One>
int ragged_one_by_one(blr_handle* h, int64_t B, const int64_t* offsets, One one) {
  int rc = 0;
  {
    const AsyncScope drain(h, false);
    for (int64_t b = 0; b < B && rc == 0; ++b) rc = one(b, offsets[b], offsets[b + 1] - offsets[b]);
  }
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

// One launch of fused_ragged_kernel over the r.p.B regressors r.order lists (r.offsets, r.order: on the device); the kernel is only
// enqueued.  r.p.B is the length of the list and nothing else: the kernel indexes every array by the regressor it reads from the list.
template <typename T>
int ragged_enqueue(blr_handle* h, RaggedArgs<T>& r) {
  const int64_t B = r.p.B;
  int rc;
  const int NB = (r.p.D + 15) / 16;
  const bool vec_ok = r.p.layout == BLR_LAYOUT_COLVECS && r.p.D % Mfma<T>::VEC == 0 && aligned16(r.p.X, r.p.ldx, 0) && !h->opt.no_ldsdma;
  const int mode = r.p.layout == BLR_LAYOUT_ROWVECS ? 1 : (vec_ok ? 4 : 0);
  r.p.vec_ok = vec_ok ? 1 : 0;
  const void* const kern = ragged_kernel_ptr(T(0), NB, mode);
  if (!kern) return bad_arg(h, 5, "this build carries no unequal-count kernel for this D and element type (BLR_DEV_FAST)");
  if ((rc = set_lds_once(h, kern, ragged_kernel_lds(T(0), NB)))) return rc;
  ragged_kernel_launch(NB, mode, (unsigned)std::min<int64_t>(B, 1 << 20), h->stream, r);
  HIP_TRY(h, hipGetLastError());
  h->route_buf = std::string("fused_ragged_kernel<") + (sizeof(T) == 8 ? "double" : "float") + ", " + std::to_string(NB) + ", " + std::to_string(mode) + ">";
  h->route = h->route_buf.c_str();
  h->route_i8_B = 0;
  return 0;
}

// D <= 128: offsets and the longest-first order go to the handle's metadata buffer (ragged_meta_upload), then ONE launch
template <typename T>
int ragged_launch(blr_handle* h, RaggedArgs<T>& r, const int64_t* offsets) {
  const int64_t B = r.p.B;
  std::vector<int32_t> order((size_t)B);
  for (int64_t b = 0; b < B; ++b) order[(size_t)b] = (int32_t)b;
  std::stable_sort(order.begin(), order.end(), [offsets](int32_t i, int32_t j) { return offsets[i + 1] - offsets[i] > offsets[j + 1] - offsets[j]; });
  const char* dev[2];
  if (const int rc = ragged_meta_upload(h, {{offsets, ragged_table_bytes(B)}, {order.data(), (size_t)B * sizeof(int32_t)}}, dev)) return rc;
  r.offsets = reinterpret_cast<const int64_t*>(dev[0]);
  r.order = reinterpret_cast<const int32_t*>(dev[1]);
  return ragged_enqueue<T>(h, r);
}

template <typename T>
int posterior_ragged(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, const T* X, int64_t ldx,
                     const T* y, int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw, int64_t stridemw,
                     const T* Lw, int64_t ldl, int64_t strideLw, T* mw_post, int64_t stride_mwpost, T* T_post, int64_t ldt,
                     int64_t strideT, T* Lw_post, int64_t ldlp, int64_t strideLp, double* logpdf, int32_t* info) {
  RaggedFront f;
  if (const int rc = ragged_front(h, f, memspace, layout, B, D, offsets, X, ldx, noise_kind, strides)) return rc;
  const bool any = f.any, diag = f.diag;
  if (any && !y) return bad_arg(h, 9, "y is NULL (reference :74 length check)");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 10, "noise_kind (isotropic or diagonal; dense Sigma_y is not supported for unequal counts)");
  if (!s && (noise_kind == BLR_NOISE_ISOTROPIC || any)) return bad_arg(h, 11, "s is NULL");
  if (strides < 0) return bad_arg(h, 12, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 13, "prior_kind");
  if (!mw) return bad_arg(h, 14, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 15, "stridemw < 0");
  if (!Lw) return bad_arg(h, 16, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 17, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 18, "strideLw < 0");
  if (mw_post && B > 1 && stride_mwpost < D) return bad_arg(h, 20, "stride_mwpost < D");
  if (T_post && ldt < D) return bad_arg(h, 22, "ldt < D");
  if (T_post && B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 23, "strideT too small");
  if (Lw_post && ldlp < D) return bad_arg(h, 25, "ldlp < D");
  if (Lw_post && B > 1 && strideLp < (int64_t)mat_extent(D, D, ldlp)) return bad_arg(h, 26, "strideLp too small");
  if (B > 0 && !info) return bad_arg(h, 28, "info is NULL");
  if (B == 0) return 0;
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));
  RaggedArgs<T> r{};
  PosteriorArgs<T>& a = r.p;
  a.ldx = ldx; a.strides = diag ? 0 : strides; a.stridemw = stridemw; a.ldl = ldl; a.strideLw = strideLw;
  a.stride_mwpost = stride_mwpost; a.ldt = ldt; a.strideT = strideT; a.ldlp = ldlp; a.strideLp = strideLp;
  a.layout = layout; a.noise_kind = noise_kind; a.prior_kind = prior_kind;
  a.D = (int)D; a.B = (int)B;

  CallIO io(h, memspace);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  int rc;
  if ((rc = io.in(X, f.x_all, &a.X))) return rc;
  if ((rc = io.in(y, f.n_all, &a.y))) return rc;
  if ((rc = io.in(s, f.s_all, &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &a.Lw))) return rc;
  if ((rc = io.out(mw_post, extent(B, stride_mwpost, (size_t)D), &a.mw_post))) return rc;
  if ((rc = io.out(T_post, extent(B, strideT, mat_extent(D, D, ldt)), &a.T_post))) return rc;
  if ((rc = io.out(Lw_post, extent(B, strideLp, mat_extent(D, D, ldlp)), &a.Lw_post))) return rc;
  if ((rc = io.out(logpdf, (size_t)B, &a.logpdf))) return rc;
  if ((rc = io.out(info, (size_t)B, &a.info))) return rc;
  // no data at all (or, host memspace, nothing staged): the kernel never dereferences these, but keep the pointers valid
  if (!a.X) a.X = a.mw;
  if (!a.y) a.y = a.mw;
  if (!a.s) a.s = a.mw;
  if (D <= kMaxSmallD) {
    if ((rc = ragged_launch<T>(h, r, offsets))) return rc;
    return io.finish();
  }
  // D > 128: through the pipeline of blr_posterior_batched_*
  if ((rc = ragged_one_by_one(h, B, offsets, [&](int64_t b, int64_t o, int64_t n) {
         return posterior_batched<T>(h, BLR_MEM_DEVICE, layout, 1, D, n, a.X + (f.colv ? o * ldx : o), ldx, 0, a.y + o, 0, noise_kind,
                                     diag ? a.s + o : a.s + b * strides, 0, prior_kind, a.mw + b * stridemw, 0, a.Lw + b * strideLw, ldl, 0,
                                     a.mw_post ? a.mw_post + b * stride_mwpost : (T*)nullptr, 0, a.T_post ? a.T_post + b * strideT : (T*)nullptr,
                                     ldt, 0, a.Lw_post ? a.Lw_post + b * strideLp : (T*)nullptr, ldlp, 0,
                                     a.logpdf ? a.logpdf + b : (double*)nullptr, a.info + b);
       })))
    return rc;
  return io.finish();
}

// ---- evidence grid for regressors with unequal counts (blr_grid_ragged.hpp, blr_grid_ragged_plan.hpp) ---------------
static_assert(kEvidenceNoBad == kGridNoBad && kEvidencePriorNone == kGridPriorNone &&
                  evidence_stat_elems<double, 8>() == grid_stat_elems<double, 8>() && evidence_stat_elems<float, 3>() == grid_stat_elems<float, 3>(),
              "blr_grid_ragged.hpp repeats the constants of blr_grid.hpp");
#define BLR_EVIDENCE_PICK(NAME, RET)                                                                             \
  template <typename... A> inline RET NAME(double, A... a) { return NAME##_f64(a...); }                          \
  template <typename... A> inline RET NAME(float, A... a) { return NAME##_f32(a...); }
BLR_EVIDENCE_PICK(ragged_evidence_stats_ptr, const void*)
BLR_EVIDENCE_PICK(ragged_evidence_eval_ptr, const void*)
BLR_EVIDENCE_PICK(ragged_evidence_lds, size_t)
BLR_EVIDENCE_PICK(ragged_evidence_stat_elems, int)
#undef BLR_EVIDENCE_PICK
inline void ragged_evidence_stats_launch(int NB, int mode, unsigned grid, hipStream_t st, const RaggedEvidenceArgs<double>& a) { ragged_evidence_stats_launch_f64(NB, mode, grid, st, a); }
inline void ragged_evidence_stats_launch(int NB, int mode, unsigned grid, hipStream_t st, const RaggedEvidenceArgs<float>& a) { ragged_evidence_stats_launch_f32(NB, mode, grid, st, a); }
inline void ragged_evidence_reduce_launch(int NB, unsigned B, hipStream_t st, const RaggedEvidenceArgs<double>& a) { ragged_evidence_reduce_launch_f64(NB, B, st, a); }
inline void ragged_evidence_reduce_launch(int NB, unsigned B, hipStream_t st, const RaggedEvidenceArgs<float>& a) { ragged_evidence_reduce_launch_f32(NB, B, st, a); }
inline void ragged_evidence_eval_launch(int NB, unsigned grid, hipStream_t st, const RaggedEvidenceArgs<double>& a) { ragged_evidence_eval_launch_f64(NB, grid, st, a); }
inline void ragged_evidence_eval_launch(int NB, unsigned grid, hipStream_t st, const RaggedEvidenceArgs<float>& a) { ragged_evidence_eval_launch_f32(NB, grid, st, a); }

// device operands, D <= 128: the launches of grid_small_nb with the statistics pass over the plan's items.  The loader is picked as
// grid_launch picks it for B = 1 on a slice: every slice of an aligned X with an aligned ldx is aligned, whatever `offsets` holds.
template <typename T>
int grid_ragged_small(blr_handle* h, RaggedEvidenceArgs<T> a, const int64_t* offsets, int64_t* best_out) {
  const int64_t B = a.B;
  const int NB = (a.D + 15) / 16;
  const bool vec_ok = a.layout == BLR_LAYOUT_COLVECS && a.D % Mfma<T>::VEC == 0 && aligned16(a.X, a.ldx, 0);
  const int mode = a.layout == BLR_LAYOUT_ROWVECS ? 1 : (vec_ok ? 4 : 0);
  const void* const k_stats = ragged_evidence_stats_ptr(T(0), NB, mode);
  const void* const k_eval = ragged_evidence_eval_ptr(T(0), NB);
  if (!k_stats || !k_eval) return bad_arg(h, 5, "this build carries no unequal-count evidence kernel for this D and element type (BLR_DEV_FAST)");
  int rc;
  GridRaggedPlan plan;
  plan_grid_ragged(offsets, B, plan);
  const size_t SZ = (size_t)ragged_evidence_stat_elems(T(0), NB), lds = ragged_evidence_lds(T(0), NB);
  Carve carve;
  const size_t nblk = (size_t)plan.slots;
  const size_t o_st = carve(nblk * SZ * sizeof(T)), o_sc = carve(nblk * 2 * sizeof(double)), o_bad = carve(nblk * sizeof(int32_t));
  const size_t o_pl = carve((size_t)B * sizeof(double)), o_pi = carve((size_t)B * sizeof(int32_t)), o_best = carve((size_t)B * sizeof(int64_t));
  if ((rc = h->loo_ws.reserve(h, carve.off))) return rc;
  char* const ws = h->loo_ws.p;
  a.stats = reinterpret_cast<T*>(ws + o_st); a.scal = reinterpret_cast<double*>(ws + o_sc); a.bad = reinterpret_cast<int32_t*>(ws + o_bad);
  double* const prior_logdet = reinterpret_cast<double*>(ws + o_pl);
  int32_t* const prior_info = reinterpret_cast<int32_t*>(ws + o_pi);
  int64_t* const best = reinterpret_cast<int64_t*>(ws + o_best);
  a.prior_logdet = prior_logdet; a.prior_info = prior_info; a.best = best;
  const char* dev[3];
  if ((rc = ragged_meta_upload(h, {{offsets, ragged_table_bytes(B)}, {plan.items.data(), plan.items.size() * sizeof(GridRaggedItem)},
                                   {plan.slot0.data(), (size_t)(B + 1) * sizeof(int32_t)}}, dev)))
    return rc;
  a.offsets = reinterpret_cast<const int64_t*>(dev[0]);
  a.items = reinterpret_cast<const GridRaggedItem*>(dev[1]);
  a.slot0 = reinterpret_cast<const int32_t*>(dev[2]);
  if ((rc = set_lds_once(h, k_stats, lds))) return rc;
  if ((rc = set_lds_once(h, k_eval, lds))) return rc;
  GridArgs<T> p{};  // what grid_prior_kernel reads
  p.Lw = a.Lw; p.ldl = a.ldl; p.strideLw = a.strideLw; p.prior_kind = a.prior_kind; p.D = a.D; p.B = a.B;
  p.prior_logdet = prior_logdet; p.prior_info = prior_info;
  if ((rc = grid_prior_enqueue<T>(h, NB, p))) return rc;  // (every launch is checked before the ones that read its output are enqueued)
  ragged_evidence_stats_launch(NB, mode, (unsigned)plan.slots, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  if (plan.reduce) {
    ragged_evidence_reduce_launch(NB, (unsigned)B, h->stream, a);
    HIP_TRY(h, hipGetLastError());
  }
  a.refit = 0;
  ragged_evidence_eval_launch(NB, (unsigned)(B * a.G), h->stream, a);
  HIP_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(grid_argmax_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream,
                     (const double*)a.logpdf, a.stride_lp, a.G, a.B, best, best_out);
  HIP_TRY(h, hipGetLastError());
  if (a.mw_best || a.T_best) {
    a.refit = 1;
    ragged_evidence_eval_launch(NB, (unsigned)B, h->stream, a);
    HIP_TRY(h, hipGetLastError());
  }
  h->route_buf = std::string("ragged_evidence_stats_kernel<") + (sizeof(T) == 8 ? "double" : "float") + ", " + std::to_string(NB) + ", " + std::to_string(mode) + ">";
  h->route = h->route_buf.c_str();
  h->route_i8_B = 0;
  return 0;
}

template <typename T>
int logpdf_grid_ragged(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, const T* X, int64_t ldx,
                       const T* y, int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw,
                       int64_t ldl, int64_t strideLw, int64_t G, const T* alpha, int64_t stride_alpha, const T* tau, int64_t stride_tau,
                       double* logpdf, int64_t stride_lp, int64_t* best, T* mw_best, int64_t stride_mwbest, T* T_best, int64_t ldt,
                       int64_t strideT, int32_t* info, int64_t stride_info) {
  RaggedFront f;
  if (const int rc = ragged_front(h, f, memspace, layout, B, D, offsets, X, ldx, noise_kind, strides)) return rc;
  const bool any = f.any, diag = f.diag;
  if (any && !y) return bad_arg(h, 9, "y is NULL (reference :74 length check)");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 10, "noise_kind (the grid scales an isotropic or diagonal base noise; dense Sigma_y is not supported)");
  if (!s && (noise_kind == BLR_NOISE_ISOTROPIC || any)) return bad_arg(h, 11, "s is NULL");
  if (strides < 0) return bad_arg(h, 12, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 13, "prior_kind (dense or diagonal precision; pass a carried-forward factor as U'U)");
  if (!mw) return bad_arg(h, 14, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 15, "stridemw < 0");
  if (!Lw) return bad_arg(h, 16, "Lw is NULL");
  if (prior_kind == BLR_PRIOR_DENSE && ldl < D) return bad_arg(h, 17, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 18, "strideLw < 0");
  if (G < 0 || G > (1 << 20)) return bad_arg(h, 19, "G out of range (0..2^20)");
  if (alpha && stride_alpha != 0 && stride_alpha < G) return bad_arg(h, 21, "stride_alpha (0 = one grid for every regressor, else >= G)");
  if (tau && stride_tau != 0 && stride_tau < G) return bad_arg(h, 23, "stride_tau (0 = one grid for every regressor, else >= G)");
  if (G > 0 && !logpdf) return bad_arg(h, 24, "logpdf is NULL");
  if (stride_lp < G) return bad_arg(h, 25, "stride_lp < G");
  if (mw_best && B > 1 && stride_mwbest < D) return bad_arg(h, 28, "stride_mwbest < D");
  if (T_best && ldt < D) return bad_arg(h, 30, "ldt < D");
  if (T_best && B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 31, "strideT too small");
  if (G > 0 && !info) return bad_arg(h, 32, "info is NULL");
  if (stride_info < G) return bad_arg(h, 33, "stride_info < G");
  // one workgroup of 256 threads per (regressor, setting) / (regressor, column block): a launch takes fewer than 2^32 threads
  if (B * std::max<int64_t>(G, 1) >= ((int64_t)1 << 24)) return bad_arg(h, 19, "B * G too large (< 2^24)");
  if (D <= kMaxSmallD && grid_ragged_slots(offsets, B) >= ((int64_t)1 << 24)) return bad_arg(h, 19, "too many column blocks (sum of S_b < 2^24)");
  if (!h) return -1;
  h->last_chunks = 1;  // (no chunk loop; the D > 128 route's nested calls set their own)
  if (B == 0 || G == 0) return 0;
  HIP_TRY(h, hipSetDevice(h->device));
  RaggedEvidenceArgs<T> a{};
  a.ldx = ldx; a.strides = diag ? 0 : strides; a.stridemw = stridemw; a.ldl = ldl; a.strideLw = strideLw;
  a.stride_alpha = stride_alpha; a.stride_tau = stride_tau; a.stride_lp = stride_lp; a.stride_info = stride_info;
  a.stride_mwbest = stride_mwbest; a.ldt = ldt; a.strideT = strideT;
  a.layout = layout; a.noise_kind = noise_kind; a.prior_kind = prior_kind;
  a.D = (int)D; a.B = (int)B; a.G = (int)G;
  CallIO io(h, memspace);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  int64_t* best_out = nullptr;
  int rc;
  if ((rc = io.in(X, f.x_all, &a.X))) return rc;
  if ((rc = io.in(y, f.n_all, &a.y))) return rc;
  if ((rc = io.in(s, f.s_all, &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &a.Lw))) return rc;
  if ((rc = io.in(alpha, extent(B, stride_alpha, (size_t)G), &a.alpha))) return rc;
  if ((rc = io.in(tau, extent(B, stride_tau, (size_t)G), &a.tau))) return rc;
  if ((rc = io.out(logpdf, extent(B, stride_lp, (size_t)G), &a.logpdf))) return rc;
  if ((rc = io.out(info, extent(B, stride_info, (size_t)G), &a.info))) return rc;
  if ((rc = io.out(best, (size_t)B, &best_out))) return rc;
  if ((rc = io.out(mw_best, extent(B, stride_mwbest, (size_t)D), &a.mw_best))) return rc;
  if ((rc = io.out(T_best, extent(B, strideT, mat_extent(D, D, ldt)), &a.T_best))) return rc;
  // no data at all (or, host memspace, nothing staged): the kernels never dereference these, but keep the pointers valid
  if (!a.X) a.X = a.mw;
  if (!a.y) a.y = a.mw;
  if (!a.s) a.s = a.mw;
  if (D <= kMaxSmallD) {
    if ((rc = grid_ragged_small<T>(h, a, offsets, best_out))) return rc;
    return io.finish();
  }
  // D > 128: correct, not fast -- blr_logpdf_grid_* with B = 1 on each slice
  if ((rc = ragged_one_by_one(h, B, offsets, [&](int64_t b, int64_t o, int64_t n) {
         return logpdf_grid<T>(h, BLR_MEM_DEVICE, layout, 1, D, n, a.X + (f.colv ? o * ldx : o), ldx, 0, a.y + o, 0, noise_kind,
                               diag ? a.s + o : a.s + b * strides, 0, prior_kind, a.mw + b * stridemw, 0, a.Lw + b * strideLw, ldl, 0, G,
                               a.alpha ? a.alpha + b * stride_alpha : (const T*)nullptr, 0, a.tau ? a.tau + b * stride_tau : (const T*)nullptr, 0,
                               a.logpdf + b * stride_lp, stride_lp, best_out ? best_out + b : (int64_t*)nullptr,
                               a.mw_best ? a.mw_best + b * stride_mwbest : (T*)nullptr, stride_mwbest, a.T_best ? a.T_best + b * strideT : (T*)nullptr,
                               ldt, strideT, a.info + b * stride_info, stride_info);
       })))
    return rc;
  return io.finish();
}

// ---- condition / forget on resident states with unequal counts (blr_revise_ragged.hpp, blr_revise_ragged_plan.hpp) ----
// One front for the pair (DOWN: forget).  The plan's lists and offsets go to the metadata buffer in one upload; then the idle fill, one
// launch per chunk of the sweep list and -- update only -- one launch of fused_ragged_kernel per chunk of the refit list, in place.
template <typename T, bool DOWN>
int revise_ragged(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, const T* X, int64_t ldx, const T* y,
                  int noise_kind, const T* s, int64_t strides, T* mw, int64_t stridemw, T* Tf, int64_t ldt, int64_t strideT, double* logpdf,
                  int32_t* info) {
  RaggedFront f;
  if (const int rc = ragged_front(h, f, memspace, layout, B, D, offsets, X, ldx, noise_kind, strides)) return rc;
  const bool diag = f.diag;
  if (f.any && !y) return bad_arg(h, 9, "y is NULL (reference :74 length check)");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 10, "noise_kind (isotropic or diagonal; a resident state is not revised under a dense Sigma_y)");
  if (!s && (noise_kind == BLR_NOISE_ISOTROPIC || f.any)) return bad_arg(h, 11, "s is NULL");
  if (strides < 0) return bad_arg(h, 12, "strides < 0");
  if (!mw) return bad_arg(h, 13, "mw is NULL");
  if (B > 1 && stridemw < D) return bad_arg(h, 14, "stridemw < D");
  if (!Tf) return bad_arg(h, 15, "T is NULL");
  if (ldt < D) return bad_arg(h, 16, "ldt < D");
  if (B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 17, "strideT too small");
  if (B > 0 && !info) return bad_arg(h, 19, "info is NULL");
  if (B == 0) return 0;
  if (!h) return -1;
  HIP_TRY(h, hipSetDevice(h->device));
  ReviseRaggedPlan plan;
  plan_revise_ragged(offsets, B, D, DOWN, h->opt, plan);
  const int64_t ns = (int64_t)plan.sweep.size(), nr = (int64_t)plan.refit.size();
  h->ragged_lists = {ns, nr, (int64_t)plan.idle.size()};
  h->last_chunks = plan.last_chunks;

  ReviseRaggedArgs<T> r{};
  SweepArgs<T>& a = r.s;
  a.ldx = ldx; a.layout = layout; a.strides = diag ? 0 : strides; a.noise_kind = noise_kind;
  a.stridemw = stridemw; a.ldt = ldt; a.strideT = strideT; a.D = (int)D;
  CallIO io(h, memspace);
  int rc;
  if ((rc = io.in(X, f.x_all, &a.X))) return rc;
  if ((rc = io.in(y, f.n_all, &a.y))) return rc;
  if ((rc = io.in(s, f.s_all, &a.s))) return rc;
  if ((rc = io.out(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.out(Tf, extent(B, strideT, mat_extent(D, D, ldt)), &a.Tf))) return rc;
  if ((rc = io.out(logpdf, (size_t)B, &a.logpdf))) return rc;
  if ((rc = io.out(info, (size_t)B, &a.info))) return rc;
  // no data at all (or, host memspace, nothing staged): never dereferenced, but keep the pointers valid
  if (!a.X) a.X = a.mw;
  if (!a.y) a.y = a.mw;
  if (!a.s) a.s = a.mw;

  const char* dev[3];
  if ((rc = ragged_meta_upload(h, {{offsets, ragged_table_bytes(B)}, {plan.sweep.data(), (size_t)ns * sizeof(int32_t)},
                                   {plan.refit.data(), (size_t)nr * sizeof(int32_t)}}, dev)))
    return rc;
  r.offsets = reinterpret_cast<const int64_t*>(dev[0]);
  const int32_t* const sweep_dev = reinterpret_cast<const int32_t*>(dev[1]);
  const int32_t* const refit_dev = reinterpret_cast<const int32_t*>(dev[2]);
  if (!plan.idle.empty()) {
    hipLaunchKernelGGL(revise_ragged_idle_kernel, dim3((unsigned)std::min<int64_t>((B + kThreads - 1) / kThreads, 1024)), dim3(kThreads), 0,
                       h->stream, r.offsets, B, a.logpdf, a.info);
    HIP_TRY(h, hipGetLastError());
  }
  if (plan.serial) {
    // correct, not fast: the equal-count entry point with B = 1 on each active regressor's slice and state
    if ((rc = ragged_one_by_one(h, B, offsets, [&](int64_t b, int64_t o, int64_t n) {
           if (n == 0) return 0;
           const auto one = DOWN ? downdate_factor<T> : update_factor<T>;
           return one(h, BLR_MEM_DEVICE, layout, 1, D, n, a.X + (f.colv ? o * ldx : o), ldx, 0, a.y + o, 0, noise_kind,
                      diag ? a.s + o : a.s + b * strides, 0, a.mw + b * stridemw, 0, a.Tf + b * strideT, ldt, 0,
                      a.logpdf ? a.logpdf + b : (double*)nullptr, a.info + b);
         })))
      return rc;
    h->last_chunks = plan.last_chunks;  // (the nested calls counted their own)
    return io.finish();
  }
  if (ns > 0) {
    void (*const kern)(ReviseRaggedArgs<T>) = DOWN ? downdate_ragged_kernel<T> : update_ragged_sweep_kernel<T>;
    const int lds = DOWN ? downdate_lds_bytes<T>((int)D) : sweep_lds_bytes<T>((int)D);
    if ((rc = set_lds_once(h, kern, (size_t)lds))) return rc;
    for (int64_t c0 = 0; c0 < ns; c0 += plan.chunk) {
      r.list = sweep_dev + c0;
      hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(plan.chunk, ns - c0)), dim3(kThreads), lds, h->stream, r);
    }
    HIP_TRY(h, hipGetLastError());
    h->route = DOWN ? "downdate_ragged_kernel" : "update_ragged_sweep_kernel";
    h->route_i8_B = 0;
  }
  if (nr > 0) {
    // the SAME state re-factored in place, the old factor entering as D pseudo-observations (what blr_update_factor_* does for k >= 2)
    RaggedArgs<T> g{};
    PosteriorArgs<T>& p = g.p;
    p.X = a.X; p.ldx = ldx; p.y = a.y; p.s = a.s; p.strides = a.strides;
    p.mw = a.mw; p.stridemw = stridemw; p.Lw = a.Tf; p.ldl = ldt; p.strideLw = strideT;
    p.mw_post = a.mw; p.stride_mwpost = stridemw; p.T_post = a.Tf; p.ldt = ldt; p.strideT = strideT;
    p.logpdf = a.logpdf; p.info = a.info;
    p.layout = layout; p.noise_kind = noise_kind; p.prior_kind = BLR_PRIOR_UPPER_FACTOR; p.D = (int)D;
    g.offsets = r.offsets;
    for (int64_t c0 = 0; c0 < nr; c0 += plan.chunk) {
      p.B = (int)std::min<int64_t>(plan.chunk, nr - c0);
      g.order = refit_dev + c0;
      if ((rc = ragged_enqueue<T>(h, g))) return rc;
    }
  }
  return io.finish();
}

// ---- ragged marginals and leave-one-out (blr_marg_ragged.hpp, blr_ragged_items.hpp) ---------------------------------
// The plan of a call, and offsets and its items in the handle's metadata buffer (K14's: the entry points never share a call)
template <typename T>
int marg_ragged_plan(blr_handle* h, const int64_t* offsets, int64_t B, RaggedPlan& p, MargRaggedArgs<T>& a) {
  plan_ragged(offsets, B, h->cus, (int)sizeof(T), h->opt, p);
  const char* dev[2];
  if (const int rc = ragged_meta_upload(h, {{offsets, ragged_table_bytes(B)}, {p.items.data(), p.items.size() * sizeof(RaggedItem)}}, dev)) return rc;
  a.offsets = reinterpret_cast<const int64_t*>(dev[0]);
  a.items = reinterpret_cast<const RaggedItem*>(dev[1]);
  return 0;
}

// ---- what the packed held-out entry points share behind their own argument checks (blr_loo_ragged_*, blr_kfold_ragged_*): the
// counterparts of heldout_status, LogpdfSpill and heldout_totals ----
// Status of every state, the noise scan on its slice (off_dev: the uploaded offsets): loo_ragged_check_kernel, at most 65535
// regressors per launch (grid.x).  Returns that chunk; the caller asks for the launches' error.
template <typename T>
int64_t heldout_ragged_status(blr_handle* h, int64_t B, int64_t D, const T* Tf, int64_t ldt, int64_t strideT, const T* s, int64_t strides,
                              int noise_kind, const int64_t* off_dev, int32_t* info) {
  const int64_t ychunk = h->cap_chunk(65535);
  for (int64_t b0 = 0; b0 < B; b0 += ychunk)
    hipLaunchKernelGGL(loo_ragged_check_kernel<T>, dim3((unsigned)std::min<int64_t>(ychunk, B - b0)), dim3(kThreads), 0, h->stream, Tf + b0 * strideT,
                       ldt, strideT, (int)D, noise_kind == BLR_NOISE_DIAGONAL ? s : s + b0 * strides, strides, noise_kind, off_dev + b0, info + b0);
  return ychunk;
}
// The totals need the log densities somewhere: wanted without them, n doubles go to the held-out workspace behind the `front` bytes
// the caller uses of it, packed as the output is (first: the index of its first entry).  Reserves front + the spill + pad bytes, if
// any of the first two.
inline int heldout_ragged_spill(blr_handle* h, const double* total, size_t front, size_t n, int64_t first, size_t pad, double** ll) {
  const bool on = total && !*ll;
  if (!front && !on) return 0;
  if (const int rc = h->loo_ws.reserve(h, front + (on ? n * sizeof(double) : 0) + pad)) return rc;
  if (on) *ll = reinterpret_cast<double*>(h->loo_ws.p + front) - first;
  return 0;
}
// Totals of every regressor over its log densities ll[ll_off[b] .. ll_off[b + 1]) (ll_off: a device table), in the chunks of the status
inline void heldout_ragged_totals(blr_handle* h, int64_t B, int64_t ychunk, const double* ll, const int64_t* ll_off, double* total, const int32_t* info) {
  for (int64_t b0 = 0; b0 < B; b0 += ychunk)
    hipLaunchKernelGGL(loo_ragged_total_kernel, dim3((unsigned)std::min<int64_t>(ychunk, B - b0)), dim3(kThreads), 0, h->stream, ll, ll_off + b0,
                       total + b0, info + b0);
}

// The product stream takes D = 128 with a factor when the variance is wanted: RowVecs, or ColVecs whose X and ldx are multiples of 16
// bytes (every regressor's slice then is).  Asked of the caller's pointer as well as of the staged one: a host-memspace call takes the
// route the same call takes in device memspace, so the two give the same bits
template <typename T>
bool marg_ragged_gemm_takes(const blr_handle* h, int layout, int64_t D, const T* X, int64_t ldx) {
  return !h->opt.no_marg_gemm && D == kPB && (layout == BLR_LAYOUT_ROWVECS || ((ldx % Mfma<T>::VEC) == 0 && ((uintptr_t)X % 16) == 0));
}

// One workgroup per item, chunk by chunk (a.offsets / a.items: the uploaded tables; everything indexes the global regressor)
template <typename T, bool LOO>
int marg_ragged_launch(blr_handle* h, MargRaggedArgs<T> a, const RaggedPlan& p, bool gemm) {
  using G = MargGemmCfg<T>;
  using RC = MargRaggedRowsCfg<T>;
  const bool rowv = a.layout == BLR_LAYOUT_ROWVECS;
  void (*const gk)(MargRaggedArgs<T>, const T*) = rowv ? marg_ragged_gemm_kernel<T, true, LOO> : marg_ragged_gemm_kernel<T, false, LOO>;
  void (*const rk)(MargRaggedArgs<T>) = marg_ragged_rows_kernel<T, LOO>;
  const bool rows_factor = (LOO || a.var) && a.prior_kind == BLR_PRIOR_UPPER_FACTOR;
  int rc;
  const bool images = gemm && (LOO || a.var);
  if (gemm) {
    if (images && (rc = MargImages<T>::reserve(h, std::max<int64_t>(1, p.max_nb)))) return rc;
    if ((rc = set_lds_once(h, gk, (size_t)G::LDS_BYTES))) return rc;
  } else if ((rc = set_lds_once(h, rk, (size_t)RC::LDS_FACTOR))) {
    return rc;
  }
  const RaggedItem* const items = a.items;
  for (const RaggedChunk& c : p.chunks) {
    if (c.nitems == 0) continue;
    a.items = items + c.item0;
    if (gemm) {
      T* const img = images ? MargImages<T>::launch(h, a.U, a.ldu, a.strideU, a.D, a.info, c.b0, c.nb) : (T*)nullptr;
      hipLaunchKernelGGL(gk, dim3((unsigned)c.nitems), dim3(kThreads), G::LDS_BYTES, h->stream, a, (const T*)img);
    } else {
      hipLaunchKernelGGL(rk, dim3((unsigned)c.nitems), dim3(kThreads), rows_factor ? RC::LDS_FACTOR : RC::LDS_STREAM, h->stream, a);
    }
    HIP_TRY(h, hipGetLastError());
  }
  h->last_chunks = std::max<int64_t>(1, p.last_chunks);
  h->route = gemm ? "marg_ragged_gemm_kernel" : "marg_ragged_rows_kernel";
  h->route_i8_B = 0;
  return 0;
}

template <typename T>
int marginals_ragged(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, const T* X, int64_t ldx,
                     int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw, int64_t ldl,
                     int64_t strideLw, T* mean, T* var, int32_t* info) {
  RaggedFront f;
  if (const int rc = ragged_front(h, f, memspace, layout, B, D, offsets, X, ldx, noise_kind, strides)) return rc;
  const bool any = f.any, colv = f.colv, diag = f.diag;
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 9, "noise_kind (isotropic or diagonal; dense Sigma_y is not supported for unequal counts)");
  if (var && any && !s) return bad_arg(h, 10, "s is NULL");
  if (strides < 0) return bad_arg(h, 11, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 12, "prior_kind");
  if (!mw) return bad_arg(h, 13, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 14, "stridemw < 0");
  if (var && !Lw) return bad_arg(h, 15, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 16, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 17, "strideLw < 0");
  if (B > 0 && !info) return bad_arg(h, 20, "info is NULL");
  if (B == 0) return 0;
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  MargRaggedArgs<T> a{};
  a.ldx = ldx; a.strides = strides; a.stridemw = stridemw; a.layout = layout; a.noise_kind = noise_kind; a.D = (int)D;
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  const T* Lw_dev = nullptr;
  int32_t* info_dev = nullptr;
  int rc;
  if ((rc = io.in(X, f.x_all, &a.X))) return rc;
  if ((rc = io.in(var ? s : (const T*)nullptr, f.s_all, &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(var ? Lw : (const T*)nullptr, extent(B, strideLw, lw_one), &Lw_dev))) return rc;
  if ((rc = io.out(mean, f.n_all, &a.mean))) return rc;
  if ((rc = io.out(var, f.n_all, &a.var))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_dev))) return rc;
  if (!any || (!mean && !var)) {  // nothing per observation to write: the status of a call without a factorisation
    HIP_TRY(h, hipMemsetAsync(info_dev, 0, (size_t)B * sizeof(int32_t), h->stream));
    return io.finish();
  }
  if (D > kMaxSmallD) {  // through blr_marginals_batched_*: an empty regressor keeps the status of a call without a factorisation
    HIP_TRY(h, hipMemsetAsync(info_dev, 0, (size_t)B * sizeof(int32_t), h->stream));
    if ((rc = ragged_one_by_one(h, B, offsets, [&](int64_t b, int64_t o, int64_t n) {
           if (n == 0) return 0;
           return marginals_batched<T>(h, BLR_MEM_DEVICE, layout, 1, D, n, a.X + (colv ? o * ldx : o), ldx, 0, noise_kind,
                                       a.s ? (diag ? a.s + o : a.s + b * strides) : (const T*)nullptr, 0, prior_kind, a.mw + b * stridemw, 0,
                                       Lw_dev ? Lw_dev + b * strideLw : (const T*)nullptr, ldl, 0, a.mean ? a.mean + o : (T*)nullptr, 0,
                                       a.var ? a.var + o : (T*)nullptr, 0, info_dev + b);
         })))
      return rc;
    return io.finish();
  }
  RaggedPlan plan;
  if ((rc = marg_ragged_plan<T>(h, offsets, B, plan, a))) return rc;
  // a dense prior is factorised once per regressor; its status is the call's
  int32_t* chol_info = nullptr;
  int kind = prior_kind;
  if (var) {
    if ((rc = prior_factor<T>(h, B, D, prior_kind, Lw_dev, ldl, strideLw, &a.U, &a.ldu, &a.strideU, &kind, &chol_info))) return rc;
  } else {
    a.U = Lw_dev; a.ldu = ldl; a.strideU = strideLw;
  }
  a.prior_kind = kind;
  a.info = chol_info;
  if (chol_info) HIP_TRY(h, hipMemcpyAsync(info_dev, chol_info, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  else HIP_TRY(h, hipMemsetAsync(info_dev, 0, (size_t)B * sizeof(int32_t), h->stream));
  // the route follows from the shape and the prior kind alone -- not from the outputs requested: a mean has the same bits alone
  // and next to its variance (the stream kernel then runs without image and product)
  const bool gemm = prior_kind != BLR_PRIOR_DIAGONAL && marg_ragged_gemm_takes<T>(h, layout, D, X, ldx) && marg_ragged_gemm_takes<T>(h, layout, D, a.X, ldx);
  if ((rc = marg_ragged_launch<T, false>(h, a, plan, gemm))) return rc;
  return io.finish();
}

template <typename T>
int loo_ragged(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, const T* X, int64_t ldx, const T* y,
               int noise_kind, const T* s, int64_t strides, const T* mw, int64_t stridemw, const T* Tf, int64_t ldt, int64_t strideT,
               T* loo_mean, T* loo_var, double* loo_logpdf, double* loo_total, int32_t* info) {
  RaggedFront f;
  if (const int rc = ragged_front(h, f, memspace, layout, B, D, offsets, X, ldx, noise_kind, strides)) return rc;
  const bool any = f.any, colv = f.colv, diag = f.diag;
  if (any && !y) return bad_arg(h, 9, "y is NULL (reference :74 length check)");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 10, "noise_kind (dense noise has no single-observation LOO: that is a block LOO)");
  if (any && !s) return bad_arg(h, 11, "s is NULL");
  if (strides < 0) return bad_arg(h, 12, "strides < 0");
  if (!mw) return bad_arg(h, 13, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 14, "stridemw < 0");
  if (!Tf) return bad_arg(h, 15, "T is NULL");
  if (ldt < D) return bad_arg(h, 16, "ldt < D");
  if (strideT < 0) return bad_arg(h, 17, "strideT < 0");
  if (B > 0 && !info) return bad_arg(h, 22, "info is NULL");
  if (B == 0) return 0;
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  MargRaggedArgs<T> a{};
  a.ldx = ldx; a.strides = strides; a.stridemw = stridemw; a.layout = layout; a.noise_kind = noise_kind; a.D = (int)D;
  a.prior_kind = BLR_PRIOR_UPPER_FACTOR; a.ldu = ldt; a.strideU = strideT;
  const size_t n_all = f.n_all;
  double* total_dev = nullptr;
  int32_t* info_dev = nullptr;
  int rc;
  if ((rc = io.in(X, f.x_all, &a.X))) return rc;
  if ((rc = io.in(y, n_all, &a.y))) return rc;
  if ((rc = io.in(s, any ? f.s_all : 0, &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Tf, extent(B, strideT, mat_extent(D, D, ldt)), &a.U))) return rc;
  if ((rc = io.out(loo_mean, n_all, &a.lm))) return rc;
  if ((rc = io.out(loo_var, n_all, &a.lv))) return rc;
  if ((rc = io.out(loo_logpdf, n_all, &a.ll))) return rc;
  if ((rc = io.out(loo_total, (size_t)B, &total_dev))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_dev))) return rc;
  if (!a.s) a.s = a.mw;  // (no observation at all: never dereferenced, but a valid pointer)
  if (D > kMaxSmallD) {  // through blr_loo_batched_*
    if ((rc = ragged_one_by_one(h, B, offsets, [&](int64_t b, int64_t o, int64_t n) {
           return loo_batched<T>(h, BLR_MEM_DEVICE, layout, 1, D, n, a.X ? a.X + (colv ? o * ldx : o) : (const T*)nullptr, ldx, 0,
                                 a.y ? a.y + o : (const T*)nullptr, 0, noise_kind, diag ? a.s + o : a.s + b * strides, 0, a.mw + b * stridemw, 0,
                                 a.U + b * strideT, ldt, 0, a.lm ? a.lm + o : (T*)nullptr, 0, a.lv ? a.lv + o : (T*)nullptr, 0,
                                 a.ll ? a.ll + o : (double*)nullptr, 0, total_dev ? total_dev + b : (double*)nullptr, info_dev + b);
         })))
      return rc;
    return io.finish();
  }
  if ((rc = ensure_stats(h))) return rc;
  a.degenerate = h->stats_dev + 3;
  a.info = info_dev;
  RaggedPlan plan;
  if ((rc = marg_ragged_plan<T>(h, offsets, B, plan, a))) return rc;
  const int64_t ychunk = heldout_ragged_status<T>(h, B, D, a.U, ldt, strideT, a.s, strides, noise_kind, a.offsets, info_dev);
  HIP_TRY(h, hipGetLastError());
  if ((rc = heldout_ragged_spill(h, total_dev, 0, n_all, offsets[0], sizeof(double), &a.ll))) return rc;
  if (any && (a.lm || a.lv || a.ll)) {
    const bool gemm = marg_ragged_gemm_takes<T>(h, layout, D, X, ldx) && marg_ragged_gemm_takes<T>(h, layout, D, a.X, ldx);
    if ((rc = marg_ragged_launch<T, true>(h, a, plan, gemm))) return rc;
  }
  if (total_dev) heldout_ragged_totals(h, B, ychunk, a.ll, a.offsets, total_dev, info_dev);
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- batched multi-output posterior: S target columns per regressor (blr_posterior_multi_batched_*) ----------------

template <typename T>
int posterior_multi_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, const T* X, int64_t ldx,
                            int64_t strideX, const T* Y, int64_t ldY, int64_t strideY, int noise_kind, const T* s, int64_t strides,
                            int prior_kind, const T* mw, int64_t stridemw, const T* Lw, int64_t ldl, int64_t strideLw, T* mw_post,
                            int64_t ldmp, int64_t stride_mwpost, T* T_post, int64_t ldt, int64_t strideT, T* Lw_post, int64_t ldlp,
                            int64_t strideLp, double* logpdf, int64_t stride_lp, int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range");
  if (S < 0 || S > (1 << 20)) return bad_arg(h, 7, "S out of range (0..2^20)");
  if (B == 0 || S == 0) return 0;
  if (N > 0 && !X) return bad_arg(h, 8, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(N, 1)) return bad_arg(h, 9, "ldx too small");
  if (strideX < 0) return bad_arg(h, 10, "strideX < 0");
  if (N > 0 && !Y) return bad_arg(h, 11, "Y is NULL (reference :74 length check)");
  if (ldY < N) return bad_arg(h, 12, "ldY < N (reference :74 length check)");
  if (strideY < 0) return bad_arg(h, 13, "strideY < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 14, "noise_kind (isotropic or diagonal; dense Sigma_y is not supported for batched multi-output targets)");
  if (!s) return bad_arg(h, 15, "s is NULL");
  if (strides < 0) return bad_arg(h, 16, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 17, "prior_kind");
  if (!mw) return bad_arg(h, 18, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 19, "stridemw < 0");
  if (!Lw) return bad_arg(h, 20, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 21, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 22, "strideLw < 0");
  if (mw_post && mw_post == mw) return bad_arg(h, 23, "mw_post == mw (the columns after the first still need the prior mean)");
  if (mw_post && ldmp < D) return bad_arg(h, 24, "ldmp < D");
  if (mw_post && B > 1 && stride_mwpost < ldmp * S) return bad_arg(h, 25, "stride_mwpost < ldmp * S");
  if (T_post && T_post == Lw) return bad_arg(h, 26, "T_post == Lw (aliasing an output with an input is not supported)");
  if (T_post && ldt < D) return bad_arg(h, 27, "ldt < D");
  if (T_post && B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 28, "strideT too small");
  if (Lw_post && ldlp < D) return bad_arg(h, 30, "ldlp < D");
  if (Lw_post && B > 1 && strideLp < (int64_t)mat_extent(D, D, ldlp)) return bad_arg(h, 31, "strideLp too small");
  if (logpdf && B > 1 && stride_lp < S) return bad_arg(h, 33, "stride_lp < S");
  if (!info) return bad_arg(h, 34, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  PosteriorArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.stridey = strideY; a.strides = strides; a.stridemw = stridemw;
  a.ldl = ldl; a.strideLw = strideLw; a.stride_mwpost = stride_mwpost; a.ldt = ldt; a.strideT = strideT;
  a.ldlp = ldlp; a.strideLp = strideLp;
  a.layout = layout; a.noise_kind = noise_kind; a.prior_kind = prior_kind;
  a.D = (int)D; a.N = (int)N; a.B = (int)B;

  CallIO io(h, memspace);
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  const size_t s_one = noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1;
  double* lp_d = nullptr;
  int rc;
  if ((rc = io.in(X, extent(B, strideX, x_one), &a.X))) return rc;
  if ((rc = io.in(Y, N > 0 ? extent(B, strideY, mat_extent(N, S, ldY)) : 0, &a.y))) return rc;
  if ((rc = io.in(s, extent(B, strides, s_one), &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Lw, extent(B, strideLw, lw_one), &a.Lw))) return rc;
  if ((rc = io.out(mw_post, extent(B, stride_mwpost, mat_extent(D, S, ldmp)), &a.mw_post))) return rc;
  if ((rc = io.out(T_post, extent(B, strideT, mat_extent(D, D, ldt)), &a.T_post))) return rc;
  if ((rc = io.out(Lw_post, extent(B, strideLp, mat_extent(D, D, ldlp)), &a.Lw_post))) return rc;
  if ((rc = io.out(logpdf, extent(B, stride_lp, (size_t)S), &lp_d))) return rc;
  if ((rc = io.out(info, (size_t)B, &a.info))) return rc;
  const T* const Y_d = a.y;

  if (D > kMaxSmallD) {
    // correct, not fast: one regressor after the other -- column 0 through the pipeline of blr_posterior_batched_* (which hands out the
    // factor, the precision and the status), the further columns through the shared-X pipeline of blr_logpdf_multi_*; the call synchronises
    const AsyncScope drain(h, false);
    double* lp_tmp = nullptr;
    int32_t* info_tmp = nullptr;
    if ((rc = io.tmp((size_t)S, &lp_tmp))) return rc;
    if ((rc = io.tmp((size_t)1, &info_tmp))) return rc;
    const std::vector<double> nans((size_t)S, __builtin_nan(""));
    for (int64_t b = 0; b < B; ++b) {
      const T* const Xb = a.X ? a.X + b * strideX : (const T*)nullptr;
      const T* const Yb = Y_d ? Y_d + b * strideY : (const T*)nullptr;
      T* const mpb = a.mw_post ? a.mw_post + b * stride_mwpost : (T*)nullptr;
      double* const lpb = lp_d ? lp_d + b * stride_lp : (double*)nullptr;
      const int64_t first_cols = N == 0 ? S : 1;  // without data there is no shared work: every column is its own (trivial) update
      for (int64_t c = 0; c < first_cols; ++c) {
        rc = posterior_batched<T>(h, BLR_MEM_DEVICE, layout, 1, D, N, Xb, ldx, 0, Yb ? Yb + c * ldY : (const T*)nullptr, 0, noise_kind,
                                  a.s + b * strides, 0, prior_kind, a.mw + b * stridemw, 0, a.Lw + b * strideLw, ldl, 0,
                                  mpb ? mpb + c * ldmp : (T*)nullptr, 0, c == 0 && a.T_post ? a.T_post + b * strideT : (T*)nullptr, ldt, 0,
                                  c == 0 && a.Lw_post ? a.Lw_post + b * strideLp : (T*)nullptr, ldlp, 0, lpb ? lpb + c : (double*)nullptr,
                                  c == 0 ? a.info + b : info_tmp);
        if (rc) return rc;  // (device pointers and in-range sizes: a HIP failure, not an argument index of the inner call)
      }
      int32_t st = 0;
      HIP_TRY(h, hipMemcpyAsync(&st, a.info + b, sizeof(st), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      if (st != 0) {
        if (lpb) HIP_TRY(h, hipMemcpyAsync(lpb, nans.data(), (size_t)S * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        continue;
      }
      for (int64_t c = 1; c < S && N > 0; c += 65536) {  // (blr_logpdf_multi_* takes up to 65536 columns)
        rc = logpdf_multi<T>(h, BLR_MEM_DEVICE, layout, D, N, std::min<int64_t>(65536, S - c), Xb, ldx, Yb + c * ldY, ldY, noise_kind,
                             a.s + b * strides, prior_kind, a.mw + b * stridemw, a.Lw + b * strideLw, ldl, lpb ? lpb + c : lp_tmp,
                             mpb ? mpb + c * ldmp : (T*)nullptr, ldmp, info_tmp);
        if (rc) return rc;
      }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return io.finish();
  }

  // D <= 128.  Step 1: column 0 of every regressor through the dispatch of blr_posterior_batched_*, unchanged; its evidence waits in the
  // handle's workspace (the caller's logpdf has a stride of its own), and so does the factor when the caller does not want it
  const size_t lp0_bytes = ((size_t)B * sizeof(double) + 255) & ~(size_t)255;
  const bool own_T = a.T_post == nullptr && S > 1;
  if ((rc = h->multi_ws.reserve(h, lp0_bytes + (own_T ? (size_t)B * D * D * sizeof(T) : 0)))) return rc;
  double* const lp0 = reinterpret_cast<double*>(h->multi_ws.p);
  if (own_T) { a.T_post = reinterpret_cast<T*>(h->multi_ws.p + lp0_bytes); a.ldt = D; a.strideT = D * D; }
  a.logpdf = lp0;
  if ((rc = posterior_run<T>(h, a))) return rc;
  // Step 2: ONE launch for the columns 1 .. S-1 of every regressor (and the copy of column 0's evidence to its place)
  MultiColsArgs<T> m{};
  m.X = a.X; m.ldx = ldx; m.strideX = strideX; m.Y = Y_d ? Y_d : a.mw; m.ldY = ldY; m.strideY = strideY; m.s = a.s; m.strides = strides;
  m.mw = a.mw; m.stridemw = stridemw; m.Tf = a.T_post ? a.T_post : a.mw; m.ldt = a.ldt; m.strideT = a.strideT; m.lp0 = lp0; m.info = a.info;
  m.mw_post = a.mw_post; m.ldmp = ldmp; m.stride_mwpost = stride_mwpost; m.logpdf = lp_d; m.stride_lp = stride_lp;
  m.noise_kind = noise_kind; m.D = (int)D; m.N = (int)N; m.S = (int)S;
  const int per_pass = kMultiColsPerPass - 1;
  const int64_t passes = std::max<int64_t>(1, (S - 1 + per_pass - 1) / per_pass);
  const size_t lds = multi_cols_lds_bytes(sizeof(T), (int)D, (int)std::min<int64_t>(S, kMultiColsPerPass));
  void (*const kern)(MultiColsArgs<T>) = layout == BLR_LAYOUT_ROWVECS ? multi_cols_kernel<T, LAYOUT_ROWVECS> : multi_cols_kernel<T, LAYOUT_COLVECS>;
  if ((rc = set_lds_once(h, kern, lds))) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)B, (unsigned)passes), dim3(kThreads), lds, h->stream, m);
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- marginals of a batched multi-output posterior: S mean columns, one variance per input (blr_marginals_multi_batched_*) ----

template <typename T>
int marginals_multi_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, const T* X, int64_t ldx,
                            int64_t strideX, int noise_kind, const T* s, int64_t strides, int prior_kind, const T* M, int64_t ldm,
                            int64_t strideM, const T* Lw, int64_t ldl, int64_t strideLw, T* mean, int64_t ldmean, int64_t stridemean,
                            T* var, int64_t stridevar, int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range");
  if (S < 0 || S > (1 << 20)) return bad_arg(h, 7, "S out of range (0..2^20)");
  if (S == 0) mean = nullptr;  // (var only: M and mean are ignored)
  if (B == 0 || N == 0 || (!mean && !var)) return 0;
  if (!X) return bad_arg(h, 8, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N) return bad_arg(h, 9, "ldx too small");
  if (strideX < 0) return bad_arg(h, 10, "strideX < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 11, "noise_kind (isotropic or diagonal; dense Sigma_y is not supported for batched marginals)");
  if (var && !s) return bad_arg(h, 12, "s is NULL");
  if (strides < 0) return bad_arg(h, 13, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 14, "prior_kind");
  if (mean && !M) return bad_arg(h, 15, "M is NULL");
  if (mean && ldm < D) return bad_arg(h, 16, "ldm < D");
  if (strideM < 0) return bad_arg(h, 17, "strideM < 0");
  if (var && !Lw) return bad_arg(h, 18, "Lw is NULL");
  if (var && prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 19, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 20, "strideLw < 0");
  if (mean && ldmean < N) return bad_arg(h, 22, "ldmean < N");
  if (mean && B > 1 && stridemean < ldmean * S) return bad_arg(h, 23, "stridemean < ldmean * S");
  if (var && B > 1 && stridevar < N) return bad_arg(h, 25, "stridevar < N");
  if (!info) return bad_arg(h, 26, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  const T *X_d = nullptr, *s_d = nullptr, *M_d = nullptr, *Lw_d = nullptr;
  T *mean_d = nullptr, *var_d = nullptr;
  int32_t* info_d = nullptr;
  int rc;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  if ((rc = io.in(X, extent(B, strideX, x_one), &X_d))) return rc;
  if ((rc = io.in(var ? s : (const T*)nullptr, extent(B, strides, noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1), &s_d))) return rc;
  if ((rc = io.in(mean ? M : (const T*)nullptr, extent(B, strideM, mat_extent(D, S, ldm)), &M_d))) return rc;
  if ((rc = io.in(var ? Lw : (const T*)nullptr, extent(B, strideLw, lw_one), &Lw_d))) return rc;
  if ((rc = io.out(mean, extent(B, stridemean, mat_extent(N, S, ldmean)), &mean_d))) return rc;
  if ((rc = io.out(var, extent(B, stridevar, (size_t)N), &var_d))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_d))) return rc;

  if (D > kMaxSmallD) {
    // correct, not fast: var of the whole batch through the route of blr_marginals_batched_* (which also writes the status), then the
    // means one regressor after the other as X'W for S weight vectors (the path of blr_apply_weights_*); the call synchronises
    const AsyncScope drain(h, false);
    std::vector<int32_t> st((size_t)B, 0);
    if (var_d) {
      // (mw is not read without a mean; X stands in as a non-NULL pointer)
      rc = marginals_batched<T>(h, BLR_MEM_DEVICE, layout, B, D, N, X_d, ldx, strideX, noise_kind, s_d, strides, prior_kind, X_d, 0, Lw_d, ldl,
                                strideLw, (T*)nullptr, 0, var_d, stridevar, info_d);
      if (rc) return rc;  // (device pointers and in-range sizes: a HIP failure, not an argument index of the inner call)
      HIP_TRY(h, hipMemcpyAsync(st.data(), info_d, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else {
      HIP_TRY(h, hipMemsetAsync(info_d, 0, (size_t)B * sizeof(int32_t), h->stream));
    }
    for (int64_t b = 0; mean_d && b < B; ++b) {
      if (st[(size_t)b] != 0) continue;  // outputs of that regressor stay untouched
      launch_project<T>(h, layout, D, N, S, X_d + b * strideX, ldx, M_d + b * strideM, ldm, (const T*)nullptr, BLR_NOISE_ISOTROPIC,
                        (const T*)nullptr, 0, mean_d + b * stridemean, ldmean);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return io.finish();
  }

  // D <= 128: the factor of a dense prior once per regressor (prior_factor), the triangular inverse of every factor as an MFMA image
  // (marg_image_kernel), then ONE launch of marginals_cols_kernel per chunk of regressors over (column passes x tile groups, regressors)
  MargColsArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.strides = strides; a.ldm = ldm; a.strideM = strideM;
  a.ldmean = ldmean; a.stridemean = stridemean; a.stridevar = stridevar;
  a.noise_kind = noise_kind; a.D = (int)D; a.N = (int)N; a.S = (int)S;
  const T* U = nullptr;
  int64_t ldu = 0, strideU = 0;
  int kind = prior_kind;
  int32_t* chol_info = nullptr;
  if (var_d && (rc = prior_factor<T>(h, B, D, prior_kind, Lw_d, ldl, strideLw, &U, &ldu, &strideU, &kind, &chol_info))) return rc;
  a.prior_kind = kind;
  if (chol_info) HIP_TRY(h, hipMemcpyAsync(info_d, chol_info, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  else HIP_TRY(h, hipMemsetAsync(info_d, 0, (size_t)B * sizeof(int32_t), h->stream));
  const bool with_image = var_d && kind == BLR_PRIOR_UPPER_FACTOR;
  const int64_t chunk = h->cap_chunk(std::min<int64_t>(std::min<int64_t>(B, 65535), with_image ? MargImages<T>::kMaxChunk : 65535));
  h->count_chunks(B, chunk);
  const size_t lds = marg_cols_lds_bytes(sizeof(T), (int)D, with_image);
  void (*const kern)(MargColsArgs<T>) = layout == BLR_LAYOUT_ROWVECS ? marginals_cols_kernel<T, LAYOUT_ROWVECS> : marginals_cols_kernel<T, LAYOUT_COLVECS>;
  if ((rc = set_lds_once(h, kern, lds))) return rc;
  if (with_image && (rc = MargImages<T>::reserve(h, chunk))) return rc;
  const int64_t passes = mean_d ? (S + kMargColsPerPass - 1) / kMargColsPerPass : 1;
  const int64_t ntiles = (N + kMargTile - 1) / kMargTile;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, B - b0);
    if (with_image)
      a.img = MargImages<T>::launch(h, U + b0 * strideU, ldu, strideU, (int)D, chol_info ? (const int32_t*)(chol_info + b0) : (const int32_t*)nullptr, 0, nb);
    const int64_t ngroups = tile_groups(h, ntiles, nb * passes);  // (the set-up: the image, the fragments of M)
    a.X = X_d; a.s = s_d; a.M = M_d; a.dprior = kind == BLR_PRIOR_DIAGONAL ? U : nullptr; a.stridedp = strideU;
    a.info = chol_info; a.mean = mean_d; a.var = var_d; a.ngroups = (int)ngroups; a.reg0 = (int)b0;
    hipLaunchKernelGGL(kern, dim3((unsigned)(passes * ngroups), (unsigned)nb), dim3(kThreads), lds, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- joint predictive covariance of a batch of regressors (blr_mean_and_cov_batched_*; blr_cov_batched.hpp) ----------

template <typename T>
int mean_and_cov_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X, int64_t ldx, int64_t strideX,
                         int noise_kind, const T* s, int64_t lds, int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw,
                         int64_t ldl, int64_t strideLw, T* mean, int64_t stridemean, T* C, int64_t ldc, int64_t strideC, int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (N < 0 || N > kMaxDenseN) return bad_arg(h, 6, "N out of range for an N x N covariance (0..16384)");
  if (B == 0 || N == 0 || (!mean && !C)) return 0;
  if (!X) return bad_arg(h, 7, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < N) return bad_arg(h, 8, "ldx too small");
  if (strideX < 0) return bad_arg(h, 9, "strideX < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL && noise_kind != BLR_NOISE_DENSE) return bad_arg(h, 10, "noise_kind");
  if (C && !s) return bad_arg(h, 11, "s is NULL");
  if (noise_kind == BLR_NOISE_DENSE && lds < N) return bad_arg(h, 12, "lds < N");
  if (strides < 0) return bad_arg(h, 13, "strides < 0");
  if (prior_kind != BLR_PRIOR_DENSE && prior_kind != BLR_PRIOR_UPPER_FACTOR && prior_kind != BLR_PRIOR_DIAGONAL)
    return bad_arg(h, 14, "prior_kind");
  if (mean && !mw) return bad_arg(h, 15, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 16, "stridemw < 0");
  if (C && !Lw) return bad_arg(h, 17, "Lw is NULL");
  if (prior_kind != BLR_PRIOR_DIAGONAL && ldl < D) return bad_arg(h, 18, "ldl < D");
  if (strideLw < 0) return bad_arg(h, 19, "strideLw < 0");
  if (mean && B > 1 && stridemean < N) return bad_arg(h, 21, "stridemean < N");
  if (C && ldc < N) return bad_arg(h, 23, "ldc < N");
  if (C && B > 1 && strideC < ldc * N) return bad_arg(h, 24, "strideC < ldc * N");
  if (!info) return bad_arg(h, 25, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  const T *X_d = nullptr, *s_d = nullptr, *mw_d = nullptr, *Lw_d = nullptr;
  T *mean_d = nullptr, *C_d = nullptr;
  int32_t* info_d = nullptr;
  int rc;
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, N, ldx) : mat_extent(N, D, ldx);
  const size_t lw_one = prior_kind == BLR_PRIOR_DIAGONAL ? (size_t)D : mat_extent(D, D, ldl);
  const size_t s_one = noise_kind == BLR_NOISE_DENSE ? mat_extent(N, N, lds) : (noise_kind == BLR_NOISE_DIAGONAL ? (size_t)N : 1);
  if ((rc = io.in(X, extent(B, strideX, x_one), &X_d))) return rc;
  if ((rc = io.in(C ? s : (const T*)nullptr, extent(B, strides, s_one), &s_d))) return rc;
  if ((rc = io.in(mean ? mw : (const T*)nullptr, extent(B, stridemw, (size_t)D), &mw_d))) return rc;
  if ((rc = io.in(C ? Lw : (const T*)nullptr, extent(B, strideLw, lw_one), &Lw_d))) return rc;
  if ((rc = io.out(mean, extent(B, stridemean, (size_t)N), &mean_d))) return rc;
  if ((rc = io.out(C, extent(B, strideC, mat_extent(N, N, ldc)), &C_d))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_d))) return rc;
  const unsigned status_grid = (unsigned)std::min<int64_t>((B + kWaves - 1) / kWaves, 1024);

  if (D > kMaxSmallD) {
    // correct, not fast: one regressor after the other through the launches of blr_mean_and_cov_* (mean_and_cov_core), into a staging
    // covariance that reaches the caller's only once the regressor's status is known to be 0; the call synchronises per regressor
    std::vector<int32_t> st((size_t)B, 0);
    if (C_d) {
      CovTemps<T> t;
      T *Ct = nullptr, *mt = nullptr;
      int32_t* it = nullptr;
      if ((rc = t.reserve(io, (int)D, (int)N))) return rc;
      if ((rc = io.tmp((size_t)N * N, &Ct))) return rc;
      if ((rc = io.tmp((size_t)N, &mt))) return rc;
      if ((rc = io.tmp(1, &it))) return rc;
      if (prior_kind != BLR_PRIOR_DENSE) {  // the rule of blr_rand_batched_*: the first non-positive diagonal entry
        hipLaunchKernelGGL(rand_batched_status_kernel<T>, dim3(status_grid), dim3(kThreads), 0, h->stream, Lw_d, ldl, strideLw,
                           prior_kind == BLR_PRIOR_DIAGONAL ? 1 : 0, (int)D, B, info_d);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(st.data(), info_d, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
      }
      for (int64_t b = 0; b < B; ++b) {
        if (st[(size_t)b] != 0) continue;  // outputs of that regressor stay untouched
        rc = mean_and_cov_core<T>(h, t, layout, (int)D, (int)N, X_d + b * strideX, ldx, noise_kind, s_d + b * strides, lds, prior_kind,
                                  mean_d ? mw_d + b * stridemw : (const T*)nullptr, Lw_d + b * strideLw, ldl, mean_d ? mt : (T*)nullptr, Ct, N, it);
        if (rc) return rc;
        HIP_TRY(h, hipMemcpyAsync(&st[(size_t)b], it, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (st[(size_t)b] != 0) continue;
        HIP_TRY(h, hipMemcpy2DAsync(C_d + b * strideC, (size_t)ldc * sizeof(T), Ct, (size_t)N * sizeof(T), (size_t)N * sizeof(T), (size_t)N,
                                    hipMemcpyDeviceToDevice, h->stream));
        if (mean_d) HIP_TRY(h, hipMemcpyAsync(mean_d + b * stridemean, mt, (size_t)N * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
      }
      HIP_TRY(h, hipMemcpyAsync(info_d, st.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    } else {  // mean only: Lw is not read and every status is 0
      HIP_TRY(h, hipMemsetAsync(info_d, 0, (size_t)B * sizeof(int32_t), h->stream));
      for (int64_t b = 0; b < B; ++b)
        hipLaunchKernelGGL(mean_small_kernel<T>, dim3((unsigned)((N + 255) / 256)), dim3(kThreads), 0, h->stream, X_d + b * strideX, ldx, layout,
                           mw_d + b * stridemw, (int)D, (int)N, mean_d + b * stridemean);
      HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return io.finish();
  }

  // D <= 128.  Once per call: the factor of a dense prior per regressor (prior_factor) and every regressor's status.  Per chunk of
  // regressors: the triangular inverses as MFMA images (marg_image_kernel), Z = X'L^-T and the mean (cov_whiten_kernel), C = Z Z' +
  // Sigma_y (cov_tiles_kernel) -- three launches whatever B
  CovArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.lds = lds; a.strides = strides; a.stridemw = stridemw; a.stridemean = stridemean;
  a.ldc = ldc; a.strideC = strideC; a.noise_kind = noise_kind; a.D = (int)D; a.N = (int)N;
  const T* U = nullptr;
  int64_t ldu = 0, strideU = 0;
  int kind = prior_kind;
  int32_t* chol_info = nullptr;
  if (C_d && (rc = prior_factor<T>(h, B, D, prior_kind, Lw_d, ldl, strideLw, &U, &ldu, &strideU, &kind, &chol_info))) return rc;
  a.prior_kind = kind;
  if (chol_info) HIP_TRY(h, hipMemcpyAsync(info_d, chol_info, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  else if (C_d) hipLaunchKernelGGL(rand_batched_status_kernel<T>, dim3(status_grid), dim3(kThreads), 0, h->stream, U, ldu, strideU,
                                   kind == BLR_PRIOR_DIAGONAL ? 1 : 0, (int)D, B, info_d);
  else HIP_TRY(h, hipMemsetAsync(info_d, 0, (size_t)B * sizeof(int32_t), h->stream));  // mean only: Lw is not read
  const bool with_image = C_d && kind == BLR_PRIOR_UPPER_FACTOR;
  // regressors per launch: grid.y, the images within 256 MiB, the rows of Z within 256 MiB (at least one regressor: 16 MiB at most)
  const size_t z_one = cov_z_elems((int)D, (int)N);
  const int64_t chunk = whitened_chunk<T>(h, B, with_image, C_d ? z_one : 0, 0);
  h->count_chunks(B, chunk);
  const size_t lds_w = cov_whiten_lds_bytes(sizeof(T), (int)D, with_image), lds_t = cov_tiles_lds_bytes(sizeof(T), (int)D);
  void (*const whiten)(CovArgs<T>) = layout == BLR_LAYOUT_ROWVECS ? cov_whiten_kernel<T, LAYOUT_ROWVECS> : cov_whiten_kernel<T, LAYOUT_COLVECS>;
  if ((rc = set_lds_once(h, whiten, lds_w))) return rc;
  if (C_d && (rc = set_lds_once(h, cov_tiles_kernel<T>, lds_t))) return rc;
  if (with_image && (rc = MargImages<T>::reserve(h, chunk))) return rc;
  if (C_d && (rc = h->cov_ws.reserve(h, (size_t)chunk * z_one * sizeof(T)))) return rc;
  const int64_t ntiles = (N + kCovTile - 1) / kCovTile, npairs = ntiles * (ntiles + 1) / 2;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, B - b0);
    if (with_image) a.img = MargImages<T>::launch(h, U + b0 * strideU, ldu, strideU, (int)D, (const int32_t*)(info_d + b0), 0, nb);
    const int64_t ngroups = tile_groups(h, ntiles, nb);
    a.X = X_d; a.s = s_d; a.mw = mw_d; a.dprior = kind == BLR_PRIOR_DIAGONAL ? U : nullptr; a.stridedp = strideU;
    a.info = info_d; a.mean = mean_d; a.C = C_d; a.Z = C_d ? reinterpret_cast<T*>(h->cov_ws.p) : nullptr;
    a.ngroups = (int)ngroups; a.reg0 = (int)b0;
    hipLaunchKernelGGL(whiten, dim3((unsigned)ngroups, (unsigned)nb), dim3(kThreads), lds_w, h->stream, a);
    if (C_d) hipLaunchKernelGGL(cov_tiles_kernel<T>, dim3((unsigned)npairs, (unsigned)nb), dim3(kThreads), lds_t, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- exact leave-one-out predictives of a batched multi-output state: S columns, one leverage per input (blr_loo_multi_batched_*,
// DESIGN.md K20; blr_loo_multi.hpp) -------------------------------------------------------------------------------------------------

template <typename T>
int loo_multi_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, const T* X, int64_t ldx,
                      int64_t strideX, const T* Y, int64_t ldY, int64_t strideY, int noise_kind, const T* s, int64_t strides, const T* M,
                      int64_t ldm, int64_t strideM, const T* Tf, int64_t ldt, int64_t strideT, T* loo_mean, int64_t ld_lm, int64_t stride_lm,
                      T* loo_var, int64_t stride_lv, double* loo_logpdf, int64_t ld_ll, int64_t stride_ll, double* loo_total, int64_t stride_lt,
                      int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range (0..2^30)");
  if (S < 0 || S > (1 << 20)) return bad_arg(h, 7, "S out of range (0..2^20)");
  if (B == 0 || S == 0) return 0;
  if (N > 0 && !X) return bad_arg(h, 8, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(N, 1)) return bad_arg(h, 9, "ldx too small");
  if (strideX < 0) return bad_arg(h, 10, "strideX < 0");
  if (N > 0 && !Y) return bad_arg(h, 11, "Y is NULL (reference :74 length check)");
  if (ldY < N) return bad_arg(h, 12, "ldY < N");
  if (strideY < 0) return bad_arg(h, 13, "strideY < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 14, "noise_kind (dense noise has no single-observation LOO: that is a block LOO)");
  if (N > 0 && !s) return bad_arg(h, 15, "s is NULL");
  if (strides < 0) return bad_arg(h, 16, "strides < 0");
  if (!M) return bad_arg(h, 17, "M is NULL");
  if (ldm < D) return bad_arg(h, 18, "ldm < D");
  if (strideM < 0) return bad_arg(h, 19, "strideM < 0");
  if (!Tf) return bad_arg(h, 20, "T is NULL");
  if (ldt < D) return bad_arg(h, 21, "ldt < D");
  if (strideT < 0) return bad_arg(h, 22, "strideT < 0");
  if (loo_mean && ld_lm < N) return bad_arg(h, 24, "ld_lm < N");
  if (loo_mean && B > 1 && stride_lm < ld_lm * S) return bad_arg(h, 25, "stride_lm < ld_lm * S");
  if (loo_var && B > 1 && stride_lv < N) return bad_arg(h, 27, "stride_lv < N");
  if (loo_logpdf && ld_ll < N) return bad_arg(h, 29, "ld_ll < N");
  if (loo_logpdf && B > 1 && stride_ll < ld_ll * S) return bad_arg(h, 30, "stride_ll < ld_ll * S");
  if (loo_total && B > 1 && stride_lt < S) return bad_arg(h, 32, "stride_lt < S");
  if (!info) return bad_arg(h, 33, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  LooColsArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.ldY = ldY; a.strideY = strideY; a.strides = strides; a.ldm = ldm; a.strideM = strideM;
  a.ld_lm = ld_lm; a.stride_lm = stride_lm; a.stride_lv = stride_lv; a.ld_ll = ld_ll; a.stride_ll = stride_ll;
  a.noise_kind = noise_kind; a.D = (int)D; a.N = (int)N; a.S = (int)S;
  const T* T_d = nullptr;
  double* tot_d = nullptr;
  int32_t* info_d = nullptr;
  int rc;
  if ((rc = heldout_stage_in<T>(io, layout, noise_kind, B, D, N, S, {X, ldx, strideX, &a.X}, {Y, ldY, strideY, &a.Y}, {s, 0, strides, &a.s},
                                {M, ldm, strideM, &a.M}, {Tf, ldt, strideT, &T_d}))) return rc;
  if ((rc = heldout_stage_out<T>(io, B, N, S, N, {loo_mean, ld_lm, stride_lm, &a.lm}, {loo_var, 0, stride_lv, &a.lv}, {loo_logpdf, ld_ll, stride_ll, &a.ll},
                                 {loo_total, 0, stride_lt, &tot_d}, info, &info_d))) return rc;
  a.info = info_d;
  if ((rc = ensure_stats(h))) return rc;
  a.degenerate = h->stats_dev + 3;

  const int64_t ychunk = heldout_status<T>(h, B, D, N, T_d, ldt, strideT, a.s, strides, noise_kind, info_d);
  h->count_chunks(B, ychunk);
  HIP_TRY(h, hipGetLastError());
  if (N == 0) return (rc = heldout_empty_totals(h, B, ychunk, true, S, tot_d, stride_lt, info_d)) ? rc : io.finish();

  // chunks of regressors: grid.y, the images (D <= 128) and the per-chunk intermediates each within their bound
  const bool small = D <= kMaxSmallD;
  const LogpdfSpill spill(tot_d, a.ll, N, S);
  const size_t item = sizeof(T), row = ((size_t)N * item + 255) & ~(size_t)255;
  const size_t per = (small ? 0 : (1 + (size_t)S) * row + sizeof(int32_t)) + spill.per;
  const int64_t chunk = whitened_chunk<T>(h, B, small, 0, per);
  const size_t off_mean = (size_t)chunk * row;                                  // (D > 128) var first, then the means
  const size_t off_ll = small ? 0 : off_mean + (size_t)chunk * S * row;
  const size_t off_zero = off_ll + (size_t)chunk * spill.per, off_inf = off_zero + 256;
  if (per && (rc = h->loo_ws.reserve(h, off_inf + (size_t)chunk * sizeof(int32_t) + 256))) return rc;
  char* const ws = h->loo_ws.p;
  const int64_t ldw = (int64_t)(row / item);
  const size_t lds = loo_cols_lds_bytes(sizeof(T), (int)D);
  void (*const kern)(LooColsArgs<T>) = layout == BLR_LAYOUT_ROWVECS ? loo_cols_kernel<T, LAYOUT_ROWVECS> : loo_cols_kernel<T, LAYOUT_COLVECS>;
  if (small) {
    if ((rc = set_lds_once(h, kern, lds))) return rc;
    if ((rc = MargImages<T>::reserve(h, chunk))) return rc;
  } else {
    HIP_TRY(h, hipMemsetAsync(ws + off_zero, 0, sizeof(T), h->stream));  // the variance route's zero noise
  }
  const int64_t ntiles = (N + kMargTile - 1) / kMargTile;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, B - b0);
    LooColsArgs<T> c = a;
    c.reg0 = (int)b0;
    if (spill.on) { c.ld_ll = spill.ld; c.stride_ll = spill.ld * S; c.ll = spill.rows(ws + off_ll, b0); }
    if (small) {
      // L^-T of every factor as an MFMA image (marg_image_kernel, the existing instantiation), then ONE launch over (tile groups, regressors)
      c.img = MargImages<T>::launch(h, T_d + b0 * strideT, ldt, strideT, (int)D, (const int32_t*)(info_d + b0), 0, nb);
      c.ngroups = (int)tile_groups(h, ntiles, nb);
      hipLaunchKernelGGL(kern, dim3((unsigned)c.ngroups, (unsigned)nb), dim3(kThreads), lds, h->stream, c);
    } else {
      // correct, not fast: the LATENT variance (zero noise) of the chunk by the large-D route of blr_marginals_batched_*, the means one
      // regressor after the other as X'M (launch_project), then the epilogue.  A state that failed the check is skipped by the finish.
      T* const var = reinterpret_cast<T*>(ws);
      T* const mean = reinterpret_cast<T*>(ws + off_mean);
      // (mw is not read without a mean; X stands in as a non-NULL pointer)
      rc = heldout_latent_marginals<T>(h, layout, nb, D, N, a.X + b0 * strideX, ldx, strideX, reinterpret_cast<const T*>(ws + off_zero), a.X, 0,
                                       T_d + b0 * strideT, ldt, strideT, (T*)nullptr, var, ldw, reinterpret_cast<int32_t*>(ws + off_inf));
      if (rc) return rc;
      for (int64_t b = 0; b < nb; ++b)
        launch_project<T>(h, layout, D, N, S, a.X + (b0 + b) * strideX, ldx, a.M + (b0 + b) * strideM, ldm, (const T*)nullptr, BLR_NOISE_ISOTROPIC,
                          (const T*)nullptr, 0, mean + b * S * ldw, ldw);
      const int64_t gx = std::max<int64_t>(1, std::min<int64_t>((N + kThreads - 1) / kThreads, (4 * (int64_t)h->cus + nb - 1) / nb));
      hipLaunchKernelGGL(loo_cols_finish_kernel<T>, dim3((unsigned)gx, (unsigned)nb), dim3(kThreads), 0, h->stream, c, (const T*)mean, ldw, S * ldw,
                         (const T*)var, ldw);
    }
    if (tot_d) heldout_cols_totals(h, b0, nb, S, c.ll, c.ld_ll, c.stride_ll, N, tot_d, stride_lt, info_d);
    HIP_TRY(h, hipGetLastError());
  }
  h->count_chunks(B, chunk);  // (after the loop: the large-D route's marginals count their own)
  return io.finish();
}

// ---- exact leave-fold-out predictives of a state's observations, contiguous folds of F <= 64 (blr_kfold_batched_*, DESIGN.md K23;
// blr_kfold.hpp) ---------------------------------------------------------------------------------------------------------------------

template <typename T>
int kfold_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t F, const T* X, int64_t ldx, int64_t strideX,
                  const T* y, int64_t stridey, int noise_kind, const T* s, int64_t strides, const T* mw, int64_t stridemw, const T* Tf,
                  int64_t ldt, int64_t strideT, T* kf_mean, int64_t stride_km, T* kf_var, int64_t stride_kv, double* kf_logpdf,
                  int64_t stride_kl, double* kf_total, int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range (0..2^30)");
  if (D > kMaxSmallD && N > kMaxDenseN) return bad_arg(h, 6, "N out of range at D > 128: the route goes through an N x N covariance (0..16384)");
  if (F < 1 || F > kFoldMax) return bad_arg(h, 7, "F out of range (1..64)");
  if (N > 0 && !X) return bad_arg(h, 8, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(N, 1)) return bad_arg(h, 9, "ldx too small");
  if (strideX < 0) return bad_arg(h, 10, "strideX < 0");
  if (N > 0 && !y) return bad_arg(h, 11, "y is NULL (reference :74 length check)");
  if (stridey < 0) return bad_arg(h, 12, "stridey < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 13, "noise_kind (dense noise couples the folds: isotropic or diagonal only)");
  if (N > 0 && !s) return bad_arg(h, 14, "s is NULL");
  if (strides < 0) return bad_arg(h, 15, "strides < 0");
  if (!mw) return bad_arg(h, 16, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 17, "stridemw < 0");
  if (!Tf) return bad_arg(h, 18, "T is NULL");
  if (ldt < D) return bad_arg(h, 19, "ldt < D");
  if (strideT < 0) return bad_arg(h, 20, "strideT < 0");
  const int64_t nfolds = (N + F - 1) / F;
  if (kf_mean && B > 1 && stride_km < N) return bad_arg(h, 22, "stride_km < N");
  if (kf_var && B > 1 && stride_kv < N) return bad_arg(h, 24, "stride_kv < N");
  if (kf_logpdf && B > 1 && stride_kl < nfolds) return bad_arg(h, 26, "stride_kl < ceil(N / F)");
  if (!info) return bad_arg(h, 28, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  if (B == 0) return 0;
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  KfoldArgs<T> k{};
  k.stridey = stridey; k.strides = strides; k.noise_kind = noise_kind; k.stride_km = stride_km; k.stride_kv = stride_kv;
  k.stride_kl = stride_kl; k.D = (int)D; k.N = (int)N; k.F = (int)F;
  int rc;
  const T *X_d = nullptr, *mw_d = nullptr, *T_d = nullptr;
  double* tot_d = nullptr;
  int32_t* info_d = nullptr;
  if ((rc = heldout_stage_in<T>(io, layout, noise_kind, B, D, N, 1, {X, ldx, strideX, &X_d}, {y, N, stridey, &k.y}, {s, 0, strides, &k.s},
                                {mw, D, stridemw, &mw_d}, {Tf, ldt, strideT, &T_d}))) return rc;
  if ((rc = heldout_stage_out<T>(io, B, N, 1, nfolds, {kf_mean, N, stride_km, &k.km}, {kf_var, 0, stride_kv, &k.kv}, {kf_logpdf, nfolds, stride_kl, &k.kl},
                                 {kf_total, 0, 1, &tot_d}, info, &info_d))) return rc;
  k.info = info_d;
  if ((rc = ensure_stats(h))) return rc;
  k.degenerate = h->stats_dev + 4;

  const int64_t ychunk = heldout_status<T>(h, B, D, N, T_d, ldt, strideT, k.s, strides, noise_kind, info_d);
  h->count_chunks(B, ychunk);
  HIP_TRY(h, hipGetLastError());
  if (N == 0) return (rc = heldout_empty_totals(h, B, ychunk, false, 1, tot_d, 1, info_d)) ? rc : io.finish();
  const int64_t pack_rows = (kFoldMax / F) * F, npacks = (N + pack_rows - 1) / pack_rows;
  const size_t lds_k = kfold_lds_bytes(sizeof(T), (int)std::min<int64_t>(D, kMaxSmallD));
  if ((rc = set_lds_once(h, kfold_kernel<T>, lds_k))) return rc;
  const LogpdfSpill spill(tot_d, k.kl, nfolds);

  if (D > kMaxSmallD) {
    // correct, not fast: one regressor after the other through the launches of blr_mean_and_cov_* (mean_and_cov_core) into a staging
    // covariance C = Z Z' + diag(s), whose diagonal blocks the fold kernel reads instead of forming the product; the call synchronises
    std::vector<int32_t> st((size_t)B, 0);
    HIP_TRY(h, hipMemcpyAsync(st.data(), info_d, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    CovTemps<T> t;
    T *Ct = nullptr, *mt = nullptr;
    double* klt = nullptr;
    int32_t* it = nullptr;
    if ((rc = t.reserve(io, (int)D, (int)N))) return rc;
    if ((rc = io.tmp((size_t)N * N, &Ct))) return rc;
    if ((rc = io.tmp((size_t)N, &mt))) return rc;
    if ((rc = io.tmp(1, &it))) return rc;
    if (spill.on && (rc = io.tmp((size_t)nfolds, &klt))) return rc;
    for (int64_t b = 0; b < B; ++b) {
      if (st[(size_t)b] != 0) continue;  // outputs of that regressor stay untouched
      rc = mean_and_cov_core<T>(h, t, layout, (int)D, (int)N, X_d + b * strideX, ldx, noise_kind, k.s + b * strides, 0, BLR_PRIOR_UPPER_FACTOR,
                                mw_d + b * stridemw, T_d + b * strideT, ldt, mt, Ct, N, it);
      if (rc) return rc;
      KfoldArgs<T> c = k;
      c.C = Ct; c.ldc = N; c.m = mt; c.stridem = 0; c.reg0 = (int)b;
      if (spill.on) { c.kl = klt; c.stride_kl = 0; }
      hipLaunchKernelGGL(kfold_kernel<T>, dim3((unsigned)npacks, 1), dim3(kThreads), lds_k, h->stream, c);
      if (tot_d) heldout_totals(h, b, 1, c.kl, c.stride_kl, nfolds, tot_d, info_d);
      HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return io.finish();
  }

  // D <= 128.  Per chunk of regressors: the triangular inverses as MFMA images (marg_image_kernel), Z = X'T^-1 and x'mw into workspace
  // (cov_whiten_kernel), the folds (kfold_kernel), the totals -- four launches whatever B.  Chunks by the rules of
  // blr_mean_and_cov_batched_*: grid.y, the images and the rows of Z within 256 MiB each, the means (and the folds' log densities when
  // only the totals are wanted) within theirs, at least one regressor
  const size_t z_one = cov_z_elems((int)D, (int)N);
  const size_t row = ((size_t)N * sizeof(T) + 255) & ~(size_t)255, per = row + spill.per;
  const int64_t chunk = whitened_chunk<T>(h, B, true, z_one, per);
  h->count_chunks(B, chunk);
  const size_t lds_w = cov_whiten_lds_bytes(sizeof(T), (int)D, true);
  void (*const whiten)(CovArgs<T>) = layout == BLR_LAYOUT_ROWVECS ? cov_whiten_kernel<T, LAYOUT_ROWVECS> : cov_whiten_kernel<T, LAYOUT_COLVECS>;
  if ((rc = set_lds_once(h, whiten, lds_w))) return rc;
  if ((rc = MargImages<T>::reserve(h, chunk))) return rc;
  if ((rc = h->cov_ws.reserve(h, (size_t)chunk * z_one * sizeof(T)))) return rc;
  if ((rc = h->loo_ws.reserve(h, (size_t)chunk * per + 256))) return rc;
  char* const ws = h->loo_ws.p;
  const int64_t ldw = (int64_t)(row / sizeof(T));
  const int64_t ntiles = (N + kCovTile - 1) / kCovTile;
  CovArgs<T> a{};
  a.X = X_d; a.ldx = ldx; a.strideX = strideX; a.mw = mw_d; a.stridemw = stridemw; a.info = info_d; a.stridemean = ldw;
  a.noise_kind = noise_kind; a.prior_kind = BLR_PRIOR_UPPER_FACTOR; a.D = (int)D; a.N = (int)N;
  a.Z = reinterpret_cast<T*>(h->cov_ws.p);
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, B - b0);
    a.img = MargImages<T>::launch(h, T_d + b0 * strideT, ldt, strideT, (int)D, (const int32_t*)(info_d + b0), 0, nb);
    a.mean = reinterpret_cast<T*>(ws) - b0 * ldw;  // (indexed by the global regressor)
    a.ngroups = (int)tile_groups(h, ntiles, nb); a.reg0 = (int)b0;
    hipLaunchKernelGGL(whiten, dim3((unsigned)a.ngroups, (unsigned)nb), dim3(kThreads), lds_w, h->stream, a);
    KfoldArgs<T> c = k;
    c.Z = a.Z; c.strideZ = (int64_t)z_one; c.m = a.mean; c.stridem = ldw; c.reg0 = (int)b0;
    if (spill.on) { c.kl = spill.rows(ws + (size_t)chunk * row, b0); c.stride_kl = spill.ld; }
    hipLaunchKernelGGL(kfold_kernel<T>, dim3((unsigned)npacks, (unsigned)nb), dim3(kThreads), lds_k, h->stream, c);
    if (tot_d) heldout_totals(h, b0, nb, c.kl, c.stride_kl, nfolds, tot_d, info_d);
    HIP_TRY(h, hipGetLastError());
  }
  return io.finish();
}

// ---- leave-fold-out predictives of regressors with unequal observation counts (blr_kfold_ragged_*; blr_kfold_ragged.hpp,
// blr_kfold_ragged_plan.hpp) ---------------------------------------------------------------------------------------------------------
// the arguments blr_kfold_ragged_fold_offsets shares with the entry points, at their positions there
inline int kfold_ragged_shape_check(blr_handle* h, int64_t B, const int64_t* offsets, int64_t F) {
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (const int rc = ragged_offsets_check(h, B, offsets)) return rc;
  if (F < 1 || F > kFoldMax) return bad_arg(h, 7, "F out of range (1..64)");
  return 0;
}

template <typename T>
int kfold_ragged(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, int64_t F, const T* X, int64_t ldx,
                 const T* y, int noise_kind, const T* s, int64_t strides, const T* mw, int64_t stridemw, const T* Tf, int64_t ldt,
                 int64_t strideT, T* kf_mean, T* kf_var, double* kf_logpdf, double* kf_total, int32_t* info) {
  RaggedFront f;
  const auto mid = [&] {  // (F sits at position 7: X and ldx one later than in the other entry points)
    for (int64_t b = 0; D > kMaxSmallD && b < B; ++b)
      if (offsets[b + 1] - offsets[b] > kMaxDenseN)
        return bad_arg(h, 6, "a regressor with more than 16384 observations at D > 128: the route goes through an N x N covariance");
    return F < 1 || F > kFoldMax ? bad_arg(h, 7, "F out of range (1..64)") : 0;
  };
  if (const int rc = ragged_front(h, f, memspace, layout, B, D, offsets, X, ldx, noise_kind, strides, 8, mid)) return rc;
  const bool any = f.any, colv = f.colv, diag = f.diag;
  if (any && !y) return bad_arg(h, 10, "y is NULL (reference :74 length check)");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 11, "noise_kind (dense noise couples the folds: isotropic or diagonal only)");
  if (any && !s) return bad_arg(h, 12, "s is NULL");
  if (strides < 0) return bad_arg(h, 13, "strides < 0");
  if (!mw) return bad_arg(h, 14, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 15, "stridemw < 0");
  if (!Tf) return bad_arg(h, 16, "T is NULL");
  if (ldt < D) return bad_arg(h, 17, "ldt < D");
  if (strideT < 0) return bad_arg(h, 18, "strideT < 0");
  if (B > 0 && !info) return bad_arg(h, 23, "info is NULL");
  if (B == 0) return 0;
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  KfoldRaggedPlan plan;  // (D > 128: only its fold offsets are used)
  plan_kfold_ragged(offsets, B, F, (int)std::min<int64_t>(D, kMaxSmallD), h->cus, (int)sizeof(T), h->opt, plan);
  const std::vector<int64_t>& fo = plan.fold_offsets;

  CallIO io(h, memspace);
  KfoldRaggedArgs<T> a{};
  a.ldx = ldx; a.strides = strides; a.noise_kind = noise_kind; a.stridemw = stridemw; a.D = (int)D; a.F = (int)F;
  const size_t n_all = f.n_all, nf_all = (size_t)fo[(size_t)B];
  const T* T_d = nullptr;
  double* total_dev = nullptr;
  int32_t* info_dev = nullptr;
  int rc;
  if ((rc = io.in(X, f.x_all, &a.X))) return rc;
  if ((rc = io.in(y, n_all, &a.y))) return rc;
  if ((rc = io.in(s, any ? f.s_all : 0, &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Tf, extent(B, strideT, mat_extent(D, D, ldt)), &T_d))) return rc;
  if ((rc = io.out(kf_mean, n_all, &a.km))) return rc;
  if ((rc = io.out(kf_var, n_all, &a.kv))) return rc;
  if ((rc = io.out(kf_logpdf, nf_all, &a.kl))) return rc;
  if ((rc = io.out(kf_total, (size_t)B, &total_dev))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_dev))) return rc;
  if (!a.s) a.s = a.mw;  // (no observation at all: never dereferenced, but a valid pointer)
  if (D > kMaxSmallD) {  // through blr_kfold_batched_*
    if ((rc = ragged_one_by_one(h, B, offsets, [&](int64_t b, int64_t o, int64_t n) {
           return kfold_batched<T>(h, BLR_MEM_DEVICE, layout, 1, D, n, F, a.X ? a.X + (colv ? o * ldx : o) : (const T*)nullptr, ldx, 0,
                                   a.y ? a.y + o : (const T*)nullptr, 0, noise_kind, diag ? a.s + o : a.s + b * strides, 0, a.mw + b * stridemw, 0,
                                   T_d + b * strideT, ldt, 0, a.km ? a.km + o : (T*)nullptr, 0, a.kv ? a.kv + o : (T*)nullptr, 0,
                                   a.kl ? a.kl + fo[(size_t)b] : (double*)nullptr, 0, total_dev ? total_dev + b : (double*)nullptr, info_dev + b);
         })))
      return rc;
    h->last_chunks = 1;
    return io.finish();
  }
  if ((rc = ensure_stats(h))) return rc;
  a.degenerate = h->stats_dev + 4;
  a.info = info_dev;

  // offsets, the two tables and the items
  {
    const size_t tbl = ragged_table_bytes(B);
    const char* dev[4];
    if ((rc = ragged_meta_upload(h, {{offsets, tbl}, {plan.pack_offsets.data(), tbl}, {fo.data(), tbl},
                                     {plan.items.data(), plan.items.size() * sizeof(RaggedItem)}}, dev)))
      return rc;
    a.offsets = reinterpret_cast<const int64_t*>(dev[0]);
    a.pack_offsets = reinterpret_cast<const int64_t*>(dev[1]);
    a.fold_offsets = reinterpret_cast<const int64_t*>(dev[2]);
    a.items = reinterpret_cast<const RaggedItem*>(dev[3]);
  }
  const int64_t ychunk = heldout_ragged_status<T>(h, B, D, T_d, ldt, strideT, a.s, strides, noise_kind, a.offsets, info_dev);
  HIP_TRY(h, hipGetLastError());
  const bool folds = any && (a.km || a.kv || a.kl || total_dev);
  if (folds) {
    const int DP = 16 * (((int)D + 15) / 16);
    const size_t m_bytes = ((size_t)plan.max_rows * sizeof(T) + 255) & ~(size_t)255;
    const size_t lds_w = cov_whiten_lds_bytes(sizeof(T), (int)D, true), lds_k = kfold_lds_bytes(sizeof(T), (int)D);
    void (*const whiten)(KfoldRaggedArgs<T>) = colv ? kfold_ragged_whiten_kernel<T, LAYOUT_COLVECS> : kfold_ragged_whiten_kernel<T, LAYOUT_ROWVECS>;
    if ((rc = set_lds_once(h, whiten, lds_w))) return rc;
    if ((rc = set_lds_once(h, kfold_ragged_kernel<T>, lds_k))) return rc;
    if ((rc = MargImages<T>::reserve(h, plan.max_nb))) return rc;
    if ((rc = h->cov_ws.reserve(h, (size_t)plan.max_rows * DP * sizeof(T) + 256))) return rc;
    if ((rc = heldout_ragged_spill(h, total_dev, m_bytes, nf_all, 0, 256, &a.kl))) return rc;  // (m in front of the spill)
    a.Z = reinterpret_cast<T*>(h->cov_ws.p);
    a.m = reinterpret_cast<T*>(h->loo_ws.p);
    const RaggedItem* const items = a.items;
    for (const RaggedChunk& c : plan.chunks) {
      if (c.nitems == 0) continue;  // (no observation in the chunk)
      const int64_t npacks = plan.pack_offsets[(size_t)(c.b0 + c.nb)] - plan.pack_offsets[(size_t)c.b0];
      a.items = items + c.item0;
      a.b0 = (int)c.b0; a.nb = (int)c.nb;
      a.img = MargImages<T>::launch(h, T_d, ldt, strideT, (int)D, (const int32_t*)info_dev, c.b0, c.nb);
      hipLaunchKernelGGL(whiten, dim3((unsigned)c.nitems), dim3(kThreads), lds_w, h->stream, a);
      hipLaunchKernelGGL(kfold_ragged_kernel<T>, dim3((unsigned)npacks), dim3(kThreads), lds_k, h->stream, a);
      HIP_TRY(h, hipGetLastError());
    }
    h->route = "kfold_ragged_kernel";
    h->route_i8_B = 0;
  }
  h->last_chunks = std::max<int64_t>(1, plan.last_chunks);
  if (total_dev) heldout_ragged_totals(h, B, ychunk, a.kl, a.fold_offsets, total_dev, info_dev);
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- exact leave-fold-out predictives of a batched multi-output state: S columns, one fold factor per fold (blr_kfold_multi_batched_*,
// DESIGN.md K25; blr_kfold_multi.hpp) ------------------------------------------------------------------------------------------------

template <typename T>
int kfold_multi_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, int64_t F, const T* X, int64_t ldx,
                        int64_t strideX, const T* Y, int64_t ldY, int64_t strideY, int noise_kind, const T* s, int64_t strides, const T* M,
                        int64_t ldm, int64_t strideM, const T* Tf, int64_t ldt, int64_t strideT, T* kf_mean, int64_t ld_km, int64_t stride_km,
                        T* kf_var, int64_t stride_kv, double* kf_logpdf, int64_t ld_kl, int64_t stride_kl, double* kf_total, int64_t stride_kt,
                        int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxSmallD) return bad_arg(h, 5, "D out of range (1..128): the fold's rows of Z live in LDS, there is no slow route");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range (0..2^30)");
  if (S < 0 || S > (1 << 20)) return bad_arg(h, 7, "S out of range (0..2^20)");
  const int64_t ldmn = (N + kCovTile - 1) / kCovTile * kCovTile;  // a column of the means workspace
  if (S * ldmn > ((int64_t)1 << 28)) return bad_arg(h, 7, "S * 64 ceil(N / 64) > 2^28: the means workspace of one regressor");
  if (F < 1 || F > kFoldMax) return bad_arg(h, 8, "F out of range (1..64)");
  if (B == 0 || S == 0) return 0;
  if (N > 0 && !X) return bad_arg(h, 9, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(N, 1)) return bad_arg(h, 10, "ldx too small");
  if (strideX < 0) return bad_arg(h, 11, "strideX < 0");
  if (N > 0 && !Y) return bad_arg(h, 12, "Y is NULL (reference :74 length check)");
  if (ldY < N) return bad_arg(h, 13, "ldY < N");
  if (strideY < 0) return bad_arg(h, 14, "strideY < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 15, "noise_kind (dense noise couples the folds: isotropic or diagonal only)");
  if (N > 0 && !s) return bad_arg(h, 16, "s is NULL");
  if (strides < 0) return bad_arg(h, 17, "strides < 0");
  if (!M) return bad_arg(h, 18, "M is NULL");
  if (ldm < D) return bad_arg(h, 19, "ldm < D");
  if (strideM < 0) return bad_arg(h, 20, "strideM < 0");
  if (!Tf) return bad_arg(h, 21, "T is NULL");
  if (ldt < D) return bad_arg(h, 22, "ldt < D");
  if (strideT < 0) return bad_arg(h, 23, "strideT < 0");
  const int64_t nfolds = (N + F - 1) / F;
  if (kf_mean && ld_km < N) return bad_arg(h, 25, "ld_km < N");
  if (kf_mean && B > 1 && stride_km < ld_km * S) return bad_arg(h, 26, "stride_km < ld_km * S");
  if (kf_var && B > 1 && stride_kv < N) return bad_arg(h, 28, "stride_kv < N");
  if (kf_logpdf && ld_kl < nfolds) return bad_arg(h, 30, "ld_kl < ceil(N / F)");
  if (kf_logpdf && B > 1 && stride_kl < ld_kl * S) return bad_arg(h, 31, "stride_kl < ld_kl * S");
  if (kf_total && B > 1 && stride_kt < S) return bad_arg(h, 33, "stride_kt < S");
  if (!info) return bad_arg(h, 34, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  KfoldWhitenArgs<T> a{};
  KfoldColsArgs<T> k{};
  a.ldx = ldx; a.strideX = strideX; a.ldm = ldm; a.strideM = strideM; a.ldmn = ldmn; a.D = (int)D; a.N = (int)N; a.S = (int)S;
  k.ldmn = ldmn; k.ldY = ldY; k.strideY = strideY; k.strides = strides; k.noise_kind = noise_kind; k.ld_km = ld_km; k.stride_km = stride_km;
  k.stride_kv = stride_kv; k.ld_kl = ld_kl; k.stride_kl = stride_kl; k.D = (int)D; k.N = (int)N; k.F = (int)F; k.S = (int)S;
  const T* T_d = nullptr;
  double* tot_d = nullptr;
  int32_t* info_d = nullptr;
  int rc;
  if ((rc = heldout_stage_in<T>(io, layout, noise_kind, B, D, N, S, {X, ldx, strideX, &a.X}, {Y, ldY, strideY, &k.Y}, {s, 0, strides, &k.s},
                                {M, ldm, strideM, &a.M}, {Tf, ldt, strideT, &T_d}))) return rc;
  if ((rc = heldout_stage_out<T>(io, B, N, S, nfolds, {kf_mean, ld_km, stride_km, &k.km}, {kf_var, 0, stride_kv, &k.kv}, {kf_logpdf, ld_kl, stride_kl, &k.kl},
                                 {kf_total, 0, stride_kt, &tot_d}, info, &info_d))) return rc;
  a.info = info_d; k.info = info_d;
  if ((rc = ensure_stats(h))) return rc;
  k.degenerate = h->stats_dev + 4;

  const int64_t ychunk = heldout_status<T>(h, B, D, N, T_d, ldt, strideT, k.s, strides, noise_kind, info_d);
  h->count_chunks(B, ychunk);
  HIP_TRY(h, hipGetLastError());
  if (N == 0) return (rc = heldout_empty_totals(h, B, ychunk, true, S, tot_d, stride_kt, info_d)) ? rc : io.finish();

  // Per chunk of regressors: the triangular inverses as MFMA images (marg_image_kernel), Z = X'T^-1 and the S means X'M into workspace
  // (kfold_whiten_cols_kernel), the folds (kfold_cols_kernel), the totals -- four launches whatever B, S and the fold count.  Chunks by
  // the rules of blr_kfold_batched_*: grid.y, the images, the rows of Z and the means (with the log densities when only the totals are
  // wanted) within 256 MiB each, at least one regressor
  const LogpdfSpill spill(tot_d, k.kl, nfolds, S);
  const bool do_cols = k.km || k.kl || spill.on;
  const int64_t pack_rows = (kFoldMax / F) * F, npacks = (N + pack_rows - 1) / pack_rows;
  const size_t z_one = cov_z_elems((int)D, (int)N);
  const size_t mean_one = do_cols ? (size_t)S * (size_t)ldmn * sizeof(T) : 0;
  const size_t per = mean_one + spill.per;
  const int64_t chunk = whitened_chunk<T>(h, B, true, z_one, per);
  h->count_chunks(B, chunk);
  const size_t lds_w = kfold_whiten_cols_lds_bytes(sizeof(T), (int)D), lds_k = kfold_cols_lds_bytes(sizeof(T), (int)D);
  void (*const whiten)(KfoldWhitenArgs<T>) =
      layout == BLR_LAYOUT_ROWVECS ? kfold_whiten_cols_kernel<T, LAYOUT_ROWVECS> : kfold_whiten_cols_kernel<T, LAYOUT_COLVECS>;
  if ((rc = set_lds_once(h, whiten, lds_w))) return rc;
  if ((rc = set_lds_once(h, kfold_cols_kernel<T>, lds_k))) return rc;
  if ((rc = MargImages<T>::reserve(h, chunk))) return rc;
  if ((rc = h->cov_ws.reserve(h, (size_t)chunk * z_one * sizeof(T)))) return rc;
  if (per && (rc = h->loo_ws.reserve(h, (size_t)chunk * per + 256))) return rc;
  char* const ws = h->loo_ws.p;
  const int64_t ntiles = (N + kCovTile - 1) / kCovTile;
  a.Z = reinterpret_cast<T*>(h->cov_ws.p);
  a.mean = do_cols ? reinterpret_cast<T*>(ws) : nullptr;
  k.Z = a.Z; k.strideZ = (int64_t)z_one; k.mean = a.mean;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, B - b0);
    a.img = MargImages<T>::launch(h, T_d + b0 * strideT, ldt, strideT, (int)D, (const int32_t*)(info_d + b0), 0, nb);
    a.ngroups = (int)tile_groups(h, ntiles, nb); a.reg0 = (int)b0;
    hipLaunchKernelGGL(whiten, dim3((unsigned)a.ngroups, (unsigned)nb), dim3(kThreads), lds_w, h->stream, a);
    KfoldColsArgs<T> c = k;
    c.reg0 = (int)b0;
    if (spill.on) { c.ld_kl = spill.ld; c.stride_kl = spill.ld * S; c.kl = spill.rows(ws + (size_t)chunk * mean_one, b0); }
    hipLaunchKernelGGL(kfold_cols_kernel<T>, dim3((unsigned)npacks, (unsigned)nb), dim3(kThreads), lds_k, h->stream, c);
    if (tot_d) heldout_cols_totals(h, b0, nb, S, c.kl, c.ld_kl, c.stride_kl, nfolds, tot_d, stride_kt, info_d);
    HIP_TRY(h, hipGetLastError());
  }
  return io.finish();
}

// ---- exact leave-fold-out predictives for LARGE folds, removed in weight space (blr_kfold_large_batched_*, DESIGN.md K24;
// blr_kfold_large.hpp) ---------------------------------------------------------------------------------------------------------------

// statistics (+ reduce) and factorisation of one chunk: the launches that depend on the block count
template <typename T, int NB>
int kfold_large_nb(blr_handle* h, const KflArgs<T>& a, int64_t nb, bool vec_ok) {
  using C = SmallCfg<T, NB>;
  constexpr int SZ = kfl_stat_elems<T, NB>();
  int rc;
  void (*const factor)(KflArgs<T>) = kfl_factor_kernel<T, NB>;
  if ((rc = set_lds_once(h, factor, (size_t)C::LDS_BYTES))) return rc;
  const dim3 sgrid((unsigned)(a.nfolds * a.S), (unsigned)nb);
  if constexpr (sizeof(T) == sizeof(double)) {
    void (*const stats)(KflArgs<T>) = a.layout == BLR_LAYOUT_ROWVECS ? kfl_stats_kernel<T, NB, 1>
                                      : (vec_ok ? kfl_stats_kernel<T, NB, 4> : kfl_stats_kernel<T, NB, 0>);
    if ((rc = set_lds_once(h, stats, (size_t)C::LDS_BYTES))) return rc;
    hipLaunchKernelGGL(stats, sgrid, dim3(kThreads), C::LDS_BYTES, h->stream, a);
  } else {  // fp32: the statistics accumulated in double from the float rows (blr_kfold_large.hpp, kfl_stats32_kernel)
    void (*const stats)(KflArgs<T>) = a.layout == BLR_LAYOUT_ROWVECS ? kfl_stats32_kernel<LAYOUT_ROWVECS> : kfl_stats32_kernel<LAYOUT_COLVECS>;
    const size_t lds = kfl_stats32_lds_bytes(a.D);
    if ((rc = set_lds_once(h, stats, lds))) return rc;
    hipLaunchKernelGGL(stats, sgrid, dim3(kThreads), lds, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  if (a.S > 1) {
    hipLaunchKernelGGL(kfl_reduce_kernel<T>, dim3((unsigned)(nb * a.nfolds), 8), dim3(kThreads), 0, h->stream, a, SZ);
    HIP_TRY(h, hipGetLastError());
  }
  hipLaunchKernelGGL(factor, dim3((unsigned)a.nfolds, (unsigned)nb), dim3(kThreads), C::LDS_BYTES, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

template <typename T>
int kfold_large_batched(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t F, const T* X, int64_t ldx,
                        int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s, int64_t strides, const T* mw,
                        int64_t stridemw, const T* Tf, int64_t ldt, int64_t strideT, T* kf_mean, int64_t stride_km, T* kf_var,
                        int64_t stride_kv, double* kf_logpdf, int64_t stride_kl, double* kf_total, int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxSmallD) return bad_arg(h, 5, "D out of range (1..128)");
  if (N < 0 || N > (1 << 30)) return bad_arg(h, 6, "N out of range (0..2^30)");
  if (F < 1) return bad_arg(h, 7, "F < 1");
  const int64_t nfolds = N == 0 ? 0 : (F >= N ? 1 : (N + F - 1) / F);
  if (nfolds > kFoldLargeMaxFolds)
    return bad_arg(h, 7, "ceil(N / F) > 1024: this route is for few, large folds (many small ones: blr_kfold_batched_*)");
  if (N > 0 && !X) return bad_arg(h, 8, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(N, 1)) return bad_arg(h, 9, "ldx too small");
  if (strideX < 0) return bad_arg(h, 10, "strideX < 0");
  if (N > 0 && !y) return bad_arg(h, 11, "y is NULL (reference :74 length check)");
  if (stridey < 0) return bad_arg(h, 12, "stridey < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 13, "noise_kind (dense noise couples the folds: isotropic or diagonal only)");
  if (N > 0 && !s) return bad_arg(h, 14, "s is NULL");
  if (strides < 0) return bad_arg(h, 15, "strides < 0");
  if (!mw) return bad_arg(h, 16, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 17, "stridemw < 0");
  if (!Tf) return bad_arg(h, 18, "T is NULL");
  if (ldt < D) return bad_arg(h, 19, "ldt < D");
  if (strideT < 0) return bad_arg(h, 20, "strideT < 0");
  if (kf_mean && B > 1 && stride_km < N) return bad_arg(h, 22, "stride_km < N");
  if (kf_var && B > 1 && stride_kv < N) return bad_arg(h, 24, "stride_kv < N");
  if (kf_logpdf && B > 1 && stride_kl < nfolds) return bad_arg(h, 26, "stride_kl < ceil(N / F)");
  if (!info) return bad_arg(h, 28, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  if (B == 0) return 0;
  HIP_TRY(h, hipSetDevice(h->device));

  CallIO io(h, memspace);
  KflArgs<T> k{};
  k.ldx = ldx; k.strideX = strideX; k.stridey = stridey; k.strides = strides; k.stridemw = stridemw; k.ldt = ldt; k.strideT = strideT;
  k.stride_km = stride_km; k.stride_kv = stride_kv; k.stride_kl = stride_kl;
  k.layout = layout; k.noise_kind = noise_kind; k.D = (int)D; k.N = (int)N; k.F = (int)std::min<int64_t>(F, std::max<int64_t>(N, 1));
  k.nfolds = (int)nfolds;
  int rc;
  double* tot_d = nullptr;
  int32_t* info_d = nullptr;
  if ((rc = heldout_stage_in<T>(io, layout, noise_kind, B, D, N, 1, {X, ldx, strideX, &k.X}, {y, N, stridey, &k.y}, {s, 0, strides, &k.s},
                                {mw, D, stridemw, &k.mw}, {Tf, ldt, strideT, &k.Tf}))) return rc;
  if ((rc = heldout_stage_out<T>(io, B, N, 1, nfolds, {kf_mean, N, stride_km, &k.km}, {kf_var, 0, stride_kv, &k.kv}, {kf_logpdf, nfolds, stride_kl, &k.kl},
                                 {kf_total, 0, 1, &tot_d}, info, &info_d))) return rc;
  k.info = info_d;
  if ((rc = ensure_stats(h))) return rc;
  k.degenerate = h->stats_dev + 4;

  const int64_t ychunk = heldout_status<T>(h, B, D, N, k.Tf, ldt, strideT, k.s, strides, noise_kind, info_d);
  h->count_chunks(B, ychunk);
  HIP_TRY(h, hipGetLastError());
  if (N == 0) return (rc = heldout_empty_totals(h, B, ychunk, false, 1, tot_d, 1, info_d)) ? rc : io.finish();

  // Per chunk of regressors: the state matrix, the folds' statistics (+ reduce), their factors, the images of the factors, the
  // predictions, the totals -- the same launches whatever B and the fold count are.  Chunks: grid.y / grid.z <= 65535; the statistics,
  // the factors and the images within 256 MiB each; at least one regressor
  int S = 1, cols = 64;
  kfl_splits(k.F, &S, &cols);
  k.S = S;
  const int NB = (int)(D + 15) / 16, DP = 16 * NB;
  const size_t packed = (size_t)DP * (DP + 1) / 2, SZ = packed + DP;
  const size_t stats_one = (size_t)nfolds * S * SZ * sizeof(double), U_one = (size_t)nfolds * D * D * sizeof(T);
  const LogpdfSpill spill(tot_d, k.kl, nfolds, 1, sizeof(double));  // (rows of nfolds doubles, not padded, in cov_ws)
  const bool predict = k.km || k.kv;
  const size_t bound = (size_t)256 << 20;
  int64_t chunk = std::min<int64_t>(std::min<int64_t>(B, 65535), MargImages<T>::kMaxChunk / nfolds);
  chunk = std::min<int64_t>(chunk, (int64_t)(bound / stats_one));
  chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(bound / U_one)));
  chunk = h->cap_chunk(chunk);
  h->count_chunks(B, chunk);
  Carve carve;
  const size_t nrf = (size_t)chunk * nfolds;
  const size_t o_st = carve((size_t)chunk * stats_one), o_U = carve((size_t)chunk * U_one), o_A = carve((size_t)chunk * packed * sizeof(double));
  const size_t o_ld = carve((size_t)chunk * sizeof(double)), o_sc = carve(nrf * S * 2 * sizeof(double));
  const size_t o_mw = carve(nrf * D * sizeof(T)), o_fi = carve(nrf * sizeof(int32_t)), o_kl = carve((size_t)chunk * spill.per);
  if ((rc = h->cov_ws.reserve(h, carve.off))) return rc;
  char* const ws = h->cov_ws.p;
  k.stats = reinterpret_cast<double*>(ws + o_st); k.U = reinterpret_cast<T*>(ws + o_U); k.A = reinterpret_cast<double*>(ws + o_A);
  k.ldA = reinterpret_cast<double*>(ws + o_ld); k.scal = reinterpret_cast<double*>(ws + o_sc); k.mwf = reinterpret_cast<T*>(ws + o_mw);
  k.finfo = reinterpret_cast<int32_t*>(ws + o_fi);
  const size_t lds_s = kfl_state_lds_bytes(sizeof(T), (int)D), lds_p = kfl_predict_lds_bytes(sizeof(T), (int)D);
  void (*const pred)(KflArgs<T>) = layout == BLR_LAYOUT_ROWVECS ? kfl_predict_kernel<T, LAYOUT_ROWVECS> : kfl_predict_kernel<T, LAYOUT_COLVECS>;
  void (*const state)(KflArgs<T>) = kfl_state_kernel<T>;
  if ((rc = set_lds_once(h, state, lds_s))) return rc;
  if (predict && (rc = set_lds_once(h, pred, lds_p))) return rc;
  if (predict && (rc = MargImages<T>::reserve(h, chunk * nfolds))) return rc;
  const bool vec_ok = layout == BLR_LAYOUT_COLVECS && D % Mfma<T>::VEC == 0 && aligned16(k.X, ldx, strideX);
  const int64_t ntiles = ((int64_t)k.F + kCovTile - 1) / kCovTile;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, B - b0);
    KflArgs<T> c = k;
    c.reg0 = (int)b0;
    if (spill.on) { c.kl = spill.rows(ws + o_kl, b0); c.stride_kl = spill.ld; }
    hipLaunchKernelGGL(state, dim3((unsigned)nb), dim3(kThreads), lds_s, h->stream, c);
    HIP_TRY(h, hipGetLastError());
    switch (NB) {
      case 1: rc = kfold_large_nb<T, 1>(h, c, nb, vec_ok); break;
      case 2: rc = kfold_large_nb<T, 2>(h, c, nb, vec_ok); break;
      case 3: rc = kfold_large_nb<T, 3>(h, c, nb, vec_ok); break;
      case 4: rc = kfold_large_nb<T, 4>(h, c, nb, vec_ok); break;
      case 5: rc = kfold_large_nb<T, 5>(h, c, nb, vec_ok); break;
      case 6: rc = kfold_large_nb<T, 6>(h, c, nb, vec_ok); break;
      case 7: rc = kfold_large_nb<T, 7>(h, c, nb, vec_ok); break;
      default: rc = kfold_large_nb<T, 8>(h, c, nb, vec_ok); break;
    }
    if (rc) return rc;
    if (predict) {
      // the factors of the chunk's folds as images (a fold without a factor is skipped by its status word), then the folds' rows
      // against them
      c.img = MargImages<T>::launch(h, c.U, D, D * D, (int)D, (const int32_t*)c.finfo, 0, nb * nfolds);
      c.ngroups = (int)tile_groups(h, ntiles, nb * nfolds);
      hipLaunchKernelGGL(pred, dim3((unsigned)c.ngroups, (unsigned)nfolds, (unsigned)nb), dim3(kThreads), lds_p, h->stream, c);
    }
    if (tot_d) heldout_totals(h, b0, nb, c.kl, c.stride_kl, nfolds, tot_d, info_d);
    HIP_TRY(h, hipGetLastError());
  }
  return io.finish();
}

// ---- large folds of regressors with unequal observation counts and their own fold sizes (blr_kfold_large_ragged_*, DESIGN.md K28;
// blr_kfold_large_ragged.hpp, blr_kfold_large_ragged_plan.hpp) ------------------------------------------------------------------------
// the arguments the two host helpers share with the entry points, at their positions there
inline int kfold_large_ragged_sizes_check(blr_handle* h, int64_t B, const int64_t* offsets, const int64_t* fold_sizes) {
  if (B > 0 && !fold_sizes) return bad_arg(h, 7, "fold_sizes is NULL (a host array of B entries)");
  for (int64_t b = 0; b < B; ++b) {
    if (fold_sizes[b] < 1) return bad_arg(h, 7, "a fold size < 1");
    if (kflr_folds(offsets[b + 1] - offsets[b], fold_sizes[b]) > kFoldLargeMaxFolds)
      return bad_arg(h, 7, "ceil(N_b / F_b) > 1024: this route is for few, large folds (many small ones: blr_kfold_ragged_*)");
  }
  return 0;
}

// statistics (+ reduce) and factorisation of one chunk: the launches that depend on the block count (kfold_large_nb's, flat)
template <typename T, int NB>
int kfold_large_ragged_nb(blr_handle* h, KflrArgs<T> a, const KflrChunk& c, const KflrItem* stat, const KflrItem* red, bool vec_ok) {
  using C = SmallCfg<T, NB>;
  constexpr int SZ = kfl_stat_elems<T, NB>();
  int rc;
  void (*const factor)(KflrArgs<T>) = kflr_factor_kernel<T, NB>;
  if ((rc = set_lds_once(h, factor, (size_t)C::LDS_BYTES))) return rc;
  a.items = stat + c.stat0;
  if constexpr (sizeof(T) == sizeof(double)) {
    void (*const stats)(KflrArgs<T>) = a.layout == BLR_LAYOUT_ROWVECS ? kflr_stats_kernel<T, NB, 1>
                                       : (vec_ok ? kflr_stats_kernel<T, NB, 4> : kflr_stats_kernel<T, NB, 0>);
    if ((rc = set_lds_once(h, stats, (size_t)C::LDS_BYTES))) return rc;
    hipLaunchKernelGGL(stats, dim3((unsigned)c.nstat), dim3(kThreads), C::LDS_BYTES, h->stream, a);
  } else {
    void (*const stats)(KflrArgs<T>) = a.layout == BLR_LAYOUT_ROWVECS ? kflr_stats32_kernel<LAYOUT_ROWVECS> : kflr_stats32_kernel<LAYOUT_COLVECS>;
    const size_t lds = kfl_stats32_lds_bytes(a.D);
    if ((rc = set_lds_once(h, stats, lds))) return rc;
    hipLaunchKernelGGL(stats, dim3((unsigned)c.nstat), dim3(kThreads), lds, h->stream, a);
  }
  HIP_TRY(h, hipGetLastError());
  if (c.nred > 0) {
    a.items = red + c.red0;
    hipLaunchKernelGGL(kflr_reduce_kernel<T>, dim3((unsigned)c.nred), dim3(kThreads), 0, h->stream, a, SZ);
    HIP_TRY(h, hipGetLastError());
  }
  hipLaunchKernelGGL(factor, dim3((unsigned)c.nfolds), dim3(kThreads), C::LDS_BYTES, h->stream, a);
  HIP_TRY(h, hipGetLastError());
  return 0;
}

template <typename T>
int kfold_large_ragged(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, const int64_t* fold_sizes,
                       const T* X, int64_t ldx, const T* y, int noise_kind, const T* s, int64_t strides, const T* mw, int64_t stridemw,
                       const T* Tf, int64_t ldt, int64_t strideT, T* kf_mean, T* kf_var, double* kf_logpdf, double* kf_total, int32_t* info) {
  RaggedFront f;
  const auto mid = [&] { return kfold_large_ragged_sizes_check(h, B, offsets, fold_sizes); };  // (position 7: X and ldx one later)
  if (const int rc = ragged_front(h, f, memspace, layout, B, D, offsets, X, ldx, noise_kind, strides, 8, mid, kMaxSmallD, "D out of range (1..128)")) return rc;
  const bool any = f.any, colv = f.colv;
  if (any && !y) return bad_arg(h, 10, "y is NULL (reference :74 length check)");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 11, "noise_kind (dense noise couples the folds: isotropic or diagonal only)");
  if (any && !s) return bad_arg(h, 12, "s is NULL");
  if (strides < 0) return bad_arg(h, 13, "strides < 0");
  if (!mw) return bad_arg(h, 14, "mw is NULL");
  if (stridemw < 0) return bad_arg(h, 15, "stridemw < 0");
  if (!Tf) return bad_arg(h, 16, "T is NULL");
  if (ldt < D) return bad_arg(h, 17, "ldt < D");
  if (strideT < 0) return bad_arg(h, 18, "strideT < 0");
  if (B > 0 && !info) return bad_arg(h, 23, "info is NULL");
  if (B == 0) return 0;
  if (!h) return -1;
  h->last_chunks = 1;
  HIP_TRY(h, hipSetDevice(h->device));

  KflrPlan plan;
  plan_kfold_large_ragged(offsets, fold_sizes, B, (int)D, h->cus, (int)sizeof(T), h->opt, plan);
  const std::vector<int64_t>& fo = plan.fold_offsets;

  CallIO io(h, memspace);
  KflrArgs<T> a{};
  a.ldx = ldx; a.strides = strides; a.stridemw = stridemw; a.layout = layout; a.noise_kind = noise_kind; a.D = (int)D;
  const size_t n_all = f.n_all, nf_all = (size_t)fo[(size_t)B];
  const T* T_d = nullptr;
  double* total_dev = nullptr;
  int32_t* info_dev = nullptr;
  int rc;
  if ((rc = io.in(X, f.x_all, &a.X))) return rc;
  if ((rc = io.in(y, n_all, &a.y))) return rc;
  if ((rc = io.in(s, any ? f.s_all : 0, &a.s))) return rc;
  if ((rc = io.in(mw, extent(B, stridemw, (size_t)D), &a.mw))) return rc;
  if ((rc = io.in(Tf, extent(B, strideT, mat_extent(D, D, ldt)), &T_d))) return rc;
  if ((rc = io.out(kf_mean, n_all, &a.km))) return rc;
  if ((rc = io.out(kf_var, n_all, &a.kv))) return rc;
  if ((rc = io.out(kf_logpdf, nf_all, &a.kl))) return rc;
  if ((rc = io.out(kf_total, (size_t)B, &total_dev))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_dev))) return rc;
  if (!a.s) a.s = a.mw;  // (no observation at all: never dereferenced, but a valid pointer)
  if ((rc = ensure_stats(h))) return rc;
  a.degenerate = h->stats_dev + 4;
  a.info = info_dev;

  // offsets, the fold table, the records and the three item tables
  const int64_t* off_dev;
  const KflrItem *stat_dev, *red_dev, *pred_dev;
  {
    const size_t tbl = ragged_table_bytes(B);
    const char* dev[6];
    if ((rc = ragged_meta_upload(h, {{offsets, tbl}, {fo.data(), tbl}, {plan.regs.data(), plan.regs.size() * sizeof(KflrReg)},
                                     {plan.stat.data(), plan.stat.size() * sizeof(KflrItem)}, {plan.red.data(), plan.red.size() * sizeof(KflrItem)},
                                     {plan.pred.data(), plan.pred.size() * sizeof(KflrItem)}}, dev)))
      return rc;
    off_dev = reinterpret_cast<const int64_t*>(dev[0]);
    a.fold_offsets = reinterpret_cast<const int64_t*>(dev[1]);
    a.regs = reinterpret_cast<const KflrReg*>(dev[2]);
    stat_dev = reinterpret_cast<const KflrItem*>(dev[3]);
    red_dev = reinterpret_cast<const KflrItem*>(dev[4]);
    pred_dev = reinterpret_cast<const KflrItem*>(dev[5]);
  }
  const int64_t ychunk = heldout_ragged_status<T>(h, B, D, T_d, ldt, strideT, a.s, strides, noise_kind, off_dev, info_dev);
  HIP_TRY(h, hipGetLastError());
  const bool predict = a.km || a.kv;
  if (any && (predict || a.kl || total_dev)) {
    const int NB = (int)(D + 15) / 16, DP = 16 * NB;
    const size_t packed = (size_t)DP * (DP + 1) / 2, SZ = packed + DP;
    if ((rc = heldout_ragged_spill(h, total_dev, 0, nf_all, 0, 256, &a.kl))) return rc;
    Carve carve;
    const size_t nrf = (size_t)plan.max_folds, nsl = (size_t)plan.max_slots, nbm = (size_t)plan.max_nb;
    const size_t o_st = carve(nsl * SZ * sizeof(double)), o_U = carve(nrf * D * D * sizeof(T)), o_A = carve(nbm * packed * sizeof(double));
    const size_t o_ld = carve(nbm * sizeof(double)), o_sc = carve(nsl * 2 * sizeof(double));
    const size_t o_mw = carve(nrf * D * sizeof(T)), o_fi = carve(nrf * sizeof(int32_t));
    if ((rc = h->cov_ws.reserve(h, carve.off))) return rc;
    char* const ws = h->cov_ws.p;
    a.stats = reinterpret_cast<double*>(ws + o_st); a.U = reinterpret_cast<T*>(ws + o_U); a.A = reinterpret_cast<double*>(ws + o_A);
    a.ldA = reinterpret_cast<double*>(ws + o_ld); a.scal = reinterpret_cast<double*>(ws + o_sc); a.mwf = reinterpret_cast<T*>(ws + o_mw);
    a.finfo = reinterpret_cast<int32_t*>(ws + o_fi);
    const size_t lds_s = kfl_state_lds_bytes(sizeof(T), (int)D), lds_p = kfl_predict_lds_bytes(sizeof(T), (int)D);
    void (*const pred)(KflrArgs<T>) = layout == BLR_LAYOUT_ROWVECS ? kflr_predict_kernel<T, LAYOUT_ROWVECS> : kflr_predict_kernel<T, LAYOUT_COLVECS>;
    void (*const state)(KflArgs<T>) = kfl_state_kernel<T>;
    if ((rc = set_lds_once(h, state, lds_s))) return rc;
    if (predict && (rc = set_lds_once(h, pred, lds_p))) return rc;
    if (predict && (rc = MargImages<T>::reserve(h, std::max<int64_t>(1, plan.max_folds)))) return rc;
    // (every regressor's slice starts at a multiple of the vector when X and ldx do: ColVecs columns are ldx apart.)  Asked of the
    // STAGED pointer alone, unlike marg_ragged_gemm_takes: the answer only picks phase_gram's loader (MODE 4 or 0), which moves the
    // same values into the same LDS places -- the arithmetic and its order do not depend on it, so a host-memspace call whose staged
    // copy is aligned where the caller's array is not still gives the device-memspace call's bits (as in kfold_large_batched)
    const bool vec_ok = colv && D % Mfma<T>::VEC == 0 && aligned16(a.X, ldx, 0);
    KflArgs<T> st{};  // kfl_state_kernel reads the factors and the status and writes A, logdet A: nothing of the folds
    st.Tf = T_d; st.ldt = ldt; st.strideT = strideT; st.info = info_dev; st.A = a.A; st.ldA = a.ldA; st.D = (int)D;
    for (const KflrChunk& c : plan.chunks) {
      if (c.nfolds == 0) continue;  // (no observation in the chunk)
      KflrArgs<T> k = a;
      k.b0 = (int)c.b0; k.nb = (int)c.nb; k.fold0 = c.fold0; k.slot0 = c.slot0;
      st.reg0 = (int)c.b0;
      hipLaunchKernelGGL(state, dim3((unsigned)c.nb), dim3(kThreads), lds_s, h->stream, st);
      HIP_TRY(h, hipGetLastError());
      switch (NB) {
        case 1: rc = kfold_large_ragged_nb<T, 1>(h, k, c, stat_dev, red_dev, vec_ok); break;
        case 2: rc = kfold_large_ragged_nb<T, 2>(h, k, c, stat_dev, red_dev, vec_ok); break;
        case 3: rc = kfold_large_ragged_nb<T, 3>(h, k, c, stat_dev, red_dev, vec_ok); break;
        case 4: rc = kfold_large_ragged_nb<T, 4>(h, k, c, stat_dev, red_dev, vec_ok); break;
        case 5: rc = kfold_large_ragged_nb<T, 5>(h, k, c, stat_dev, red_dev, vec_ok); break;
        case 6: rc = kfold_large_ragged_nb<T, 6>(h, k, c, stat_dev, red_dev, vec_ok); break;
        case 7: rc = kfold_large_ragged_nb<T, 7>(h, k, c, stat_dev, red_dev, vec_ok); break;
        default: rc = kfold_large_ragged_nb<T, 8>(h, k, c, stat_dev, red_dev, vec_ok); break;
      }
      if (rc) return rc;
      if (predict) {
        k.img = MargImages<T>::launch(h, k.U, D, D * D, (int)D, (const int32_t*)k.finfo, 0, c.nfolds);
        k.items = pred_dev + c.pred0;
        hipLaunchKernelGGL(pred, dim3((unsigned)c.npred), dim3(kThreads), lds_p, h->stream, k);
        HIP_TRY(h, hipGetLastError());
      }
    }
    h->route = "kflr_factor_kernel";
    h->route_i8_B = 0;
  }
  h->last_chunks = std::max<int64_t>(1, plan.last_chunks);
  if (total_dev) heldout_ragged_totals(h, B, ychunk, a.kl, a.fold_offsets, total_dev, info_dev);
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

// ---- rank-k update / downdate of a resident MULTI-OUTPUT state: one factor, S mean columns (blr_update_multi_factor_*,
// blr_downdate_multi_factor_*; blr_state_cols.hpp) ---------------------------------------------------------------------

static_assert(kStateChunk == kSweepMaxK, "state_cols_kernel walks the observations in the sweep's chunks");

template <typename T, bool DOWN>
int state_multi_factor(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, int64_t S, const T* X, int64_t ldx,
                       int64_t strideX, const T* Y, int64_t ldY, int64_t strideY, int noise_kind, const T* s, int64_t strides, T* M,
                       int64_t ldm, int64_t strideM, T* Tf, int64_t ldt, int64_t strideT, double* logpdf, int64_t stride_lp, int32_t* info) {
  // (the argument checks come before the handle's: they need no device)
  if (h) h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (layout != BLR_LAYOUT_COLVECS && layout != BLR_LAYOUT_ROWVECS) return bad_arg(h, 3, "unknown layout (reference :26-31)");
  if (B < 0 || B > (1 << 30)) return bad_arg(h, 4, "B out of range (0..2^30)");
  if (D < 1 || D > kMaxLargeD) return bad_arg(h, 5, "D out of range (1..8192)");
  if (k < 0 || k > (1 << 30)) return bad_arg(h, 6, "k out of range (0..2^30)");
  if (S < 0 || S > (1 << 20)) return bad_arg(h, 7, "S out of range (0..2^20)");
  if (B == 0 || S == 0) return 0;
  if (k > 0 && !X) return bad_arg(h, 8, "X is NULL");
  if (layout == BLR_LAYOUT_COLVECS ? ldx < D : ldx < std::max<int64_t>(k, 1)) return bad_arg(h, 9, "ldx too small");
  if (strideX < 0) return bad_arg(h, 10, "strideX < 0");
  if (k > 0 && !Y) return bad_arg(h, 11, "Y is NULL (reference :74 length check)");
  if (ldY < k) return bad_arg(h, 12, "ldY < k (reference :74 length check)");
  if (strideY < 0) return bad_arg(h, 13, "strideY < 0");
  if (noise_kind != BLR_NOISE_ISOTROPIC && noise_kind != BLR_NOISE_DIAGONAL)
    return bad_arg(h, 14, "noise_kind (isotropic or diagonal; a resident state is not updated or downdated under dense noise)");
  if (!s) return bad_arg(h, 15, "s is NULL");
  if (strides < 0) return bad_arg(h, 16, "strides < 0");
  if (!M) return bad_arg(h, 17, "M is NULL");
  if (ldm < D) return bad_arg(h, 18, "ldm < D");
  if (B > 1 && strideM < ldm * S) return bad_arg(h, 19, "strideM < ldm * S");
  if (!Tf) return bad_arg(h, 20, "T is NULL");
  if (ldt < D) return bad_arg(h, 21, "ldt < D");
  if (B > 1 && strideT < (int64_t)mat_extent(D, D, ldt)) return bad_arg(h, 22, "strideT too small");
  if (logpdf && B > 1 && stride_lp < S) return bad_arg(h, 24, "stride_lp < S");
  if (!info) return bad_arg(h, 25, "info is NULL");
  if (!h) return -1;
  h->last_chunks = 1;  // (a route with a chunk loop counts its own)
  HIP_TRY(h, hipSetDevice(h->device));

  if (k == 0) {  // nothing to condition on or to forget: the state keeps its bits, every evidence is 0
    if (memspace == BLR_MEM_HOST) {
      for (int64_t b = 0; b < B; ++b) {
        info[b] = 0;
        for (int64_t c = 0; logpdf && c < S; ++c) logpdf[b * stride_lp + c] = 0.0;
      }
      return 0;
    }
    HIP_TRY(h, hipMemsetAsync(info, 0, (size_t)B * sizeof(int32_t), h->stream));
    if (logpdf) HIP_TRY(h, hipMemset2DAsync(logpdf, (size_t)std::max<int64_t>(stride_lp, S) * sizeof(double), 0, (size_t)S * sizeof(double), (size_t)B, h->stream));
    if (!h->async) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  auto single = [&](int ms, const T* X_, const T* y_, const T* s_, T* m_, T* T_, double* lp_, int32_t* info_) {
    if (DOWN) return downdate_factor<T>(h, ms, layout, B, D, k, X_, ldx, strideX, y_, strideY, noise_kind, s_, strides, m_, strideM, T_, ldt, strideT, lp_, info_);
    return update_factor<T>(h, ms, layout, B, D, k, X_, ldx, strideX, y_, strideY, noise_kind, s_, strides, m_, strideM, T_, ldt, strideT, lp_, info_);
  };
  // S = 1 with a dense evidence vector IS the single-column entry point
  if (S == 1 && (!logpdf || B == 1 || stride_lp == 1)) return single(memspace, X, Y, s, M, Tf, logpdf, info);

  StateColsArgs<T> a{};
  a.ldx = ldx; a.strideX = strideX; a.layout = layout; a.ldY = ldY; a.strideY = strideY; a.strides = strides; a.noise_kind = noise_kind;
  a.ldm = ldm; a.strideM = strideM; a.ldt = ldt; a.strideT = strideT; a.stride_lp = stride_lp;
  a.D = (int)D; a.k = (int)k; a.S = (int)S;
  CallIO io(h, memspace);
  const size_t x_one = layout == BLR_LAYOUT_COLVECS ? mat_extent(D, k, ldx) : mat_extent(k, D, ldx);
  const size_t s_one = noise_kind == BLR_NOISE_DIAGONAL ? (size_t)k : 1;
  T* T_d = nullptr;
  int32_t* info_d = nullptr;
  int rc;
  if ((rc = io.in(X, extent(B, strideX, x_one), &a.X))) return rc;
  if ((rc = io.in(Y, extent(B, strideY, mat_extent(k, S, ldY)), &a.Y))) return rc;
  if ((rc = io.in(s, extent(B, strides, s_one), &a.s))) return rc;
  if ((rc = io.out(M, extent(B, strideM, mat_extent(D, S, ldm)), &a.M))) return rc;
  if ((rc = io.out(Tf, extent(B, strideT, mat_extent(D, D, ldt)), &T_d))) return rc;
  if ((rc = io.out(logpdf, extent(B, stride_lp, (size_t)S), &a.logpdf))) return rc;
  if ((rc = io.out(info, (size_t)B, &info_d))) return rc;
  a.Tf = T_d; a.info = info_d;

  // Pre-pass: the old diagonal of T (the log-determinant term of the further columns' evidence) into the handle's workspace, next to
  // column 0's evidence (the caller's logpdf has a stride of its own)
  const size_t lp0_bytes = ((size_t)B * sizeof(double) + 255) & ~(size_t)255;
  const bool global = D > kMaxSmallD;
  // (fp32, D <= 128: the whole factor too -- state_cols_kernel<float> forms A m_c of the state before the call from it)
  const bool save_T = sizeof(T) == 4 && !global && S > 1;
  const size_t diag_bytes = ((size_t)B * D * sizeof(T) + 255) & ~(size_t)255;
  if ((rc = h->multi_ws.reserve(h, lp0_bytes + diag_bytes + (save_T ? (size_t)B * D * D * sizeof(T) : 0)))) return rc;
  double* const lp0 = reinterpret_cast<double*>(h->multi_ws.p);
  T* const diag0 = reinterpret_cast<T*>(h->multi_ws.p + lp0_bytes);
  a.lp0 = lp0; a.diag0 = diag0;
  a.T0 = reinterpret_cast<T*>(h->multi_ws.p + lp0_bytes + diag_bytes);
  hipLaunchKernelGGL(state_diag_kernel<T>, dim3((unsigned)((B * D + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, (const T*)T_d, ldt,
                     strideT, (int)D, B * D, diag0);
  if constexpr (sizeof(T) == 4) {
    if (save_T)
      hipLaunchKernelGGL(state_save_kernel<T>, dim3((unsigned)((B * D * D + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, (const T*)T_d,
                         ldt, strideT, (int)D, B * D * D, const_cast<T*>(a.T0));
  }
  HIP_TRY(h, hipGetLastError());
  {
    // Step 1: column 0 and the factor through the single-column entry point, unchanged (device operands; at D <= 128 it only enqueues,
    // at larger D it may synchronise)
    const AsyncScope nested(h, global ? h->async : true);
    if ((rc = single(BLR_MEM_DEVICE, a.X, a.Y, a.s, a.M, T_d, lp0, info_d))) return rc;  // (checked operands: a HIP failure)
  }
  // Step 2: the columns 1 .. S-1 of every regressor (and the copy of column 0's evidence to its place)
  void (*const kern)(StateColsArgs<T>) = global ? state_cols_global_kernel<T, DOWN> : state_cols_kernel<T, DOWN>;
  if (!global) {
    const int64_t passes = std::max<int64_t>(1, (S - 1 + kStateColsPerPass - 1) / kStateColsPerPass);
    const size_t lds = state_cols_lds_bytes(sizeof(T), (int)D);
    if ((rc = set_lds_once(h, kern, lds))) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)B, (unsigned)passes), dim3(kThreads), lds, h->stream, a);
  } else {
    // correct, not fast: one workgroup per (column, regressor) reading T' from global memory; column 0's evidence is copied by the host
    const size_t lds = state_cols_global_lds_bytes((int)D);
    if ((rc = set_lds_once(h, kern, lds))) return rc;
    if (a.logpdf) HIP_TRY(h, hipMemcpy2DAsync(a.logpdf, (size_t)stride_lp * sizeof(double), lp0, sizeof(double), sizeof(double), (size_t)B, hipMemcpyDeviceToDevice, h->stream));
    const int64_t chunk = h->cap_chunk(32768);
    if (S > 1) h->count_chunks(B, chunk);
    for (int64_t b0 = 0; S > 1 && b0 < B; b0 += chunk) {
      StateColsArgs<T> g = a;
      g.X += b0 * strideX; g.Y += b0 * strideY; g.s += b0 * strides; g.M += b0 * strideM; g.Tf += b0 * strideT;
      g.diag0 += b0 * D; g.info += b0;
      if (g.logpdf) g.logpdf += b0 * stride_lp;
      hipLaunchKernelGGL(kern, dim3((unsigned)(S - 1), (unsigned)std::min<int64_t>(chunk, B - b0)), dim3(kThreads), lds, h->stream, g);
    }
  }
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

}  // namespace

// =======================================================================================================
extern "C" {

int blr_abi_version(void) { return BLR_ABI_VERSION; }

int blr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int blr_create(int device, blr_handle** out) {
  if (!out) return -2;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return -(1000 + (int)(e == hipSuccess ? hipErrorNoDevice : e));
  if (device < 0 || device >= n) return -1;
  blr_handle* h = new (std::nothrow) blr_handle();
  if (!h) return -(1000 + (int)hipErrorOutOfMemory);
  h->device = device;
  if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&h->ev0)) != hipSuccess || (e = hipEventCreate(&h->ev1)) != hipSuccess) {
    delete h;
    return -(1000 + (int)e);
  }
  h->stream = h->own_stream;
  h->opt.from_environment();  // the only getenv calls of the library
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->cus = cus;
  *out = h;
  return 0;
}

int blr_destroy(blr_handle* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  if (h->comm && rccl().ok) (void)rccl().CommDestroy(h->comm);
  for (DevBuf* b : h->releasable()) (void)hipFree(b->p);
  (void)hipFree(h->xchg.p);
  if (h->stats_dev) (void)hipFree(h->stats_dev);
  if (h->ticket) (void)hipFree(h->ticket);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return 0;
}

const char* blr_last_error(blr_handle* h) { return h ? h->err.c_str() : "null handle"; }

int blr_release_workspace(blr_handle* h) {
  if (!h) return -1;
  h->err.clear();
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (DevBuf* b : h->releasable()) {
    const int rc = b->release(h);
    if (rc) return rc;
  }
  return 0;
}

int blr_set_option(blr_handle* h, const char* key, const char* value) {
  if (!h) return -1;
  h->err.clear();
  const int orc = h->opt.set(key, value);
  if (orc == -2) return bad_arg(h, 2, "unknown option key");
  if (orc != 0) return bad_arg(h, 3, "malformed option value");
  h->gram_plans.clear();  // (cached launch plans were made under the old switches)
  return 0;
}

// Work of one handle is ordered by ITS stream: the arrival counters of panel_chain_kernel, the tagged exchange buffer and the
// grow-only scratch assume that a launch's predecessor on the handle has finished with them.  Switching streams therefore
// drains the old one first and re-arms both banks of arrival counters (a launch clears the bank of its successor, which on a
// second stream could already be counting in it).
static int switch_stream(blr_handle* h, hipStream_t next) {
  if (next == h->stream) return 0;
  h->err.clear();
  HIP_TRY(h, hipSetDevice(h->device));
  // The old stream must still be alive here (header).  If the caller has destroyed it all the same, the drain fails -- and must not
  // leave the handle bound to a dead stream for good: clear the error, drain the device instead, and switch anyway.
  if (hipStreamSynchronize(h->stream) != hipSuccess) {
    (void)hipGetLastError();
    HIP_TRY(h, hipDeviceSynchronize());
  }
  h->stream = next;
  if (h->ticket) HIP_TRY(h, hipMemsetAsync(h->ticket + 16, 0, 2 * kPanelArriveWords * sizeof(unsigned), h->stream));
  h->panel_launches = 0;
  return 0;
}
int blr_set_stream(blr_handle* h, void* hip_stream) {
  if (!h) return -1;
  return switch_stream(h, static_cast<hipStream_t>(hip_stream));
}
int blr_reset_stream(blr_handle* h) {
  if (!h) return -1;
  return switch_stream(h, h->own_stream);
}
const char* blr_last_route(blr_handle* h) {
  if (!h) return "null handle";
  // The int8 route decides ON THE DEVICE what it keeps: a probe slice that hands back more than a quarter of its regressors (heavy
  // tails) sends the rest of the batch to the fp64 kernel, and then that kernel is what a profile of the call shows.  Look at the
  // call's hand-back count (this drains the handle's stream) and name the kernel that did most of the work.
  if (h->route_i8_B > 0 && h->stats_dev != nullptr) {
    unsigned long long v[3] = {0, 0, 0};
    if (hipSetDevice(h->device) == hipSuccess &&
        hipMemcpyAsync(v, h->stats_dev, sizeof(v), hipMemcpyDeviceToHost, h->stream) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess) {
      const unsigned long long handed = v[0] - v[2];
      if (2 * handed > (unsigned long long)h->route_i8_B) {
        h->route_buf = "fused_small_kernel<double, 8, 4> (int8 route handed back " + std::to_string(handed) + " of " + std::to_string(h->route_i8_B) + ")";
        return h->route_buf.c_str();
      }
    } else {
      (void)hipGetLastError();
    }
  }
  return h->route;
}

int blr_get_stat(blr_handle* h, const char* key, int64_t* value) {
  if (!h) return -1;
  h->err.clear();
  if (!key) return bad_arg(h, 2, "key is NULL");
  if (!value) return bad_arg(h, 3, "value is NULL");
  if (!strcmp(key, "i8_regressors")) { *value = (int64_t)h->i8_attempted; return 0; }
  if (!strcmp(key, "last_chunks")) { *value = h->last_chunks; return 0; }  // chunks / slices of regressors of the most recent call
  // the kernels of the most recent blr_sample_weights_* / blr_apply_weights_* / blr_rand_* / blr_rand_batched_* call: a bitmask
  // (weights: 1 diag, 2 mfma, 2 + 4 mfma with the 16-byte loader of U, 8 large, 16 batched NS = 1, 32 batched NS = 4;
  // projection: 64 fused, 128 scalar, 256 mfma, none of them = no projection; blr_host.hpp DrawRoute)
  if (!strcmp(key, "draw_route")) { *value = h->draw_route; return 0; }
  // the plan of the most recent blr_update_factor_ragged_* / blr_downdate_factor_ragged_* call: regressors per list
  if (!strcmp(key, "ragged_sweep")) { *value = h->ragged_lists[0]; return 0; }
  if (!strcmp(key, "ragged_refit")) { *value = h->ragged_lists[1]; return 0; }
  if (!strcmp(key, "ragged_idle")) { *value = h->ragged_lists[2]; return 0; }
  // the variance route of the most recent blr_marginals_batched_* call (host-side, set next to marg_blocksub_kernel's launches)
  if (!strcmp(key, "marg_block_rt")) { *value = h->marg_block.rt; return 0; }
  if (!strcmp(key, "marg_block_walk")) { *value = h->marg_block.walk; return 0; }
  if (!strcmp(key, "marg_block_renumbered")) { *value = h->marg_block.renumbered; return 0; }
  if (!strcmp(key, "i8_handed_back")) {
    unsigned long long v = 0;
    if (h->stats_dev) {
      HIP_TRY(h, hipSetDevice(h->device));
      HIP_TRY(h, hipMemcpyAsync(&v, h->stats_dev, sizeof(v), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    *value = (int64_t)v;
    return 0;
  }
  if (!strcmp(key, "planes_redone")) {  // large-D fp32 updates whose sampled row scales did not hold: exact row maxima + planes made again
    unsigned long long v = 0;
    if (h->stats_dev) {
      HIP_TRY(h, hipSetDevice(h->device));
      HIP_TRY(h, hipMemcpyAsync(&v, h->stats_dev + 1, sizeof(v), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    *value = (int64_t)v;
    return 0;
  }
  if (!strcmp(key, "loo_degenerate")) {  // observations blr_loo_batched_* gave NaN: 1 - h_n <= 0 or not finite (cumulative)
    unsigned long long v = 0;
    if (h->stats_dev) {
      HIP_TRY(h, hipSetDevice(h->device));
      HIP_TRY(h, hipMemcpyAsync(&v, h->stats_dev + 3, sizeof(v), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    *value = (int64_t)v;
    return 0;
  }
  if (!strcmp(key, "kfold_degenerate")) {  // folds blr_kfold_batched_* / blr_kfold_multi_batched_* / blr_kfold_large_batched_* gave NaN: a pivot <= 0 or not finite (cumulative)
    unsigned long long v = 0;
    if (h->stats_dev) {
      HIP_TRY(h, hipSetDevice(h->device));
      HIP_TRY(h, hipMemcpyAsync(&v, h->stats_dev + 4, sizeof(v), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    *value = (int64_t)v;
    return 0;
  }
  if (!strcmp(key, "workspace_bytes")) {
    *value = (int64_t)(h->ws.bytes + h->feat.bytes + h->aux.bytes + h->i8side.bytes + h->xchg.bytes + h->loo_ws.bytes + h->ragged_meta.bytes + h->multi_ws.bytes + h->cov_ws.bytes);
    return 0;
  }
  return bad_arg(h, 2, "unknown statistic");
}
int blr_reset_stats(blr_handle* h) {
  if (!h) return -1;
  h->err.clear();
  if (h->stats_dev) {  // (device counter first: a failure must not leave the two counters apart)
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemsetAsync(h->stats_dev, 0, 5 * sizeof(unsigned long long), h->stream));  // (total, planes made twice, the last call's base, LOO degenerate, K-fold degenerate)
  }
  h->i8_attempted = 0;
  return 0;
}
int blr_set_async(blr_handle* h, int async) {
  if (!h) return -1;
  h->async = async != 0;
  return 0;
}
int blr_synchronize(blr_handle* h) {
  if (!h) return -1;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

int blr_device_alloc(blr_handle* h, size_t bytes, void** dptr) {
  if (!h) return -1;
  if (!dptr) return -3;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMalloc(dptr, bytes ? bytes : 1));
  return 0;
}
int blr_device_free(blr_handle* h, void* dptr) {
  if (!h) return -1;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipFree(dptr));
  return 0;
}
int blr_memcpy_h2d(blr_handle* h, void* dst, const void* src, size_t bytes) {
  if (!h) return -1;
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}
int blr_memcpy_d2h(blr_handle* h, void* dst, const void* src, size_t bytes) {
  if (!h) return -1;
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

int blr_timer_start(blr_handle* h) {
  if (!h) return -1;
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  return 0;
}
int blr_timer_stop(blr_handle* h, float* elapsed_ms) {
  if (!h) return -1;
  if (!elapsed_ms) return -2;
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  HIP_TRY(h, hipEventSynchronize(h->ev1));
  HIP_TRY(h, hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
  return 0;
}

#define BLR_DEFINE(SUF, T)                                                                                          \
  int blr_posterior_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,        \
                                  const T* X, int64_t ldx, int64_t strideX, const T* y, int64_t stridey,            \
                                  int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw,         \
                                  int64_t stridemw, const T* Lw, int64_t ldl, int64_t strideLw, T* mw_post,         \
                                  int64_t stride_mwpost, T* T_post, int64_t ldt, int64_t strideT, T* Lw_post,      \
                                  int64_t ldlp, int64_t strideLp, double* logpdf, int32_t* info) {                  \
    return posterior_batched<T>(h, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides,  \
                                prior_kind, mw, stridemw, Lw, ldl, strideLw, mw_post, stride_mwpost, T_post, ldt,    \
                                strideT, Lw_post, ldlp, strideLp, logpdf, info);                                    \
  }                                                                                                                 \
  int blr_update_factor_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, const T* X, \
                              int64_t ldx, int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s, \
                              int64_t strides, T* mw, int64_t stridemw, T* Tf, int64_t ldt, int64_t strideT,         \
                              double* logpdf, int32_t* info) {                                                       \
    return update_factor<T>(h, memspace, layout, B, D, k, X, ldx, strideX, y, stridey, noise_kind, s, strides, mw,   \
                            stridemw, Tf, ldt, strideT, logpdf, info);                                               \
  }                                                                                                                 \
  int blr_downdate_factor_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k,           \
                                const T* X, int64_t ldx, int64_t strideX, const T* y, int64_t stridey,              \
                                int noise_kind, const T* s, int64_t strides, T* mw, int64_t stridemw, T* Tf,        \
                                int64_t ldt, int64_t strideT, double* logpdf, int32_t* info) {                      \
    return downdate_factor<T>(h, memspace, layout, B, D, k, X, ldx, strideX, y, stridey, noise_kind, s, strides,    \
                              mw, stridemw, Tf, ldt, strideT, logpdf, info);                                         \
  }                                                                                                                 \
  int blr_update_factor_ragged_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,                 \
                                     const int64_t* offsets, const T* X, int64_t ldx, const T* y, int noise_kind,   \
                                     const T* s, int64_t strides, T* mw, int64_t stridemw, T* Tf, int64_t ldt,      \
                                     int64_t strideT, double* logpdf, int32_t* info) {                              \
    return revise_ragged<T, false>(h, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw,       \
                                   stridemw, Tf, ldt, strideT, logpdf, info);                                       \
  }                                                                                                                 \
  int blr_downdate_factor_ragged_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,               \
                                       const int64_t* offsets, const T* X, int64_t ldx, const T* y, int noise_kind, \
                                       const T* s, int64_t strides, T* mw, int64_t stridemw, T* Tf, int64_t ldt,    \
                                       int64_t strideT, double* logpdf, int32_t* info) {                            \
    return revise_ragged<T, true>(h, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw,        \
                                  stridemw, Tf, ldt, strideT, logpdf, info);                                        \
  }                                                                                                                 \
  int blr_loo_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X,  \
                            int64_t ldx, int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s, \
                            int64_t strides, const T* mw, int64_t stridemw, const T* Tf, int64_t ldt,               \
                            int64_t strideT, T* loo_mean, int64_t stride_lm, T* loo_var, int64_t stride_lv,         \
                            double* loo_logpdf, int64_t stride_ll, double* loo_total, int32_t* info) {              \
    return loo_batched<T>(h, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides, mw,     \
                          stridemw, Tf, ldt, strideT, loo_mean, stride_lm, loo_var, stride_lv, loo_logpdf,          \
                          stride_ll, loo_total, info);                                                             \
  }                                                                                                                 \
  int blr_kfold_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t F, \
                              const T* X, int64_t ldx, int64_t strideX, const T* y, int64_t stridey, int noise_kind, \
                              const T* s, int64_t strides, const T* mw, int64_t stridemw, const T* Tf, int64_t ldt,  \
                              int64_t strideT, T* kf_mean, int64_t stride_km, T* kf_var, int64_t stride_kv,         \
                              double* kf_logpdf, int64_t stride_kl, double* kf_total, int32_t* info) {              \
    return kfold_batched<T>(h, memspace, layout, B, D, N, F, X, ldx, strideX, y, stridey, noise_kind, s, strides,    \
                            mw, stridemw, Tf, ldt, strideT, kf_mean, stride_km, kf_var, stride_kv, kf_logpdf,       \
                            stride_kl, kf_total, info);                                                            \
  }                                                                                                                 \
  int blr_kfold_large_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,     \
                                    int64_t F, const T* X, int64_t ldx, int64_t strideX, const T* y, int64_t stridey, \
                                    int noise_kind, const T* s, int64_t strides, const T* mw, int64_t stridemw,     \
                                    const T* Tf, int64_t ldt, int64_t strideT, T* kf_mean, int64_t stride_km,       \
                                    T* kf_var, int64_t stride_kv, double* kf_logpdf, int64_t stride_kl,             \
                                    double* kf_total, int32_t* info) {                                              \
    return kfold_large_batched<T>(h, memspace, layout, B, D, N, F, X, ldx, strideX, y, stridey, noise_kind, s,      \
                                  strides, mw, stridemw, Tf, ldt, strideT, kf_mean, stride_km, kf_var, stride_kv,   \
                                  kf_logpdf, stride_kl, kf_total, info);                                            \
  }                                                                                                                 \
  int blr_logpdf_grid_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const T* X,  \
                            int64_t ldx, int64_t strideX, const T* y, int64_t stridey, int noise_kind, const T* s, \
                            int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw,            \
                            int64_t ldl, int64_t strideLw, int64_t G, const T* alpha, int64_t stride_alpha,         \
                            const T* tau, int64_t stride_tau, double* logpdf, int64_t stride_lp, int64_t* best,     \
                            T* mw_best, int64_t stride_mwbest, T* T_best, int64_t ldt, int64_t strideT,             \
                            int32_t* info, int64_t stride_info) {                                                   \
    return logpdf_grid<T>(h, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides,        \
                          prior_kind, mw, stridemw, Lw, ldl, strideLw, G, alpha, stride_alpha, tau, stride_tau,     \
                          logpdf, stride_lp, best, mw_best, stride_mwbest, T_best, ldt, strideT, info, stride_info);\
  }                                                                                                                 \
  int blr_logpdf_grid_ragged_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,                   \
                                   const int64_t* offsets, const T* X, int64_t ldx, const T* y, int noise_kind,     \
                                   const T* s, int64_t strides, int prior_kind, const T* mw, int64_t stridemw,      \
                                   const T* Lw, int64_t ldl, int64_t strideLw, int64_t G, const T* alpha,           \
                                   int64_t stride_alpha, const T* tau, int64_t stride_tau, double* logpdf,          \
                                   int64_t stride_lp, int64_t* best, T* mw_best, int64_t stride_mwbest, T* T_best,  \
                                   int64_t ldt, int64_t strideT, int32_t* info, int64_t stride_info) {              \
    return logpdf_grid_ragged<T>(h, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, prior_kind, \
                                 mw, stridemw, Lw, ldl, strideLw, G, alpha, stride_alpha, tau, stride_tau, logpdf,  \
                                 stride_lp, best, mw_best, stride_mwbest, T_best, ldt, strideT, info, stride_info); \
  }                                                                                                                 \
  int blr_posterior_ragged_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,                     \
                                 const int64_t* offsets, const T* X, int64_t ldx, const T* y, int noise_kind,       \
                                 const T* s, int64_t strides, int prior_kind, const T* mw, int64_t stridemw,        \
                                 const T* Lw, int64_t ldl, int64_t strideLw, T* mw_post, int64_t stride_mwpost,     \
                                 T* T_post, int64_t ldt, int64_t strideT, T* Lw_post, int64_t ldlp,                 \
                                 int64_t strideLp, double* logpdf, int32_t* info) {                                 \
    return posterior_ragged<T>(h, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, prior_kind,   \
                               mw, stridemw, Lw, ldl, strideLw, mw_post, stride_mwpost, T_post, ldt, strideT,       \
                               Lw_post, ldlp, strideLp, logpdf, info);                                              \
  }                                                                                                                 \
  int blr_marginals_ragged_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,                     \
                                 const int64_t* offsets, const T* X, int64_t ldx, int noise_kind, const T* s,       \
                                 int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw,       \
                                 int64_t ldl, int64_t strideLw, T* mean, T* var, int32_t* info) {                   \
    return marginals_ragged<T>(h, memspace, layout, B, D, offsets, X, ldx, noise_kind, s, strides, prior_kind, mw,  \
                               stridemw, Lw, ldl, strideLw, mean, var, info);                                       \
  }                                                                                                                 \
  int blr_loo_ragged_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets,   \
                           const T* X, int64_t ldx, const T* y, int noise_kind, const T* s, int64_t strides,        \
                           const T* mw, int64_t stridemw, const T* Tf, int64_t ldt, int64_t strideT, T* loo_mean,   \
                           T* loo_var, double* loo_logpdf, double* loo_total, int32_t* info) {                      \
    return loo_ragged<T>(h, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw, stridemw, Tf,   \
                         ldt, strideT, loo_mean, loo_var, loo_logpdf, loo_total, info);                             \
  }                                                                                                                 \
  int blr_kfold_ragged_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets, \
                             int64_t F, const T* X, int64_t ldx, const T* y, int noise_kind, const T* s,            \
                             int64_t strides, const T* mw, int64_t stridemw, const T* Tf, int64_t ldt,              \
                             int64_t strideT, T* kf_mean, T* kf_var, double* kf_logpdf, double* kf_total,           \
                             int32_t* info) {                                                                       \
    return kfold_ragged<T>(h, memspace, layout, B, D, offsets, F, X, ldx, y, noise_kind, s, strides, mw, stridemw,  \
                           Tf, ldt, strideT, kf_mean, kf_var, kf_logpdf, kf_total, info);                           \
  }                                                                                                                 \
  int blr_kfold_large_ragged_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,                   \
                                   const int64_t* offsets, const int64_t* fold_sizes, const T* X, int64_t ldx,      \
                                   const T* y, int noise_kind, const T* s, int64_t strides, const T* mw,            \
                                   int64_t stridemw, const T* Tf, int64_t ldt, int64_t strideT, T* kf_mean,         \
                                   T* kf_var, double* kf_logpdf, double* kf_total, int32_t* info) {                 \
    return kfold_large_ragged<T>(h, memspace, layout, B, D, offsets, fold_sizes, X, ldx, y, noise_kind, s, strides, \
                                 mw, stridemw, Tf, ldt, strideT, kf_mean, kf_var, kf_logpdf, kf_total, info);       \
  }                                                                                                                 \
  int blr_posterior_multi_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,   \
                                        int64_t S, const T* X, int64_t ldx, int64_t strideX, const T* Y,            \
                                        int64_t ldY, int64_t strideY, int noise_kind, const T* s, int64_t strides,  \
                                        int prior_kind, const T* mw, int64_t stridemw, const T* Lw, int64_t ldl,    \
                                        int64_t strideLw, T* mw_post, int64_t ldmp, int64_t stride_mwpost,          \
                                        T* T_post, int64_t ldt, int64_t strideT, T* Lw_post, int64_t ldlp,          \
                                        int64_t strideLp, double* logpdf, int64_t stride_lp, int32_t* info) {       \
    return posterior_multi_batched<T>(h, memspace, layout, B, D, N, S, X, ldx, strideX, Y, ldY, strideY, noise_kind, \
                                      s, strides, prior_kind, mw, stridemw, Lw, ldl, strideLw, mw_post, ldmp,        \
                                      stride_mwpost, T_post, ldt, strideT, Lw_post, ldlp, strideLp, logpdf,         \
                                      stride_lp, info);                                                             \
  }                                                                                                                 \
  int blr_marginals_multi_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,   \
                                        int64_t S, const T* X, int64_t ldx, int64_t strideX, int noise_kind,        \
                                        const T* s, int64_t strides, int prior_kind, const T* M, int64_t ldm,       \
                                        int64_t strideM, const T* Lw, int64_t ldl, int64_t strideLw, T* mean,       \
                                        int64_t ldmean, int64_t stridemean, T* var, int64_t stridevar,              \
                                        int32_t* info) {                                                            \
    return marginals_multi_batched<T>(h, memspace, layout, B, D, N, S, X, ldx, strideX, noise_kind, s, strides,     \
                                      prior_kind, M, ldm, strideM, Lw, ldl, strideLw, mean, ldmean, stridemean,     \
                                      var, stridevar, info);                                                        \
  }                                                                                                                 \
  int blr_mean_and_cov_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,      \
                                     const T* X, int64_t ldx, int64_t strideX, int noise_kind, const T* s,          \
                                     int64_t lds, int64_t strides, int prior_kind, const T* mw, int64_t stridemw,  \
                                     const T* Lw, int64_t ldl, int64_t strideLw, T* mean, int64_t stridemean,       \
                                     T* C, int64_t ldc, int64_t strideC, int32_t* info) {                           \
    return mean_and_cov_batched<T>(h, memspace, layout, B, D, N, X, ldx, strideX, noise_kind, s, lds, strides,      \
                                   prior_kind, mw, stridemw, Lw, ldl, strideLw, mean, stridemean, C, ldc, strideC,  \
                                   info);                                                                           \
  }                                                                                                                 \
  int blr_loo_multi_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,         \
                                  int64_t S, const T* X, int64_t ldx, int64_t strideX, const T* Y, int64_t ldY,     \
                                  int64_t strideY, int noise_kind, const T* s, int64_t strides, const T* M,         \
                                  int64_t ldm, int64_t strideM, const T* Tf, int64_t ldt, int64_t strideT,          \
                                  T* loo_mean, int64_t ld_lm, int64_t stride_lm, T* loo_var, int64_t stride_lv,     \
                                  double* loo_logpdf, int64_t ld_ll, int64_t stride_ll, double* loo_total,          \
                                  int64_t stride_lt, int32_t* info) {                                               \
    return loo_multi_batched<T>(h, memspace, layout, B, D, N, S, X, ldx, strideX, Y, ldY, strideY, noise_kind, s,   \
                                strides, M, ldm, strideM, Tf, ldt, strideT, loo_mean, ld_lm, stride_lm, loo_var,    \
                                stride_lv, loo_logpdf, ld_ll, stride_ll, loo_total, stride_lt, info);               \
  }                                                                                                                 \
  int blr_kfold_multi_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,       \
                                    int64_t S, int64_t F, const T* X, int64_t ldx, int64_t strideX, const T* Y,     \
                                    int64_t ldY, int64_t strideY, int noise_kind, const T* s, int64_t strides,      \
                                    const T* M, int64_t ldm, int64_t strideM, const T* Tf, int64_t ldt,             \
                                    int64_t strideT, T* kf_mean, int64_t ld_km, int64_t stride_km, T* kf_var,       \
                                    int64_t stride_kv, double* kf_logpdf, int64_t ld_kl, int64_t stride_kl,         \
                                    double* kf_total, int64_t stride_kt, int32_t* info) {                           \
    return kfold_multi_batched<T>(h, memspace, layout, B, D, N, S, F, X, ldx, strideX, Y, ldY, strideY, noise_kind, \
                                  s, strides, M, ldm, strideM, Tf, ldt, strideT, kf_mean, ld_km, stride_km, kf_var, \
                                  stride_kv, kf_logpdf, ld_kl, stride_kl, kf_total, stride_kt, info);               \
  }                                                                                                                 \
  int blr_update_multi_factor_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k,       \
                                    int64_t S, const T* X, int64_t ldx, int64_t strideX, const T* Y, int64_t ldY,   \
                                    int64_t strideY, int noise_kind, const T* s, int64_t strides, T* M,             \
                                    int64_t ldm, int64_t strideM, T* Tf, int64_t ldt, int64_t strideT,              \
                                    double* logpdf, int64_t stride_lp, int32_t* info) {                             \
    return state_multi_factor<T, false>(h, memspace, layout, B, D, k, S, X, ldx, strideX, Y, ldY, strideY,          \
                                        noise_kind, s, strides, M, ldm, strideM, Tf, ldt, strideT, logpdf,          \
                                        stride_lp, info);                                                           \
  }                                                                                                                 \
  int blr_downdate_multi_factor_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k,     \
                                      int64_t S, const T* X, int64_t ldx, int64_t strideX, const T* Y, int64_t ldY, \
                                      int64_t strideY, int noise_kind, const T* s, int64_t strides, T* M,           \
                                      int64_t ldm, int64_t strideM, T* Tf, int64_t ldt, int64_t strideT,            \
                                      double* logpdf, int64_t stride_lp, int32_t* info) {                           \
    return state_multi_factor<T, true>(h, memspace, layout, B, D, k, S, X, ldx, strideX, Y, ldY, strideY,           \
                                       noise_kind, s, strides, M, ldm, strideM, Tf, ldt, strideT, logpdf,           \
                                       stride_lp, info);                                                            \
  }                                                                                                                 \
  int blr_posterior_##SUF(blr_handle* h, int layout, int64_t D, int64_t N, const T* X, int64_t ldx, const T* y,     \
                          int noise_kind, const T* s, int prior_kind, const T* mw, const T* Lw, int64_t ldl,        \
                          T* mw_post, T* T_post, int64_t ldt, T* Lw_post, int64_t ldlp, double* logpdf) {           \
    return posterior_single<T>(h, layout, D, N, X, ldx, y, noise_kind, s, prior_kind, mw, Lw, ldl, mw_post, T_post, \
                               ldt, Lw_post, ldlp, logpdf);                                                         \
  }                                                                                                                 \
  int blr_marginals_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,        \
                                  const T* X, int64_t ldx, int64_t strideX, int noise_kind, const T* s,             \
                                  int64_t strides, int prior_kind, const T* mw, int64_t stridemw, const T* Lw,      \
                                  int64_t ldl, int64_t strideLw, T* mean, int64_t stridemean, T* var,               \
                                  int64_t stridevar, int32_t* info) {                                               \
    return marginals_batched<T>(h, memspace, layout, B, D, N, X, ldx, strideX, noise_kind, s, strides, prior_kind,  \
                                mw, stridemw, Lw, ldl, strideLw, mean, stridemean, var, stridevar, info);           \
  }                                                                                                                 \
  int blr_rand_##SUF(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const T* X,          \
                     int64_t ldx, int noise_kind, const T* s, int prior_kind, const T* mw, const T* Lw,             \
                     int64_t ldl, const T* Z1, int64_t ldz1, const T* Z2, int64_t ldz2, T* Y, int64_t ldy) {        \
    return rand_impl<T>(h, memspace, layout, D, N, S, X, ldx, noise_kind, s, prior_kind, mw, Lw, ldl, Z1, ldz1, Z2, \
                        ldz2, Y, ldy);                                                                              \
  }                                                                                                                 \
  int blr_sample_weights_##SUF(blr_handle* h, int memspace, int64_t D, int64_t S, int prior_kind, const T* mw,      \
                               const T* Lw, int64_t ldl, const T* Z, int64_t ldz, T* W, int64_t ldw) {              \
    return sample_weights<T>(h, memspace, D, S, prior_kind, mw, Lw, ldl, Z, ldz, W, ldw);                           \
  }                                                                                                                 \
  int blr_rand_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,   \
                             const T* X, int64_t ldx, int64_t strideX, int noise_kind, const T* s, int64_t strides, \
                             int prior_kind, const T* mw, int64_t stridemw, const T* Lw, int64_t ldl,              \
                             int64_t strideLw, const T* Z1, int64_t ldz1, int64_t strideZ1, const T* Z2,           \
                             int64_t ldz2, int64_t strideZ2, T* W, int64_t ldw, int64_t strideW, T* Y,             \
                             int64_t ldy, int64_t strideY, int32_t* info) {                                        \
    return rand_batched<T>(h, memspace, layout, B, D, N, S, X, ldx, strideX, noise_kind, s, strides, prior_kind, mw, \
                           stridemw, Lw, ldl, strideLw, Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y,  \
                           ldy, strideY, info);                                                                     \
  }                                                                                                                 \
  int blr_rand_multi_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,        \
                                   int64_t S, int64_t R, const T* X, int64_t ldx, int64_t strideX, int noise_kind,  \
                                   const T* s, int64_t strides, int prior_kind, const T* M, int64_t ldm,            \
                                   int64_t strideM, const T* Lw, int64_t ldl, int64_t strideLw, const T* Z1,        \
                                   int64_t ldz1, int64_t strideZ1, const T* Z2, int64_t ldz2, int64_t strideZ2,     \
                                   T* W, int64_t ldw, int64_t strideW, T* Y, int64_t ldy, int64_t strideY,          \
                                   int32_t* info) {                                                                 \
    return rand_multi_batched<T>(h, memspace, layout, B, D, N, S, R, X, ldx, strideX, noise_kind, s, strides,       \
                                 prior_kind, M, ldm, strideM, Lw, ldl, strideLw, Z1, ldz1, strideZ1, Z2, ldz2,      \
                                 strideZ2, W, ldw, strideW, Y, ldy, strideY, info);                                 \
  }                                                                                                                 \
  int blr_rff_features_##SUF(blr_handle* h, int memspace, int64_t Din, int64_t D, int64_t N, const T* Xin,          \
                             int64_t ldxin, const T* Omega, int64_t ldo, const T* phase, T scale, T* Phi,           \
                             int64_t ldphi) {                                                                       \
    return rff_features<T>(h, memspace, Din, D, N, Xin, ldxin, Omega, ldo, phase, scale, Phi, ldphi);               \
  }                                                                                                                 \
  int blr_logpdf_grad_batched_##SUF(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,      \
                                    const T* X, int64_t ldx, int64_t strideX, const T* y, int64_t stridey,          \
                                    int noise_kind, const T* s, int64_t strides, int prior_kind, const T* mw,       \
                                    int64_t stridemw, const T* Lw, int64_t ldl, int64_t strideLw, double* logpdf,   \
                                    T* dX, int64_t lddx, int64_t stridedX, T* dy, int64_t stridedy, T* ds,          \
                                    int64_t strideds, T* dmw, int64_t stridedmw, T* mw_post, int64_t stride_mwpost, \
                                    T* Ainv, int64_t ldai, int64_t strideAi, int32_t* info) {                       \
    return logpdf_grad_batched<T>(h, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides, \
                                  prior_kind, mw, stridemw, Lw, ldl, strideLw, logpdf, dX, lddx, stridedX, dy,       \
                                  stridedy, ds, strideds, dmw, stridedmw, mw_post, stride_mwpost, Ainv, ldai,        \
                                  strideAi, info);                                                                  \
  }                                                                                                                 \
  int blr_logpdf_multi_##SUF(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const T* X,  \
                             int64_t ldx, const T* Y, int64_t ldY, int noise_kind, const T* s, int prior_kind,      \
                             const T* mw, const T* Lw, int64_t ldl, double* logpdf, T* mw_post, int64_t ldmp,       \
                             int32_t* info) {                                                                       \
    return logpdf_multi<T>(h, memspace, layout, D, N, S, X, ldx, Y, ldY, noise_kind, s, prior_kind, mw, Lw, ldl,     \
                           logpdf, mw_post, ldmp, info);                                                            \
  }                                                                                                                 \
  int blr_gram_stats_##SUF(blr_handle* h, int layout, int64_t D, int64_t N, const T* X, int64_t ldx, const T* y,    \
                           int noise_kind, const T* s, const T* mw, T* stats, int64_t lds, double* scal) {          \
    return gram_stats<T>(h, layout, D, N, X, ldx, y, noise_kind, s, mw, stats, lds, scal);                          \
  }                                                                                                                 \
  int blr_posterior_from_stats_##SUF(blr_handle* h, int64_t D, int64_t N_total, T* stats, int64_t lds,              \
                                     const double* scal, int prior_kind, const T* mw, const T* Lw, int64_t ldl,     \
                                     T* mw_post, T* T_post, int64_t ldt, T* Lw_post, int64_t ldlp, double* logpdf,  \
                                     int32_t* info) {                                                               \
    return posterior_from_stats<T>(h, D, N_total, stats, lds, scal, prior_kind, mw, Lw, ldl, mw_post, T_post, ldt,   \
                                   Lw_post, ldlp, logpdf, info);                                                    \
  }                                                                                                                 \
  int blr_posterior_rff_##SUF(blr_handle* h, int memspace, int64_t Din, int64_t D, int64_t N, const T* Xin,         \
                              int64_t ldxin, const T* Omega, int64_t ldo, const T* phase, T scale, const T* y,      \
                              int noise_kind, const T* s, int prior_kind, const T* mw, const T* Lw, int64_t ldl,    \
                              T* mw_post, T* T_post, int64_t ldt, T* Lw_post, int64_t ldlp, double* logpdf,         \
                              int32_t* info) {                                                                      \
    return posterior_rff<T>(h, memspace, Din, D, N, Xin, ldxin, Omega, ldo, phase, scale, y, noise_kind, s,         \
                            prior_kind, mw, Lw, ldl, mw_post, T_post, ldt, Lw_post, ldlp, logpdf, info);            \
  }                                                                                                                 \
  int blr_posterior_dense_noise_##SUF(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, const T* X,    \
                                      int64_t ldx, const T* y, const T* Sy, int64_t ldsy, int prior_kind,           \
                                      const T* mw, const T* Lw, int64_t ldl, T* mw_post, T* T_post, int64_t ldt,    \
                                      T* Lw_post, int64_t ldlp, double* logpdf, int32_t* info) {                    \
    return posterior_dense_noise<T>(h, memspace, layout, D, N, X, ldx, y, Sy, ldsy, prior_kind, mw, Lw, ldl,        \
                                    mw_post, T_post, ldt, Lw_post, ldlp, logpdf, info);                             \
  }                                                                                                                 \
  int blr_mean_and_cov_##SUF(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, const T* X,             \
                             int64_t ldx, int noise_kind, const T* s, int64_t lds, int prior_kind, const T* mw,     \
                             const T* Lw, int64_t ldl, T* mean, T* C, int64_t ldc, int32_t* info) {                 \
    return mean_and_cov<T>(h, memspace, layout, D, N, X, ldx, noise_kind, s, lds, prior_kind, mw, Lw, ldl, mean,    \
                           C, ldc, info);                                                                           \
  }                                                                                                                 \
  int blr_apply_weights_##SUF(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const T* X, \
                              int64_t ldx, const T* W, int64_t ldw, T* Y, int64_t ldy) {                            \
    return apply_weights<T>(h, memspace, layout, D, N, S, X, ldx, W, ldw, Y, ldy);                                  \
  }                                                                                                                 \
  int blr_rand_dense_noise_##SUF(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S,          \
                                 const T* X, int64_t ldx, const T* Sy, int64_t ldsy, int prior_kind, const T* mw,   \
                                 const T* Lw, int64_t ldl, const T* Z1, int64_t ldz1, const T* Z2, int64_t ldz2,    \
                                 T* Y, int64_t ldy) {                                                               \
    return rand_dense_noise<T>(h, memspace, layout, D, N, S, X, ldx, Sy, ldsy, prior_kind, mw, Lw, ldl, Z1, ldz1,   \
                               Z2, ldz2, Y, ldy);                                                                   \
  }

BLR_DEFINE(f64, double)
BLR_DEFINE(f32, float)

// host arithmetic only: no handle, no device (blr_kfold_ragged_plan.hpp)
int blr_kfold_ragged_fold_offsets(int64_t B, const int64_t* offsets, int64_t F, int64_t* fold_offsets) {
  if (const int rc = kfold_ragged_shape_check(nullptr, B, offsets, F)) return rc;
  if (!fold_offsets) return -21;
  kfold_ragged_fold_offsets(offsets, B, F, fold_offsets);
  return 0;
}

// host arithmetic only: no handle, no device (blr_kfold_large_ragged_plan.hpp)
int blr_kfold_large_ragged_fold_sizes(int64_t B, const int64_t* offsets, int64_t K, int64_t* fold_sizes) {
  if (B < 0 || B > (1 << 30)) return -4;
  if (const int rc = ragged_offsets_check(nullptr, B, offsets)) return rc;
  if (K < 1 || K > kFoldLargeMaxFolds) return -3;
  if (B > 0 && !fold_sizes) return -7;
  kflr_fold_sizes(offsets, B, K, fold_sizes);
  return 0;
}
int blr_kfold_large_ragged_fold_offsets(int64_t B, const int64_t* offsets, const int64_t* fold_sizes, int64_t* fold_offsets) {
  if (B < 0 || B > (1 << 30)) return -4;
  if (const int rc = ragged_offsets_check(nullptr, B, offsets)) return rc;
  if (const int rc = kfold_large_ragged_sizes_check(nullptr, B, offsets, fold_sizes)) return rc;
  if (!fold_offsets) return -21;
  kflr_fold_offsets(offsets, fold_sizes, B, fold_offsets);
  return 0;
}

// ---- multi-GPU exchange: RCCL called directly ------------------------------------------------------
int blr_comm_unique_id(void* id128) {
  if (!id128) return -1;
  if (!rccl().ok) return -2001;
  ncclUniqueId id;
  static_assert(sizeof(ncclUniqueId) == BLR_UNIQUE_ID_BYTES, "ncclUniqueId is 128 bytes");
  ncclResult_t r = rccl().GetUniqueId(&id);
  if (r != ncclSuccess) return -(2000 + (int)r);
  memcpy(id128, &id, sizeof id);
  return 0;
}

int blr_comm_init(blr_handle* h, int nranks, int rank, const void* id128) {
  if (!h) return -1;
  h->err.clear();
  if (nranks < 1) return bad_arg(h, 2, "nranks < 1");
  if (rank < 0 || rank >= nranks) return bad_arg(h, 3, "rank out of range");
  if (!id128) return bad_arg(h, 4, "unique id is NULL");
  if (h->comm) return bad_arg(h, 1, "the handle already has a communicator (blr_comm_destroy first)");
  if (!rccl().ok) { h->err = rccl().why; return -2001; }
  HIP_TRY(h, hipSetDevice(h->device));
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  ncclResult_t r = rccl().CommInitRank(&h->comm, nranks, id, rank);
  if (r != ncclSuccess) { h->comm = nullptr; return rccl_fail(h, r, "ncclCommInitRank"); }
  h->comm_size = nranks;
  h->comm_rank = rank;
  return 0;
}

int blr_comm_destroy(blr_handle* h) {
  if (!h) return -1;
  if (!h->comm) return 0;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  ncclResult_t r = rccl().CommDestroy(h->comm);
  h->comm = nullptr;
  h->comm_size = 0;
  h->comm_rank = 0;
  return r == ncclSuccess ? 0 : rccl_fail(h, r, "ncclCommDestroy");
}

int blr_comm_size(blr_handle* h) { return h && h->comm ? h->comm_size : (h ? 1 : -1); }
int blr_comm_rank(blr_handle* h) { return h && h->comm ? h->comm_rank : (h ? 0 : -1); }

int blr_logpdf_allgather_sum(blr_handle* h, int64_t count, const double* logpdf_local, double* logpdf_all, double* total) {
  if (!h) return -1;
  h->err.clear();
  if (count < 0 || count > ((int64_t)1 << 30)) return bad_arg(h, 2, "count out of range");
  if (count > 0 && !logpdf_local) return bad_arg(h, 3, "logpdf_local is NULL");
  if (!logpdf_all) return bad_arg(h, 4, "logpdf_all is NULL");
  if (!total) return bad_arg(h, 5, "total is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  const int64_t world = h->comm ? h->comm_size : 1;
  if (h->comm) {
    ncclResult_t r = rccl().AllGather(logpdf_local, logpdf_all, (size_t)count, ncclDouble, h->comm, h->stream);
    if (r != ncclSuccess) return rccl_fail(h, r, "ncclAllGather");
  } else if (count > 0 && logpdf_all != logpdf_local) {
    HIP_TRY(h, hipMemcpyAsync(logpdf_all, logpdf_local, (size_t)count * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  }
  // the SAME fixed-order sum over the SAME gathered vector on every rank: identical bits for any rank count
  hipLaunchKernelGGL(logpdf_sum_kernel, dim3(1), dim3(kThreads), 0, h->stream, (const double*)logpdf_all, count * world, total);
  HIP_TRY(h, hipGetLastError());
  if (!h->async) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

int blr_allreduce_sum(blr_handle* h, int is_f64, void* buf, int64_t count) {
  if (!h) return -1;
  h->err.clear();
  if (!buf) return bad_arg(h, 3, "buf is NULL");
  if (count < 0) return bad_arg(h, 4, "count < 0");
  if (!h->comm || count == 0) return 0;  // one rank: the sum over ranks is the buffer itself
  HIP_TRY(h, hipSetDevice(h->device));
  ncclResult_t r = rccl().AllReduce(buf, buf, (size_t)count, is_f64 ? ncclDouble : ncclFloat, ncclSum, h->comm, h->stream);
  if (r != ncclSuccess) return rccl_fail(h, r, "ncclAllReduce");
  if (!h->async) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

// One regressor, its observations split over the ranks of the handle's communicator: statistics of the local columns, ONE
// in-place all-reduce of the (DP + 128) x DP statistics matrix and one of the two scalars, redundant finish on every rank.
#define BLR_DEFINE_NSHARDED(SUF, T, IS64)                                                                               \
  int blr_posterior_nsharded_##SUF(blr_handle* h, int layout, int64_t D, int64_t N_local, int64_t N_total, const T* X,  \
                                   int64_t ldx, const T* y, int noise_kind, const T* s, int prior_kind, const T* mw,    \
                                   const T* Lw, int64_t ldl, T* stats, int64_t lds, double* scal, T* mw_post,           \
                                   T* T_post, int64_t ldt, T* Lw_post, int64_t ldlp, double* logpdf, int32_t* info) {   \
    if (!h) return -1;                                                                                                  \
    const int64_t DP = (D + 127) / 128 * 128;                                                                           \
    int rc = gram_stats<T>(h, layout, D, N_local, X, ldx, y, noise_kind, s, mw, stats, lds, scal);                     \
    if (rc) return rc;                                                                                                  \
    if ((rc = blr_allreduce_sum(h, IS64, stats, lds * DP))) return rc;                                                  \
    if ((rc = blr_allreduce_sum(h, 1, scal, 2))) return rc;                                                             \
    return posterior_from_stats<T>(h, D, N_total, stats, lds, scal, prior_kind, mw, Lw, ldl, mw_post, T_post, ldt,      \
                                   Lw_post, ldlp, logpdf, info);                                                        \
  }
BLR_DEFINE_NSHARDED(f64, double, 1)
BLR_DEFINE_NSHARDED(f32, float, 0)
#undef BLR_DEFINE_NSHARDED

int blr_logpdf_sum(blr_handle* h, int memspace, int64_t B, const double* logpdf, double* total) {
  if (!h) return -1;
  h->err.clear();
  if (memspace != BLR_MEM_HOST && memspace != BLR_MEM_DEVICE) return bad_arg(h, 2, "memspace");
  if (B < 0) return bad_arg(h, 3, "B < 0");
  if (B > 0 && !logpdf) return bad_arg(h, 4, "logpdf is NULL");
  if (!total) return bad_arg(h, 5, "total is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  CallIO io(h, memspace);
  const double* lp = nullptr;
  double* tot = nullptr;
  int rc;
  if ((rc = io.in(logpdf, (size_t)B, &lp))) return rc;
  if ((rc = io.out(total, 1, &tot))) return rc;
  hipLaunchKernelGGL(logpdf_sum_kernel, dim3(1), dim3(kThreads), 0, h->stream, lp, B, tot);
  HIP_TRY(h, hipGetLastError());
  return io.finish();
}

}  // extern "C"
