// Host-only state of the C ABI (blr_abi.hip includes this; blr_large_plan.hpp for BlrOptions): the run-time switches, the handle, its grow-only
// device buffers, and the call-scope object that stages BLR_MEM_HOST calls.  No kernel and no device code lives here.
#pragma once

#include "../../include/blr_mi355x.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the symbols are resolved with dlopen / dlsym on first use

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

// Run-time switches (A/B experiments and tests; the defaults are the measured best).  Read from the environment ONCE, when the
// handle is created (BLR_MI355X_<KEY>), and settable per handle with blr_set_option: no getenv on any launch path.
// One line per switch: the member, blr_set_option's key and the environment variable all come from these two tables.
#define BLR_FLAG_OPTIONS(X)                                                                                             \
  X(no_ldsdma, "NO_LDSDMA")                                                                                             \
  X(no_wave_kernel, "NO_WAVE_KERNEL")                                                                                   \
  X(no_gram_ring, "NO_GRAM_RING")                                                                                       \
  X(no_diag_split, "NO_DIAG_SPLIT")                                                                                     \
  X(no_xcd_swizzle, "NO_XCD_SWIZZLE")                                                                                   \
  X(no_mfma_project, "NO_MFMA_PROJECT")                                                                                 \
  X(plan_debug, "PLAN_DEBUG")                                                                                           \
  X(no_i8_gram, "NO_I8_GRAM")                                                                                           \
  X(no_marg_gemm, "NO_MARG_GEMM")                                                                                       \
  X(no_grad_gemm, "NO_GRAD_GEMM")                                                                                       \
  X(no_i8_diag, "NO_I8_DIAG")                                                                                           \
  X(no_i8_factor, "NO_I8_FACTOR")                                                                                       \
  X(no_i8_rowvecs, "NO_I8_ROWVECS")                                                                                     \
  X(no_i8_dense, "NO_I8_DENSE")                                                                                         \
  X(no_bf16x3, "NO_BF16X3")                                                                                             \
  X(no_planes, "NO_PLANES")                                                                                             \
  X(no_multi_planes, "NO_MULTI_PLANES") /* logpdf_multi at D > 128, fp32: the separate residual product + panel sweep */ \
  X(no_spec_rowmax, "NO_SPEC_ROWMAX")   /* exact row maxima (one more pass over X) instead of the sampled ones */       \
  X(no_fp16_planes, "NO_FP16_PLANES")                                                                                   \
  X(planes8, "PLANES8")                                                                                                 \
  X(no_i8_fallback, "NO_I8_FALLBACK")                                                                                   \
  X(no_downdate_lds, "NO_DOWNDATE_LDS") /* blr_downdate_factor_*: the global-memory kernel at every D */
// valued options: the key and the BlrOptions member function that parses its value (on = value is neither NULL nor "")
#define BLR_VALUE_OPTIONS(X)       \
  X("WAVE_SPLIT", set_wave_split)  \
  X("CHAIN_BATCH", set_chain_batch) \
  X("CHAIN_WS_MB", set_chain_ws_mb) \
  X("SWEEP", set_sweep)            \
  X("GRAM_SPLITS", set_gram_splits) \
  X("I8_PROBE_MIN", set_i8_probe_min) \
  X("I8_GROUPS", set_i8_groups)   \
  X("MAX_CHUNK", set_max_chunk)
// valued options of the host-only planners that only tests set (blr_ragged_items.hpp): parsed like the ones above, listed apart
#define BLR_PLANNER_OPTIONS(Y) Y("RAGGED_ITEM", set_ragged_item)

struct BlrOptions {
#define BLR_X(member, key) bool member = false;
  BLR_FLAG_OPTIONS(BLR_X)
#undef BLR_X
  int wave_split = 0;     // waves per regressor of the wave kernel: 0 = router, else 1 | 2 | 4
  int chain_batch = 0;    // regressors per shared launch at D > 128: 0 = as many as the workspace holds
  int i8_probe_min = 0;   // int8 route: batches beyond this many regressors start with a probe slice; 0 = kI8ProbeMin
  int i8_groups = 0;      // int8 route: digit groups kept, 0 = six under isotropic noise and seven under diagonal noise; 6 | 7 = that plan for both noise kinds
  int max_chunk = 0;      // regressors per chunk / slice of every batched entry point: 0 = the launch's own bound (tests: small groups cross every seam)
  int ragged_item = 0;    // observations per work item of the ragged marginals / LOO (blr_ragged_items.hpp): 0 = the planner's own (tests: short regressors cross item seams)
  long chain_ws_mb = 0;   // workspace bound of such a group in MiB: 0 = kChainWorkspace
  int sweep = 0;          // blr_update_factor_* route: 0 = router, 1 = always the Givens sweep, 2 = never
  int gs_fields = 0, gs_so = 0, gs_sd = 0, gs_nl = 0;  // GRAM_SPLITS = "off-diagonal,diagonal[,nlong]" (gs_fields = numbers parsed)
  static bool parse_long(const char* v, long& out) {  // the whole string must be a decimal number
    char* end = nullptr;
    const long x = strtol(v, &end, 10);
    if (end == v || *end != '\0') return false;
    out = x;
    return true;
  }
  // the parsers: 0, or -3 for a malformed value
  int set_wave_split(bool on, const char* value) {
    long v = 0;
    if (!on) { wave_split = 0; return 0; }
    if (!parse_long(value, v) || !(v == 1 || v == 2 || v == 4)) return -3;
    wave_split = (int)v;
    return 0;
  }
  int set_chain_batch(bool on, const char* value) {
    long v = 0;
    if (!on) { chain_batch = 0; return 0; }
    if (!parse_long(value, v) || v < 1 || v > 128) return -3;
    chain_batch = (int)v;
    return 0;
  }
  int set_i8_probe_min(bool on, const char* value) {
    long v = 0;
    if (!on) { i8_probe_min = 0; return 0; }
    if (!parse_long(value, v) || v < 256 || v > (1 << 20)) return -3;
    i8_probe_min = (int)v;
    return 0;
  }
  int set_i8_groups(bool on, const char* value) {
    long v = 0;
    if (!on) { i8_groups = 0; return 0; }
    if (!parse_long(value, v) || !(v == 6 || v == 7)) return -3;
    i8_groups = (int)v;
    return 0;
  }
  int set_max_chunk(bool on, const char* value) {
    long v = 0;
    if (!on) { max_chunk = 0; return 0; }
    if (!parse_long(value, v) || v < 1 || v > 65535) return -3;
    max_chunk = (int)v;
    return 0;
  }
  int set_ragged_item(bool on, const char* value) {
    long v = 0;
    if (!on) { ragged_item = 0; return 0; }
    if (!parse_long(value, v) || v < 1 || v > (1 << 30)) return -3;
    ragged_item = (int)v;
    return 0;
  }
  int set_chain_ws_mb(bool on, const char* value) {
    long v = 0;
    if (!on) { chain_ws_mb = 0; return 0; }
    if (!parse_long(value, v) || v < 1) return -3;
    chain_ws_mb = v;
    return 0;
  }
  int set_sweep(bool on, const char* value) {
    if (!on || !strcmp(value, "auto")) { sweep = 0; return 0; }
    if (!strcmp(value, "always")) { sweep = 1; return 0; }
    if (!strcmp(value, "never")) { sweep = 2; return 0; }
    return -3;
  }
  int set_gram_splits(bool on, const char* value) {
    gs_fields = gs_so = gs_sd = gs_nl = 0;
    if (on) gs_fields = sscanf(value, "%d,%d,%d", &gs_so, &gs_sd, &gs_nl);
    return (!on || gs_fields >= 2) ? 0 : -3;
  }
  // -> 0, -2 for an unknown key, -3 for a malformed value (the codes blr_set_option documents).  value NULL or "" = the built-in default
  int set(const char* key, const char* value) {
    if (!key) return -2;
    if (!strncmp(key, "BLR_MI355X_", 11)) key += 11;
    const bool on = value && *value;
#define BLR_X(member, k) if (!strcmp(key, k)) { member = on; return 0; }
    BLR_FLAG_OPTIONS(BLR_X)
#undef BLR_X
#define BLR_X(k, parser) if (!strcmp(key, k)) return parser(on, value);
    BLR_VALUE_OPTIONS(BLR_X)
    BLR_PLANNER_OPTIONS(BLR_X)
#undef BLR_X
    return -2;
  }
  void from_environment() {
    auto env = [](const char* k) { return getenv((std::string("BLR_MI355X_") + k).c_str()); };
    // boolean flags: a variable that is set -- even to the empty string -- switches the flag on
#define BLR_X(member, k) if (env(k)) member = true;
    BLR_FLAG_OPTIONS(BLR_X)
#undef BLR_X
    // valued options: an empty variable is ignored (the built-in default stays), a malformed one too
#define BLR_X(k, parser) if (const char* v = env(k)) { if (*v) (void)parser(true, v); }
    BLR_VALUE_OPTIONS(BLR_X)
    BLR_PLANNER_OPTIONS(BLR_X)
#undef BLR_X
  }
};

struct blr_handle;
inline int hip_fail(blr_handle* h, hipError_t e, const char* what);
#define HIP_TRY(h, expr)                                   \
  do {                                                     \
    hipError_t e__ = (expr);                               \
    if (e__ != hipSuccess) return hip_fail(h, e__, #expr); \
  } while (0)

// A grow-only device buffer of a handle.  Growing drains the handle's stream first (work in flight may still read the old
// block), frees, and allocates anew: the contents do not survive, and a steady-state call makes no driver call here at all.
struct DevBuf {
  char* p = nullptr;
  size_t bytes = 0;
  inline int reserve(blr_handle* h, size_t want, size_t floor = 0, bool zero = false);
  inline int release(blr_handle* h);
};

struct blr_handle {
  BlrOptions opt;
  int device = 0;
  int cus = 256;  // compute units of the device (MI355X: 256; a partitioned part reports its share)
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  bool async = false;
  std::string err = "";
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<void*> staged;  // device buffers of the HOST-memspace calls in progress (CallIO: a scope owns those past its base)
  DevBuf ws;      // scratch (factors, info); never smaller than kWsFloor
  DevBuf feat;    // feature matrix of blr_posterior_rff_*
  DevBuf aux;     // triangular-inverse images of the marginal stream (blr_marginals.hpp), temporaries of logpdf_multi
  DevBuf i8side;  // what the int8 route prepares per call (y / sqrt(s), 1 / sqrt(s), ... -- launch_fused_i8); a buffer of its own because
                  // logpdf_multi carves ITS temporaries from `aux` around a nested update that may take that route
  DevBuf loo_ws;  // chunk of mean / latent variance / logpdf of blr_loo_batched_* (the marginal routes it calls use ws and aux themselves)
  DevBuf ragged_meta;  // offsets[B + 1] and the longest-first order[B] of blr_posterior_ragged_* (a buffer of its own: the D > 128 route runs the batched pipeline, which uses ws)
  DevBuf multi_ws;  // blr_posterior_multi_batched_*: evidence of column 0 per regressor, and the factors when the caller passed T_post = NULL;
                    // blr_update_multi_factor_* / blr_downdate_multi_factor_*: that evidence and the diagonal of the factor before the call
  DevBuf cov_ws;    // blr_mean_and_cov_batched_*: the rows Z = X'L^-T of a chunk of regressors (blr_cov_batched.hpp)
  std::vector<int64_t> ragged_host;  // host image of that buffer (kept: no allocation per call in the steady state)
  // wavefront back substitution (D > 128): tagged exchange buffer (unsigned long long granules; never smaller than kXchgFloor),
  // start-order ticket counter, launch epoch
  DevBuf xchg;
  static constexpr size_t kWsFloor = (size_t)1 << 20, kXchgFloor = (size_t)1 << 18;
  // blr_release_workspace hands these back; xchg, ticket and stats_dev stay (their contents carry epochs and counters)
  std::array<DevBuf*, 8> releasable() { return {&ws, &feat, &aux, &i8side, &loo_ws, &ragged_meta, &multi_ws, &cov_ws}; }
  // counters behind blr_get_stat: [0] regressors the int8 route handed back to the fp64 kernel (cumulative); [3] degenerate
  // leverages of blr_loo_batched_* (cumulative); [4] degenerate folds of blr_kfold_batched_* (cumulative); [8 + 2 k + {0, 1}]:
  // hand-backs of slice k of the current call (two banks, alternating), read by the NEXT slice's launch (launch_fused_i8)
  unsigned long long* stats_dev = nullptr;
  unsigned long long i8_attempted = 0;   // regressors sent down the int8 route (host count)
  unsigned i8_slices = 0;                // parity = bank of the per-slice hand-back counter
  const char* route = "none";            // kernel family the most recent posterior dispatch launched (blr_last_route)
  // set by logpdf_multi around its update of column 0 (fp32, ColVecs, D > 128, S <= 128): the other columns of Y ride through the SAME
  // planes pass, Gram launch and factorisation as one more row block (blr_planes.hpp); the group function leaves what the finish needs
  struct MultiSrc { const void* Y; int64_t ldY; int S; void* Abar; int64_t lda; void* Tfull; int DP; double* qsp; int nq; bool done; };
  MultiSrc* multi_src = nullptr;
  // Regressors per launch: every batched entry point cuts its batch by its own bound (grid.y, a workspace, the images) and, when
  // option MAX_CHUNK is set, by that as well -- the same loop, the same pointer arithmetic, more rounds of it.
  int64_t cap_chunk(int64_t natural) const { return opt.max_chunk > 0 ? std::min<int64_t>(natural, opt.max_chunk) : natural; }
  int64_t last_chunks = 0;               // chunks / slices of regressors the most recent call launched (blr_get_stat "last_chunks"): 1 at
                                         // every entry, then whatever the call's chunk loop counts
  void count_chunks(int64_t B, int64_t chunk) { last_chunks = (B + chunk - 1) / chunk; }
  // blr_update_factor_ragged_* / blr_downdate_factor_ragged_*: the list lengths of the most recent call's plan (blr_get_stat
  // "ragged_sweep" / "ragged_refit" / "ragged_idle"; blr_revise_ragged_plan.hpp)
  std::array<int64_t, 3> ragged_lists{};
  // The variance route of the most recent blr_marginals_batched_* call (blr_get_stat "marg_block_rt" / "marg_block_walk" /
  // "marg_block_renumbered"): tile height of marg_blocksub_kernel (0: the call ran elsewhere), trips of its busiest workgroup
  // (the largest ceil(ntiles / grid.x) over the call's launches), and whether any launch met the kernel's renumbering condition
  struct MargBlockRoute {
    int rt = 0; int64_t walk = 0; int renumbered = 0;
    void launch(int tile_rows, int64_t ntiles, int64_t gx, int nb) {
      rt = tile_rows;
      walk = std::max<int64_t>(walk, (ntiles + gx - 1) / gx);
      if (nb > 1 && (gx * nb) % 8 == 0) renumbered = 1;
    }
  } marg_block;
  // The kernels of the most recent blr_sample_weights_* / blr_apply_weights_* / blr_rand_* / blr_rand_batched_* call (blr_get_stat
  // "draw_route"): cleared at their entry, then or-ed together by the host code that picks each launch.  One weights bit (UVEC rides on
  // MFMA: sample_weights_mfma_kernel's 16-byte loader of U, the kernel's own predicate evaluated on the host for this stat only)
  // and at most one projection bit (none: weights only, or N = 0).
  enum DrawRoute : int64_t {
    DRAW_W_DIAG = 1, DRAW_W_MFMA = 2, DRAW_W_UVEC = 4, DRAW_W_LARGE = 8, DRAW_W_BATCHED_NS1 = 16, DRAW_W_BATCHED_NS4 = 32,
    DRAW_P_FUSED = 64, DRAW_P_SCALAR = 128, DRAW_P_MFMA = 256
  };
  int64_t draw_route = 0;
  int64_t route_i8_B = 0;               // > 0: that dispatch took the int8 route with this many regressors (blr_last_route looks at its hand-backs)
  std::string route_buf;
  unsigned* ticket = nullptr;     // [0], [2], [3]: wavefront solve (tickets, done, launch count); [16 + 128 bank + g]: arrivals of panel_chain_kernel
  unsigned panel_launches = 0;    // parity = the bank of arrival words the next panel launch counts in (it clears the other one)
  // kernels whose dynamic-LDS limit has been raised on this handle's device (hipFuncSetAttribute is per device and costs a
  // driver call: once per (handle, kernel), not once per launch -- it sat on the launch path of the 5 us wave kernel)
  std::unordered_map<const void*, size_t> lds_limit;
  // multi-round Gram launches: (row blocks, N, slots) -> (off-diagonal ranges, diagonal ranges, tiles with one range less)
  std::map<std::array<int, 3>, std::array<int, 3>> gram_plans;
  // RCCL communicator of blr_comm_init (one rank per handle / GPU); NULL until then
  ncclComm_t comm = nullptr;
  int comm_size = 0, comm_rank = 0;
};

inline int hip_fail(blr_handle* h, hipError_t e, const char* what) {
  if (h) {
    h->err = std::string(what) + ": " + hipGetErrorString(e);
  }
  return -(1000 + (int)e);
}

inline int DevBuf::reserve(blr_handle* h, size_t want, size_t floor, bool zero) {
  if (want <= bytes) return 0;
  int rc = release(h);
  if (rc) return rc;
  want = std::max(want, floor);
  HIP_TRY(h, hipMalloc((void**)&p, want));
  if (zero) HIP_TRY(h, hipMemsetAsync(p, 0, want, h->stream));
  bytes = want;
  return 0;
}
inline int DevBuf::release(blr_handle* h) {
  if (!p) return 0;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipFree(p));
  p = nullptr;
  bytes = 0;
  return 0;
}

// The device view of one ABI call's arguments.  Under BLR_MEM_DEVICE `in` / `out` hand the caller's pointers through and the
// object costs nothing: no allocation, no driver call.  Under BLR_MEM_HOST every array gets a device buffer of its own (one
// hipMalloc each, its copy on the handle's stream), `finish` copies every registered output back with the extent it was
// registered with, and the destructor frees the buffers -- on early error returns too.  Scopes nest: an inner one frees only
// what it added (the buffers live in blr_handle::staged; the outputs in fixed storage here, so no call allocates host memory
// beyond that vector's growth on its first uses).
class CallIO {
 public:
  CallIO(blr_handle* hh, int memspace) : h(hh), host(memspace == BLR_MEM_HOST), base(hh->staged.size()) {}
  CallIO(const CallIO&) = delete;
  CallIO& operator=(const CallIO&) = delete;
  ~CallIO() {
    for (size_t i = base; i < h->staged.size(); ++i) (void)hipFree(h->staged[i]);
    h->staged.resize(base);
  }
  // an input of `count` elements.  HOST: p NULL or count 0 -> *dev = NULL
  template <typename T>
  int in(const T* p, size_t count, const T** dev) {
    if (!host) { *dev = p; return 0; }
    void* d = nullptr;
    const int rc = upload(p, count * sizeof(T), &d);
    *dev = static_cast<const T*>(d);
    return rc;
  }
  // an output (or an array updated in place) of `count` elements; p NULL: not wanted, neither staged nor copied back.
  // Outputs with gaps (ld > rows, stride > extent) keep the caller's bytes in the gaps: the current host contents go in first.
  template <typename T>
  int out(T* p, size_t count, T** dev) {
    if (!host) { *dev = p; return 0; }
    void* d = nullptr;
    const int rc = upload(p, count * sizeof(T), &d);
    *dev = static_cast<T*>(d);
    if (rc || !d) return rc;
    if (nouts == kMaxOuts) return hip_fail(h, hipErrorInvalidValue, "CallIO: too many outputs (internal)");
    outs[nouts++] = Out{p, d, count * sizeof(T)};
    return 0;
  }
  // a device temporary of this call, in either memspace (uninitialised; at least one element)
  template <typename T>
  int tmp(size_t count, T** dev) {
    void* d = nullptr;
    HIP_TRY(h, hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)));
    h->staged.push_back(d);
    *dev = static_cast<T*>(d);
    return 0;
  }
  // HOST: the outputs travel back in the order they were registered, then the stream is drained.  DEVICE: drained unless the
  // handle is asynchronous -- or this scope holds temporaries, which the destructor is about to free.
  int finish() {
    for (int i = 0; i < nouts; ++i) HIP_TRY(h, hipMemcpyAsync(outs[i].host, outs[i].dev, outs[i].bytes, hipMemcpyDeviceToHost, h->stream));
    nouts = 0;
    if (host || !h->async || h->staged.size() > base) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return 0;
  }

 private:
  int upload(const void* p, size_t bytes, void** dev) {
    *dev = nullptr;
    if (!p || bytes == 0) return 0;
    HIP_TRY(h, hipMalloc(dev, bytes));
    h->staged.push_back(*dev);
    HIP_TRY(h, hipMemcpyAsync(*dev, p, bytes, hipMemcpyHostToDevice, h->stream));
    return 0;
  }
  struct Out { void* host; const void* dev; size_t bytes; };
  static constexpr int kMaxOuts = 8;  // logpdf_grad_batched has the most
  blr_handle* const h;
  const bool host;
  const size_t base;
  Out outs[kMaxOuts];
  int nouts = 0;
};
