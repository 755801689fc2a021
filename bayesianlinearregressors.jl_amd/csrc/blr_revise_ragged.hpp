// Condition and forget on RESIDENT states whose regressors received UNEQUAL numbers of observations (blr_update_factor_ragged_*,
// blr_downdate_factor_ragged_*).
//
// Replaces reference test/bayesian_linear_regression.jl:49-70 ("repeated conditioning": posterior(f'(X2, S2), y2)) under a map over
// posteriors that each received a different number of new observations.  The observations of all regressors are packed side by
// side as in blr_posterior_ragged_*; regressor b owns columns [offsets[b], offsets[b+1]) and its state sits at b * strideT.
//
// One workgroup per ACTIVE regressor, taken from a list the host sorted longest-first (blr_revise_ragged_plan.hpp); a regressor
// without observations costs no workgroup.  The kernels here are the bodies of rank1_sweep_kernel (blr_update.hpp) and
// downdate_lds_kernel (blr_downdate.hpp) -- the same device function, called with the regressor from the list and the slice from
// `offsets` -- so the bits of regressor b are those of the equal-count kernel with B = 1, k = k_b on its slice: independent of B,
// of the other regressors and of the position in the list.  The re-factorisation route of the update is fused_ragged_kernel
// (blr_ragged.hpp) in place, its `order` being the plan's refit list.
#pragma once
#include "blr_common.hpp"
#include "blr_update.hpp"
#include "blr_downdate.hpp"
#include "blr_revise_ragged_plan.hpp"

namespace blr {

static_assert(kReviseMaxD == kSweepMaxD && kReviseMaxD == kDowndateLdsMaxD && kReviseSweepMaxK == kSweepMaxK,
              "the host-only planner repeats the kernels' bounds");

template <typename T>
struct ReviseRaggedArgs {
  // X, y and (diagonal noise) s: the packed arrays' bases; strideX, stridey and k are unused; strides: isotropic noise only
  SweepArgs<T> s;
  const int64_t* offsets;  // [B + 1], device
  const int32_t* list;     // [gridDim.x], device: the regressors of this launch
};

// workgroup -> its regressor and the slice it owns
template <typename T>
struct ReviseSlice {
  int64_t reg;
  const T *Xg, *yg, *sg;
  int k;
  __device__ __forceinline__ explicit ReviseSlice(const ReviseRaggedArgs<T>& r) {
    reg = uni(r.list[blockIdx.x]);
    const int64_t o0 = uni(r.offsets[reg]);
    k = uni((int)(r.offsets[reg + 1] - o0));
    Xg = r.s.X + (r.s.layout == LAYOUT_COLVECS ? o0 * r.s.ldx : o0);
    yg = r.s.y + o0;
    sg = r.s.noise_kind == NOISE_DIAGONAL ? r.s.s + o0 : r.s.s + reg * r.s.strides;
  }
};

template <typename T>
__global__ __launch_bounds__(kThreads) void update_ragged_sweep_kernel(ReviseRaggedArgs<T> r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ReviseSlice<T> sl(r);
  rank1_sweep_body<T>(smem, r.s, sl.reg, sl.Xg, sl.yg, sl.sg, sl.k);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void downdate_ragged_kernel(ReviseRaggedArgs<T> r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ReviseSlice<T> sl(r);
  downdate_lds_body<T>(smem, r.s, sl.reg, sl.Xg, sl.yg, sl.sg, sl.k);
}

// k_b = 0: the state keeps its bits and is not inspected; logpdf = 0, info = 0
__global__ __launch_bounds__(kThreads) void revise_ragged_idle_kernel(const int64_t* offsets, int64_t B, double* logpdf, int32_t* info);

// the instantiations the library uses, defined in blr_revise_ragged.hip
#define BLR_REVISE_RAGGED_INSTANCES(X, T)                                        \
  X __global__ void update_ragged_sweep_kernel<T>(ReviseRaggedArgs<T>);          \
  X __global__ void downdate_ragged_kernel<T>(ReviseRaggedArgs<T>);
BLR_REVISE_RAGGED_INSTANCES(extern template, double)
BLR_REVISE_RAGGED_INSTANCES(extern template, float)

}  // namespace blr
