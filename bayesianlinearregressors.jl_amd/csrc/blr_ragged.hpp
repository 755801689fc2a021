// Fused per-regressor inference for a batch whose regressors have UNEQUAL observation counts (blr_posterior_ragged_*).
//
// Replaces reference src/bayesian_linear_regression.jl:55-58 (logpdf), :60-69 (posterior), :72-89 under a map over fxs of different
// lengths.  The observations of all regressors are packed side by side; regressor b owns columns [offsets[b], offsets[b+1]).
//
// The kernel is fused_small_kernel's loop (blr_fused_small.hpp) with two differences:
//   - workgroup i takes regressor order[i], order[i + gridDim.x], ...: the host sorts the regressors by descending count, so the
//     hardware's in-order workgroup dispatch is longest-first list scheduling.  No atomics, no ticket counter.
//   - the regressor's slice (X, y, diagonal s, N) comes from `offsets` instead of one N and a stride: ragged_slice rewrites those
//     four fields of the LDS context that glue_prior has just filled, and ragged_finish takes N from there for the evidence.
// Everything else -- glue_prior, phase_gram, glue_after_gram, phase_chol, phase_backsolve -- is the same code on the same data, so the
// bits of regressor b are those of fused_small_kernel<T, NB, MODE> on its slice: independent of B, of the other regressors and of the
// position in `order`.
//
// The phase functions have internal linkage and are compiled once per translation unit for all their callers there: this kernel
// is instantiated in a unit of its own (blr_ragged.hip) and carries fused_small_kernel's launch bounds.
#pragma once
#include "blr_common.hpp"
#include "blr_fused_small.hpp"

namespace blr {

template <typename T>
struct RaggedArgs {
  // FIRST member: the glue phases of fused_small_kernel read it through the kernarg pointer.  X, y and (diagonal noise) s are the
  // packed arrays' bases with strideX = stridey = strides = 0; N is unused; B counts the regressors
  PosteriorArgs<T> p;
  const int64_t* offsets;  // [B + 1], device
  const int32_t* order;    // [B], device: regressor indices by descending count, ties by index
};
template <typename T>
using RaggedArgPtr = const __attribute__((address_space(4))) RaggedArgs<T>*;

// the regressor's slice of the packed arrays -> LDS context (after glue_prior, which filled it from the bases)
template <typename T, int NB>
BLR_PHASE void ragged_slice(char* smem, RaggedArgPtr<T> rp, int reg) {
  using C = SmallCfg<T, NB>;
  const __attribute__((address_space(4))) RaggedArgs<T>& r = *rp;
  RegCtx<T>* ctx = reinterpret_cast<RegCtx<T>*>(smem + C::OFF_CTX);
  if (threadIdx.x == 0) {
    const int64_t o0 = r.offsets[reg], o1 = r.offsets[reg + 1];
    ctx->X = r.p.X + (r.p.layout == LAYOUT_COLVECS ? o0 * r.p.ldx : o0);
    ctx->y = r.p.y + o0;
    if (r.p.noise_kind == NOISE_DIAGONAL) ctx->s = r.p.s + o0;
    ctx->N = (int)(o1 - o0);
  }
  __syncthreads();
}

// glue_finish with the regressor's own count in the evidence (:84 + :57)
template <typename T, int NB>
BLR_PHASE void ragged_finish(char* smem, RaggedArgPtr<T> rp, int reg, int info) {
  using C = SmallCfg<T, NB>;
  const __attribute__((address_space(4))) PosteriorArgs<T>& a = rp->p;
  T* const bvec = reinterpret_cast<T*>(smem + C::OFF_B);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  RegCtx<T>* ctx = reinterpret_cast<RegCtx<T>*>(smem + C::OFF_CTX);
  const int tid = threadIdx.x;
  if (info != 0) {
    if (tid == 0) {
      a.info[reg] = info;
      if (a.logpdf) a.logpdf[reg] = __longlong_as_double(0x7ff8000000000000LL);
    }
    return;
  }
  if (a.mw_post && tid < a.D) a.mw_post[(int64_t)reg * a.stride_mwpost + tid] = (a.mw + (int64_t)reg * a.stridemw)[tid] + bvec[tid];  // :68
  if (tid == 0) {
    a.info[reg] = 0;
    if (a.logpdf) {
      const double LOG2PI = 1.8378770664093454835606594728112;
      a.logpdf[reg] = -0.5 * ((double)ctx->N * LOG2PI + scr[5] + scr[4] + scr[7] - ctx->logdet_Lw - scr[6]);  // :84 + :57
    }
  }
}

template <typename T, int NB, int MODE /* data loader: 0 ColVecs generic, 1 RowVecs, 4 ColVecs LDS-DMA */>
__global__ __launch_bounds__(kThreads, (NB <= 4 ? 4 : (sizeof(T) == 4 ? BLR_F32_WAVES_PER_SIMD : 2))) void fused_ragged_kernel(RaggedArgs<T> r_kernarg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RaggedArgPtr<T> rp = (RaggedArgPtr<T>)__builtin_amdgcn_kernarg_segment_ptr();
  static_assert(offsetof(RaggedArgs<T>, p) == 0, "the glue of fused_small_kernel reads PosteriorArgs at the kernarg pointer");
  const KernArgPtr<T> ap = (KernArgPtr<T>)rp;
  const __attribute__((address_space(4))) PosteriorArgs<T>& a = *ap;
  for (int i = blockIdx.x; i < a.B; i += gridDim.x) {
    const int reg = rp->order[i];
    if (glue_prior<T, NB>(smem, ap, reg) != 0) continue;               // prior (:78); context from the bases
    ragged_slice<T, NB>(smem, rp, reg);                                // ... and the slice
    phase_gram<T, NB, MODE>(smem);                                     // streaming Gram -> P, bvec, scr[4..5]
    if (glue_after_gram<T, NB>(smem, ap, reg) != 0) continue;          // noise check (:79), Lw' (:92)
    const int info = phase_chol<T, NB>(smem, a.D, 1);                  // :86
    if (info == 0) phase_backsolve<T, NB>(smem, a.D, a.T_post ? a.T_post + (int64_t)reg * a.strideT : (T*)nullptr, a.ldt);
    ragged_finish<T, NB>(smem, rp, reg, info);
  }
}

// ---- host side of the instantiations (blr_ragged.hip), used by blr_abi.hip ---------------------------------------------------------
// mode: 0, 1 or 4; NB: 1 .. 8.  ragged_kernel_ptr is what hipFuncSetAttribute wants (per device: blr_abi.hip, set_lds_once)
const void* ragged_kernel_ptr_f64(int NB, int mode);
const void* ragged_kernel_ptr_f32(int NB, int mode);
size_t ragged_kernel_lds_f64(int NB);
size_t ragged_kernel_lds_f32(int NB);
void ragged_kernel_launch_f64(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedArgs<double>& a);
void ragged_kernel_launch_f32(int NB, int mode, unsigned grid, hipStream_t stream, const RaggedArgs<float>& a);

}  // namespace blr
