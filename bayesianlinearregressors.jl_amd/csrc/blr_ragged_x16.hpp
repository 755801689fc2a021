// Fused per-regressor inference on 16-bit features for a batch whose regressors have UNEQUAL observation counts
// (blr_posterior_ragged_x16): K14's packing and longest-first order on K31's streaming Gram, and a cut of the long
// regressors into work items (K26's planner, blr_ragged_items.hpp) that the posterior did not have on any data type.
//
// Whole regressors (count <= W): ragged_x16_kernel<FMT, NB, ROW>, one workgroup per regressor, longest first.  It is
// fused_x16_kernel's loop with the regressor's slice taken from `offsets`; the loader is chosen PER REGRESSOR -- a RowVecs slice
// starts 2 offsets[b] bytes into a row, so only a slice with offsets[b] % 8 == 0 can travel by LDS-DMA -- as a workgroup-uniform
// branch between two noinline phases.  phase_gram_x16r is phase_gram_x16 (blr_fused_x16.hpp) statement by statement on the same
// LDS layout, fed from the LDS context instead of `rp->X + reg * strideX`: the same arithmetic in the same order, so the bits of a
// whole regressor are those of blr_posterior_batched_x16 at B = 1 on its slice.
//
// Cut regressors (count > W): two launches.
//   ragged_x16_part_kernel<FMT, NB, ROW>: one workgroup per item of at most W observations.  The same stream (x16r_stream) with
//     weight 1 instead of 1 / sigma^2, then the partials of the item go to handle workspace, slot = the item's index among the cut
//     items of the chunk:
//       G[slot][PACKED]  fp32  raw packed lower triangle of X_item X_item' (padded to 16 NB rows), straight from the accumulators
//       b[slot][DP]      fp64  X_item r_item, r = y - X'mw formed directly per observation as K31 forms it
//       q[slot]          fp64  sum r^2
//     An item starts at a multiple of W (a multiple of 64) observations of its regressor: its 32-observation stages are the
//     regressor's own, and its alignment is that of the regressor's slice.
//   ragged_x16_finish_kernel<NB>: one workgroup per cut regressor.  Sums the regressor's partials in item order IN DOUBLE (a fixed
//     order; G is rounded to fp32 once, after the sum, so the cut costs no accuracy against the uncut fp32 accumulation), applies
//     1 / sigma^2 and the prior as phase_gram_x16 does, and runs the fp32 route's glue_after_gram / phase_chol / phase_backsolve and
//     the evidence with the regressor's own count.  The bits of a cut regressor are a function of its slice and W alone.
//
// The phase functions have internal linkage: the kernels are instantiated in a unit of their own (blr_ragged_x16.hip) and carry
// fused_x16_kernel's launch bounds; no existing code object changes.
#pragma once
#include "blr_common.hpp"
#include "blr_fused_small.hpp"
#include "blr_fused_x16.hpp"
#include "blr_ragged.hpp"

namespace blr {

struct RaggedX16Item {
  int32_t reg;    // regressor (index into the call's batch)
  int32_t first;  // first observation of the regressor this item covers (a multiple of W)
  int32_t count;  // observations it covers (<= W)
  int32_t slot;   // where its partials go
};

struct RaggedX16Args {
  // FIRST member: the glue phases of fused_small_kernel read it through the kernarg pointer.  p.X = NULL; p.y and p.s are the packed
  // y's base and the variances' base with stridey = 0 and strides = 0 / 1; p.N is unused; every array is indexed by the regressor
  PosteriorArgs<float> p;
  const unsigned short* X;     // packed 16-bit features (p.ldx in elements)
  const int64_t* offsets;      // [B + 1] of the call, device
  const int32_t* order;        // ragged_x16_kernel: its regressors, longest first; ragged_x16_finish_kernel: the cut regressors
  const int32_t* slot0;        // ragged_x16_finish_kernel: first partial slot of order[i] (its items follow one another)
  const RaggedX16Item* items;  // ragged_x16_part_kernel
  int32_t nwork;               // entries of `order` / of `items` this launch takes
  int32_t W;                   // observations per item
  int32_t dma_ok;              // the call's X may travel by LDS-DMA (aligned base, ldx % 8 == 0, ColVecs: D % 8 == 0)
  float* partG;                // [slots][PACKED]
  double* partB;               // [slots][DP]
  double* partQ;               // [slots]
};
using RaggedX16ArgPtr = const __attribute__((address_space(4))) RaggedX16Args*;

#ifndef BLR_X16_DECLS_ONLY

// ---- the stream of phase_gram_x16 over N observations at X (ColVecs: column n at X + n ldx; RowVecs: at X + n) -> acc, vec ----------
// (region 0 of the LDS layout must be free on entry; on exit the ring is dead and every wave is past the final barrier)
template <int FMT, int NB, int MODE>
__device__ __forceinline__ void x16r_stream(char* smem, const BLR_GLOBAL unsigned short* X, const BLR_GLOBAL float* y,
                                            const BLR_GLOBAL float* mw, int64_t ldx, int D, int N, float wiso,
                                            AccArr<float, NB>& acc, X16Vec<NB, (MODE & 1) != 0>& vec, int tid, int wave, int lane) {
  using C = SmallCfg<float, NB>;
  using XC = X16Cfg<NB>;
  constexpr bool ROW = (MODE & 1) != 0, FAST = MODE >= 2;
  BLR_LDS char* const lds = (BLR_LDS char*)smem;
  BLR_LDS float* const ybuf = reinterpret_cast<BLR_LDS float*>(lds + C::OFF_Y);  // [NS][32]
  float* const mwl = reinterpret_cast<float*>(smem + C::OFF_MW);
  static_assert(XC::NS * XC::SO <= 128, "ybuf holds the y of every ring slot");

  if (tid < C::DP) mwl[tid] = tid < D ? mw[tid] : 0.0f;
  __syncthreads();  // region 0 is free, mw is visible

  vec.init(mwl, lane);
  FragLane<NB, ROW> fl;
  fl.init(lane);

  const int nst = (N + XC::SO - 1) / XC::SO;
  const int nfull = FAST ? N / XC::SO : 0;  // stages 0 .. nfull - 1 travel by LDS-DMA
  // per-lane source of this wave's pieces (piece p = wave + 4 j): byte offset from the stage's base, or the zero block
  int64_t poff[XC::PW];
  bool pin[XC::PW];
#pragma unroll
  for (int j = 0; j < XC::PW; ++j) {
    const int p = wave + kWaves * j;
    if constexpr (ROW) {
      const int d = 16 * p + (lane & 15);
      pin[j] = FAST && d < D;
      poff[j] = ((int64_t)d * ldx + 8 * (lane >> 4)) * 2;
    } else {
      const int ch = p * 64 + lane, o = ch / (2 * NB), d0 = 8 * (ch % (2 * NB));
      pin[j] = FAST && d0 < D;
      poff[j] = ((int64_t)o * ldx + d0) * 2;
    }
  }
  const int npw = (NB - wave + kWaves - 1) / kWaves;            // pieces this wave issues per DMA stage (uniform)
  const int pwt = FAST ? npw + (wave == 0 ? 1 : 0) : 0;         // ... plus the y piece of wave 0
  const unsigned lds_base = lds_addr_of(smem), ybuf_addr = lds_addr_of(smem + C::OFF_Y);
  const uint64_t zero_addr = (uint64_t)(uintptr_t)g_x16_zero;
  auto issue = [&](int t) {
    const int sl = t & (XC::NS - 1), n0 = t * XC::SO;
    if (FAST && t < nfull) {
      const uint64_t sbase = (uint64_t)(uintptr_t)X + (uint64_t)((ROW ? (int64_t)n0 : (int64_t)n0 * ldx) * 2);
#pragma unroll
      for (int j = 0; j < XC::PW; ++j) {
        const int p = wave + kWaves * j;
        if (p < NB) glds16_nt(pin[j] ? sbase + (uint64_t)poff[j] : zero_addr, lds_base + (unsigned)(XC::slot_off(sl) + p * XC::PIECE));
      }
      if (wave == 0) glds_s<4, 32>((uint64_t)uni((int64_t)(uintptr_t)(y + n0)), (unsigned)(lane * 4), ybuf_addr + (unsigned)(sl * XC::SO * 4));
    } else {
      x16_stage_regs<NB, ROW>(lds + XC::slot_off(sl), ybuf + sl * XC::SO, X, ldx, y, D, N, n0, tid);
    }
  };
  auto stage_loop = [&](auto ws_tag) {
    constexpr int WS = decltype(ws_tag)::value;
    for (int t = 0; t < XC::LA && t < nst; ++t) issue(t);
    for (int t = 0; t < nst; ++t) {
      // this wave's pieces of stage t have landed: the younger DMA stages stay in flight
      const int last_dma = min(t + XC::LA - 1, nfull - 1);
      wait_vm(max(last_dma - t, 0) * pwt);
      __syncthreads();  // stage t is visible; the slot of stage t - 1 is free
      if (t + XC::LA < nst) issue(t + XC::LA);
      const int sl = t & (XC::NS - 1);
      BLR_LDS char* const slot = lds + XC::slot_off(sl);
      x16_mma_stage<FMT, NB, ROW, WS>(slot, fl, acc, wave);
      vec.template stage<FMT>(slot, ybuf + sl * XC::SO, wiso, wave, lane);
    }
  };
  if constexpr (NB == 8) {  // one copy of the loop per wave, wave index static (as phase_gram)
    switch (wave) {
      case 0: stage_loop(std::integral_constant<int, 0>{}); break;
      case 1: stage_loop(std::integral_constant<int, 1>{}); break;
      case 2: stage_loop(std::integral_constant<int, 2>{}); break;
      default: stage_loop(std::integral_constant<int, 3>{}); break;
    }
  } else {
    stage_loop(std::integral_constant<int, -1>{});
  }
  __syncthreads();  // the ring is dead
}

// A = Lw + G / sigma^2 in the accumulators: the prior precision in tile layout, or the factor's pseudo-observations in fp32
// (phase_gram_x16's prior step; region 0 of the LDS layout is free, mwl is filled)
template <int NB>
__device__ __forceinline__ void x16r_add_prior(char* smem, AccArr<float, NB>& acc, const BLR_GLOBAL float* Lw, int64_t ldl, int D,
                                               int prior_kind, float wiso, int tid, int wave, int lane) {
  using C = SmallCfg<float, NB>;
  float* const mwl = reinterpret_cast<float*>(smem + C::OFF_MW);
  if (prior_kind == PRIOR_UPPER_FACTOR) {
#pragma unroll
    for (int i = 0; i < C::TPW; ++i)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[i][v] *= wiso;
    float* const slot0 = reinterpret_cast<float*>(smem);
    float* const yb = reinterpret_cast<float*>(smem + C::OFF_Y);
    float* const wb = reinterpret_cast<float*>(smem + C::OFF_W);
    const WaveOps<NB> ops = make_wave_ops<float, NB>(wave);
    double bnone[NB], qnone = 0.0;
#pragma unroll
    for (int I = 0; I < NB; ++I) bnone[I] = 0.0;
    const int nprior = (D + C::NSC - 1) / C::NSC;
    for (int t = 0; t < nprior; ++t) {
      StageRegs<float, NB> pr;
      const int n0 = t * C::NSC;
      stage_load<float, NB, 2>(pr, Lw, ldl, D, D, n0, tid);
      pr.yv = 0.0f;
      pr.wv = (tid < C::NSC && n0 + tid < D) ? 1.0f : 0.0f;
      stage_store<float, NB, 2>(pr, slot0, yb, wb, tid);
      __syncthreads();
      compute_stage<float, NB, -1>(slot0, yb, wb, ops, acc, bnone, qnone, mwl, wave, lane, false);
      __syncthreads();
    }
  } else {
#pragma unroll
    for (int i = 0; i < C::TPW; ++i) {
      int I, K;
      const bool tile_ok = wave_tile(NB, wave, i, I, K);
      const int col = 16 * K + (lane & 15);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * I + Mfma<float>::crow(lane, v);
        float pv = 0.0f;
        if (prior_kind == PRIOR_DENSE) {  // UPPER triangle of the caller's matrix, as LAPACK 'U'
          const bool ok = tile_ok && row < D && col < D;
          const int lo = min(row, col), hi = max(row, col);
          const float val = Lw[ok ? (int64_t)hi * ldl + lo : 0];
          pv = ok ? val : 0.0f;
        } else {
          const bool ok = tile_ok && I == K && row == col && row < D;
          const float val = (I == K) ? Lw[ok ? row : 0] : 0.0f;
          pv = ok ? val : 0.0f;
        }
        acc[i][v] = pv + acc[i][v] * wiso;
      }
    }
  }
}

// accumulators -> packed lower triangle at P (LDS or global; the C layout of 16x16x32 is that of 16x16x4_f32)
template <int NB, typename Ptr>
__device__ __forceinline__ void x16r_store_packed(Ptr P, const AccArr<float, NB>& acc, int wave, int lane) {
  using C = SmallCfg<float, NB>;
#pragma unroll
  for (int i = 0; i < C::TPW; ++i) {
    int I, K;
    if (wave_tile(NB, wave, i, I, K)) {
      const int col = 16 * K + (lane & 15);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * I + Mfma<float>::crow(lane, v);
        if (col <= row) P[pidx(row, col)] = acc[i][v];
      }
    }
  }
}

// the regressor's slice of the packed arrays -> LDS context (after glue_prior, which filled it from the bases).  The context's X
// field -- a float pointer the 16-bit route never reads as one -- carries the slice's base.  Returns whether the slice may travel
// by LDS-DMA (block-uniform): the equal-count dispatch's rule on this slice
template <int NB, bool ROW>
BLR_PHASE int x16r_slice(char* smem, RaggedX16ArgPtr rp, int reg) {
  using C = SmallCfg<float, NB>;
  const __attribute__((address_space(4))) RaggedX16Args& r = *rp;
  RegCtx<float>* ctx = reinterpret_cast<RegCtx<float>*>(smem + C::OFF_CTX);
  const int64_t o0 = r.offsets[reg], o1 = r.offsets[reg + 1];
  if (threadIdx.x == 0) {
    ctx->X = reinterpret_cast<const float*>(r.X + (ROW ? o0 : o0 * r.p.ldx));
    ctx->y = r.p.y + o0;
    ctx->N = (int)(o1 - o0);
  }
  __syncthreads();
  return (r.dma_ok != 0 && (!ROW || (o0 & 7) == 0)) ? 1 : 0;
}

// =========================================================================================================
// phase 1 of a whole regressor (noinline): phase_gram_x16 on the slice in the LDS context.  On exit: what phase_gram<float, NB, *>
// leaves.  MODE: 0 ColVecs / 1 RowVecs through registers, 2 ColVecs / 3 RowVecs through the LDS-DMA ring
// =========================================================================================================
template <int FMT, int NB, int MODE>
BLR_PHASE void phase_gram_x16r(char* smem) {
  using C = SmallCfg<float, NB>;
  using acc4 = Mfma<float>::acc4;
  constexpr bool ROW = (MODE & 1) != 0;
  float* const P = reinterpret_cast<float*>(smem);
  double* const red = reinterpret_cast<double*>(smem);
  float* const bvec = reinterpret_cast<float*>(smem + C::OFF_B);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  const RegCtx<float>* ctx = reinterpret_cast<const RegCtx<float>*>(smem + C::OFF_CTX);

  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // nothing derived from tid may be hoisted above this phase
  const int lane = tid & 63;
  const int wave = uni(tid >> 6);
  const BLR_GLOBAL unsigned short* X = as_global(uni(reinterpret_cast<const unsigned short*>(ctx->X)));
  const BLR_GLOBAL float* y = as_global(uni(ctx->y));
  const BLR_GLOBAL float* s = as_global(uni(ctx->s));
  const BLR_GLOBAL float* mw = as_global(uni(ctx->mw));
  const BLR_GLOBAL float* Lw = as_global(uni(ctx->Lw));
  const int64_t ldx = uni(ctx->ldx), ldl = uni(ctx->ldl);
  const int D = uni(ctx->D), N = uni(ctx->N);
  const int prior_kind = uni(ctx->prior_kind);
  const float s_iso = s[0];
  const float wiso = 1.0f / s_iso;
  const int bad_noise_own = (s_iso > 0.0f) ? 0x7fffffff : 1;  // (reference :79; also catches NaN)

  acc4 acc[C::TPW];
#pragma unroll
  for (int i = 0; i < C::TPW; ++i) acc[i] = acc4{0.0f, 0.0f, 0.0f, 0.0f};
  X16Vec<NB, ROW> vec;
  x16r_stream<FMT, NB, MODE>(smem, X, y, mw, ldx, D, N, wiso, acc, vec, tid, wave, lane);
  x16r_add_prior<NB>(smem, acc, Lw, ldl, D, prior_kind, wiso, tid, wave, lane);

  // b partials -> LDS -> fixed-order sum
  vec.flush(red, wave, lane);
  __syncthreads();
  if (tid < C::DP) {
    double sum = 0.0;
#pragma unroll
    for (int p = 0; p < kWaves; ++p) sum += red[p * C::DP + tid];  // fixed order
    bvec[tid] = (float)sum;                                       // b = X S (y - X'mw)   (:57 Bt'dy, unwhitened)
  }
  const double quad = block_allreduce(vec.qacc, scr, tid);        // (y-m)' S (y-m)
  // (block_allreduce's barriers also fence the reads of `red` above)
  if (tid == 0) { scr[4] = quad; scr[5] = (double)N * log((double)s_iso); }
  {
    int* const iscr = reinterpret_cast<int*>(smem + C::OFF_SCR + 64);
    const int bad_noise = block_min_int(bad_noise_own, iscr, tid);
    if (tid == 0) iscr[6] = bad_noise;  // read back by glue_after_gram after the phase's final barrier
  }
  x16r_store_packed<NB>(P, acc, wave, lane);
  __syncthreads();
}

// the launch bounds of every kernel here are fused_x16_kernel's
#define BLR_X16R_BOUNDS(NB) __launch_bounds__(kThreads, ((NB) <= 4 ? 4 : BLR_F32_WAVES_PER_SIMD))

template <int FMT, int NB, bool ROW>
__global__ BLR_X16R_BOUNDS(NB) void ragged_x16_kernel(RaggedX16Args r_kernarg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RaggedX16ArgPtr rp = (RaggedX16ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
  static_assert(offsetof(RaggedX16Args, p) == 0, "the glue of fused_small_kernel reads PosteriorArgs at the kernarg pointer");
  const KernArgPtr<float> ap = (KernArgPtr<float>)rp;
  const __attribute__((address_space(4))) PosteriorArgs<float>& a = *ap;
  for (int i = blockIdx.x; i < rp->nwork; i += gridDim.x) {
    const int reg = rp->order[i];
    if (glue_prior<float, NB>(smem, ap, reg) != 0) continue;           // prior (:78); context from the bases
    if (x16r_slice<NB, ROW>(smem, rp, reg)) phase_gram_x16r<FMT, NB, ROW ? 3 : 2>(smem);  // ... and the slice; the loader it allows
    else phase_gram_x16r<FMT, NB, ROW ? 1 : 0>(smem);
    if (glue_after_gram<float, NB>(smem, ap, reg) != 0) continue;      // noise check (:79), Lw' (:92)
    const int info = phase_chol<float, NB>(smem, a.D, 1);              // :86
    if (info == 0) phase_backsolve<float, NB>(smem, a.D, a.T_post ? a.T_post + (int64_t)reg * a.strideT : (float*)nullptr, a.ldt);
    // (ragged_finish reads the PosteriorArgs at the head of its argument block and the count in the LDS context, nothing else)
    ragged_finish<float, NB>(smem, (RaggedArgPtr<float>)ap, reg, info);
  }
}

// ---- one item of a cut regressor (noinline): the stream with weight 1, then the partials -------------------------------------------
template <int FMT, int NB, int MODE>
BLR_PHASE void phase_part_x16r(char* smem, RaggedX16ArgPtr rp, int item_in) {
  using C = SmallCfg<float, NB>;
  using acc4 = Mfma<float>::acc4;
  constexpr bool ROW = (MODE & 1) != 0;
  const __attribute__((address_space(4))) RaggedX16Args& r = *rp;
  double* const red = reinterpret_cast<double*>(smem);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);

  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int wave = uni(tid >> 6);
  const RaggedX16Item it = r.items[uni(item_in)];
  const int reg = uni(it.reg), N = uni(it.count);
  const int64_t o = uni(r.offsets[reg] + (int64_t)it.first);
  const int64_t ldx = r.p.ldx;
  const int D = r.p.D;
  const BLR_GLOBAL unsigned short* X = as_global(uni(r.X + (ROW ? o : o * ldx)));
  const BLR_GLOBAL float* y = as_global(uni(r.p.y + o));
  const BLR_GLOBAL float* mw = as_global(uni(r.p.mw + (int64_t)reg * r.p.stridemw));
  const int64_t slot = uni(it.slot);

  acc4 acc[C::TPW];
#pragma unroll
  for (int i = 0; i < C::TPW; ++i) acc[i] = acc4{0.0f, 0.0f, 0.0f, 0.0f};
  X16Vec<NB, ROW> vec;
  x16r_stream<FMT, NB, MODE>(smem, X, y, mw, ldx, D, N, 1.0f, acc, vec, tid, wave, lane);

  x16r_store_packed<NB>(as_global(r.partG + slot * C::PACKED), acc, wave, lane);
  vec.flush(red, wave, lane);
  __syncthreads();
  if (tid < C::DP) {
    double sum = 0.0;
#pragma unroll
    for (int p = 0; p < kWaves; ++p) sum += red[p * C::DP + tid];  // fixed order
    r.partB[slot * C::DP + tid] = sum;
  }
  const double quad = block_allreduce(vec.qacc, scr, tid);
  if (tid == 0) r.partQ[slot] = quad;
}

template <int FMT, int NB, bool ROW>
__global__ BLR_X16R_BOUNDS(NB) void ragged_x16_part_kernel(RaggedX16Args r_kernarg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RaggedX16ArgPtr rp = (RaggedX16ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
  const __attribute__((address_space(4))) RaggedX16Args& r = *rp;
  for (int i = blockIdx.x; i < r.nwork; i += gridDim.x) {
    // an item's alignment is its regressor's (first % 64 == 0)
    const bool fast = r.dma_ok != 0 && (!ROW || (r.offsets[r.items[i].reg] & 7) == 0);
    __syncthreads();  // the previous item is done with LDS
    if (fast) phase_part_x16r<FMT, NB, ROW ? 3 : 2>(smem, rp, i);
    else phase_part_x16r<FMT, NB, ROW ? 1 : 0>(smem, rp, i);
  }
}

// ---- a cut regressor's partials -> what phase_gram<float, NB, *> leaves (noinline; after glue_prior) --------------------------------
template <int NB>
BLR_PHASE void phase_sum_parts_x16r(char* smem, RaggedX16ArgPtr rp, int reg_in, int first_slot_in) {
  using C = SmallCfg<float, NB>;
  using acc4 = Mfma<float>::acc4;
  const __attribute__((address_space(4))) RaggedX16Args& r = *rp;
  float* const P = reinterpret_cast<float*>(smem);
  float* const bvec = reinterpret_cast<float*>(smem + C::OFF_B);
  float* const mwl = reinterpret_cast<float*>(smem + C::OFF_MW);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  int* const iscr = reinterpret_cast<int*>(smem + C::OFF_SCR + 64);
  RegCtx<float>* ctx = reinterpret_cast<RegCtx<float>*>(smem + C::OFF_CTX);

  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int reg = uni(reg_in);
  const int N = uni((int)(r.offsets[reg + 1] - r.offsets[reg]));
  const int nit = (N + r.W - 1) / r.W;  // items, in the order of their observations
  const int64_t slot0 = uni(first_slot_in);
  const BLR_GLOBAL float* G = as_global(r.partG + slot0 * C::PACKED);
  const BLR_GLOBAL double* Bp = as_global(r.partB + slot0 * C::DP);
  const BLR_GLOBAL double* Qp = as_global(r.partQ + slot0);
  const BLR_GLOBAL float* s = as_global(uni(ctx->s));
  const BLR_GLOBAL float* mw = as_global(uni(ctx->mw));
  const BLR_GLOBAL float* Lw = as_global(uni(ctx->Lw));
  const int64_t ldl = uni(ctx->ldl);
  const int D = uni(ctx->D);
  const int prior_kind = uni(ctx->prior_kind);
  const float s_iso = s[0];
  const float wiso = 1.0f / s_iso;

  if (tid == 0) ctx->N = N;  // the evidence's count (ragged_finish)
  if (tid < C::DP) mwl[tid] = tid < D ? mw[tid] : 0.0f;

  // G = sum of the items' Gram matrices, in item order, in double, rounded once; into the accumulators' tile layout (an element
  // above the diagonal of a diagonal tile takes its mirror image: the packed store drops it)
  acc4 acc[C::TPW];
#pragma unroll
  for (int i = 0; i < C::TPW; ++i) {
    int I, K;
    const bool tile_ok = wave_tile(NB, wave, i, I, K);
    const int col = 16 * K + (lane & 15);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = 16 * I + Mfma<float>::crow(lane, v);
      const int e = tile_ok ? pidx(max(row, col), min(row, col)) : 0;
      double sum = 0.0;
      for (int k = 0; k < nit; ++k) sum += (double)G[(int64_t)k * C::PACKED + e];
      acc[i][v] = tile_ok ? (float)sum : 0.0f;
    }
  }
  __syncthreads();  // mwl is visible
  x16r_add_prior<NB>(smem, acc, Lw, ldl, D, prior_kind, wiso, tid, wave, lane);

  if (tid < C::DP) {
    double sum = 0.0;
    for (int k = 0; k < nit; ++k) sum += Bp[(int64_t)k * C::DP + tid];
    bvec[tid] = (float)(sum * (double)wiso);  // b = X (y - X'mw) / sigma^2
  }
  if (tid == 0) {
    double q = 0.0;
    for (int k = 0; k < nit; ++k) q += Qp[k];
    scr[4] = q * (double)wiso;
    scr[5] = (double)N * log((double)s_iso);
    iscr[6] = (s_iso > 0.0f) ? 0x7fffffff : 1;  // (reference :79; also catches NaN)
  }
  x16r_store_packed<NB>(P, acc, wave, lane);
  __syncthreads();
}

template <int NB>
__global__ BLR_X16R_BOUNDS(NB) void ragged_x16_finish_kernel(RaggedX16Args r_kernarg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RaggedX16ArgPtr rp = (RaggedX16ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
  const KernArgPtr<float> ap = (KernArgPtr<float>)rp;
  const __attribute__((address_space(4))) PosteriorArgs<float>& a = *ap;
  for (int i = blockIdx.x; i < rp->nwork; i += gridDim.x) {
    const int reg = rp->order[i];
    if (glue_prior<float, NB>(smem, ap, reg) != 0) continue;           // prior (:78); context from the bases
    phase_sum_parts_x16r<NB>(smem, rp, reg, rp->slot0[i]);             // partials -> P, bvec, scr[4..5]
    if (glue_after_gram<float, NB>(smem, ap, reg) != 0) continue;      // noise check (:79), Lw' (:92)
    const int info = phase_chol<float, NB>(smem, a.D, 1);              // :86
    if (info == 0) phase_backsolve<float, NB>(smem, a.D, a.T_post ? a.T_post + (int64_t)reg * a.strideT : (float*)nullptr, a.ldt);
    ragged_finish<float, NB>(smem, (RaggedArgPtr<float>)ap, reg, info);
  }
}

#endif  // BLR_X16_DECLS_ONLY

// ---- host side of the instantiations (blr_ragged_x16.hip), used by blr_abi.hip ------------------------------------------------------
// fmt: X16_BF16 / X16_F16; NB: 2, 4, 6, 8; which: 0 ragged_x16_kernel, 1 ragged_x16_part_kernel, 2 ragged_x16_finish_kernel (fmt and
// rowvecs ignored).  NULL: this build lacks the instantiation.
const void* ragged_x16_kernel_ptr(int which, int fmt, int NB, bool rowvecs);
size_t ragged_x16_kernel_lds(int which, int NB);
size_t ragged_x16_packed_elems(int NB);  // floats of one slot of partG; partB takes 16 NB doubles a slot
void ragged_x16_kernel_launch(int which, int fmt, int NB, bool rowvecs, unsigned grid, hipStream_t stream, const RaggedX16Args& a);

}  // namespace blr
