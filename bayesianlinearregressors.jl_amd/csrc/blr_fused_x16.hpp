// Fused per-regressor inference on 16-bit features (bf16 / fp16), D <= 128, isotropic noise: blr_posterior_batched_x16.
//
// fused_x16_kernel<FMT, NB, MODE> is fused_small_kernel<float, NB, *> with a new phase 1.  glue_prior, glue_after_gram, phase_chol,
// phase_backsolve and glue_finish are the fp32 route's code on the fp32 route's LDS layout (SmallCfg<float, NB>); phase_gram_x16 leaves
// what phase_gram<float, NB, *> leaves: the packed lower triangle of A = Lw + X X' / sigma^2 in P, b = X (y - X'mw) / sigma^2 in bvec,
// the quadratic form and logdet Sigma_y in scr[4..5], the noise status in iscr[6].
//
// Numerics: X X' runs on v_mfma_f32_16x16x32_bf16 / _f16.  A product of two 16-bit values is exact in fp32 and the accumulation is fp32
// in a fixed order (stage by stage, k inside the instruction), so the Gram matrix is what the fp32 route computes on the widened
// features up to the order of the fp32 additions, and the same bits call to call.  The column-vector work (mean, residual, b, the
// quadratic form) reads the same LDS image, widens in registers and keeps the fp32 route's types: fp32 products, double accumulators,
// the direct residual form.
//
// A stage is 32 observations.  LDS image of a stage, NB pieces of 1 KiB at a pitch of 1056 bytes:
//   ColVecs (MODE 0, 2): the memory image -- observation o at byte o * 2 DP, piece = byte >> 10.  An operand fragment (lane = feature row,
//     8 observations) is two ds_read_b64_tr_b16.  The observations of a stage are dealt to (lane group g, element e) as
//       o = 4 (4 (g & 1) + (e & 3)) + 2 (e >> 2) + (g >> 1)
//     (any bijection is correct, both operands of X X' use the same one): the 32 lanes that one pass of a 64-bit LDS read serves then
//     touch eight different pieces, and the 32 bytes of pitch padding put those on eight different groups of eight banks (NB = 8).
//   RowVecs (MODE 1, 3): fragment order -- piece I holds block row I, 16-byte slot g * 16 + r = feature 16 I + r, observations 8 g .. 8 g + 7,
//     so a fragment is one lane-linear ds_read_b128.
// Loaders: MODE 2 / 3 stream whole stages through LDS-DMA (16 bytes per lane, non-temporal; a lane outside the matrix fetches 16 zero
// bytes, so every piece is issued by all 64 lanes and the counted waits are exact), four slots, three stages in flight; the last,
// partial stage goes through registers.  MODE 0 / 1 load every stage with 2-byte loads through registers (any ldx, any 2-byte base).
#pragma once
#include "blr_common.hpp"
#include "blr_fused_small.hpp"

namespace blr {

enum : int { X16_BF16 = 0, X16_F16 = 1 };

struct X16Args {
  // FIRST member: the glue phases of fused_small_kernel read it through the kernarg pointer (p.X = NULL, p.strideX = 0)
  PosteriorArgs<float> p;
  const unsigned short* X;  // 16-bit elements; p.ldx and strideX in elements
  int64_t strideX;
};
using X16ArgPtr = const __attribute__((address_space(4))) X16Args*;

// (blr_abi.hip defines BLR_X16_DECLS_ONLY: it needs the argument block and the launch interface at the end of this file, no device code)
#ifndef BLR_X16_DECLS_ONLY
#define BLR_LDS __attribute__((address_space(3)))

template <int NB>
struct X16Cfg {
  using C = SmallCfg<float, NB>;
  static_assert(NB % 2 == 0, "even block counts only (the dispatch pads D up)");
  static constexpr int DP = 16 * NB;
  static constexpr int SO = 32;                // observations per stage
  static constexpr int ROWB = 2 * DP;          // bytes of one observation in the ColVecs image
  static constexpr int PIECE = 1024 + 32;      // LDS pitch of a 1 KiB piece
  static constexpr int STAGE = NB * PIECE;     // bytes per ring slot
  static constexpr int NS = 4, LA = 3;         // ring slots, stages in flight
  // the first slots share region 0 of the fp32 layout (free until P is written), the others follow the layout
  static constexpr int NS_IN = C::REGION0 / STAGE < NS ? C::REGION0 / STAGE : NS;
  static constexpr int LDS_BYTES = C::LDS_BYTES + (NS - NS_IN) * STAGE;
  static constexpr int PW = (NB + kWaves - 1) / kWaves;  // pieces per wave per stage (at most)
  static __device__ __forceinline__ int slot_off(int s) { return s < NS_IN ? s * STAGE : C::LDS_BYTES + (s - NS_IN) * STAGE; }
  static __device__ __forceinline__ int pad(int b) { return b + ((b >> 10) << 5); }  // byte of the unpadded image -> LDS byte
};

static __device__ __attribute__((aligned(16), unused)) unsigned g_x16_zero[4];  // what a lane outside the matrix fetches

// one LDS-DMA piece with per-lane global addresses: lane l lands at lds_addr_uniform + 16 l (see glds16 in blr_common.hpp)
__device__ __forceinline__ void glds16_nt(uint64_t gaddr, unsigned lds_addr_uniform) {
  unsigned keep, base;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "v_readfirstlane_b32 %1, %2\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %3, off nt\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep), "=&s"(base)
      : "v"(lds_addr_uniform), "v"(gaddr)
      : "memory");
}

// s_waitcnt vmcnt(n) for a run-time, wave-uniform n (the instruction takes an immediate); n <= 6 = two stages of three pieces
__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

typedef int x16_frag __attribute__((ext_vector_type(4)));  // 8 16-bit values: one MFMA operand
typedef short x16_v4s __attribute__((ext_vector_type(4)));

template <int FMT>
__device__ __forceinline__ void widen2(unsigned u, float& lo, float& hi) {
  if constexpr (FMT == X16_BF16) {
    lo = __uint_as_float(u << 16);
    hi = __uint_as_float(u & 0xffff0000u);
  } else {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 v = __builtin_bit_cast(h2, u);
    lo = (float)v[0];
    hi = (float)v[1];
  }
}

template <int FMT>
__device__ __forceinline__ Mfma<float>::acc4 mma16(x16_frag a, x16_frag b, Mfma<float>::acc4 c) {
  if constexpr (FMT == X16_BF16) {
    typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
  } else {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
  }
}

// per-lane constants of the fragment reads
template <int NB, bool ROW>
struct FragLane {
  int o0, o1;  // ColVecs: byte of (observation of read q, feature 4 (lane & 3)) -- NB == 8: already padded; RowVecs: o0 = 16 lane
  __device__ __forceinline__ void init(int lane) {
    using XC = X16Cfg<NB>;
    if constexpr (ROW) {
      o0 = 16 * lane;
      o1 = 0;
    } else {
      const int g = lane >> 4, j = (lane & 15) >> 2, c4 = lane & 3;
      const int ob = 4 * (4 * (g & 1) + j) + (g >> 1);
      const int b0 = ob * XC::ROWB + 8 * c4, b1 = (ob + 2) * XC::ROWB + 8 * c4;
      o0 = NB == 8 ? XC::pad(b0) : b0;  // (NB == 8: 32 I + 8 c4 < 256, the piece does not depend on the block row)
      o1 = NB == 8 ? XC::pad(b1) : b1;
    }
  }
  __device__ __forceinline__ x16_frag read(BLR_LDS char* slot, int I) const {
    using XC = X16Cfg<NB>;
    if constexpr (ROW) {
      return *reinterpret_cast<BLR_LDS x16_frag*>(slot + I * XC::PIECE + o0);
    } else {
      const int a0 = NB == 8 ? o0 + 32 * I : XC::pad(o0 + 32 * I), a1 = NB == 8 ? o1 + 32 * I : XC::pad(o1 + 32 * I);
      const x16_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<BLR_LDS x16_v4s*>(slot + a0));
      const x16_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<BLR_LDS x16_v4s*>(slot + a1));
      typedef short v8s __attribute__((ext_vector_type(8)));
      const v8s f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      return __builtin_bit_cast(x16_frag, f);
    }
  }
};

// the MFMAs of one stage: one instruction per tile (k = the stage's 32 observations).  WS >= 0 (NB == 8): static wave, the
// fragments of block rows 0 .. 7 - WS in registers; otherwise the two fragments of a tile are picked by LDS address.
template <int FMT, int NB, bool ROW, int WS>
__device__ __forceinline__ void x16_mma_stage(BLR_LDS char* slot, const FragLane<NB, ROW>& fl, AccArr<float, NB>& acc, int wave) {
  using C = SmallCfg<float, NB>;
  if constexpr (NB == 8 && WS >= 0) {
    x16_frag fr[8 - WS];
#pragma unroll
    for (int I = 0; I < 8 - WS; ++I) fr[I] = fl.read(slot, I);
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = mma16<FMT>(fr[(i <= WS) ? WS : 7 - WS], fr[(i <= WS) ? i : i - (WS + 1)], acc[i]);
  } else {
#pragma unroll
    for (int i = 0; i < C::TPW; ++i) {
      int I, K;
      const bool ok = wave_tile(NB, wave, i, I, K);
      if (ok) {  // wave-uniform
        const x16_frag fa = fl.read(slot, uni(I)), fb = fl.read(slot, uni(K));
        acc[i] = mma16<FMT>(fa, fb, acc[i]);
      }
    }
  }
}

// ---- column-vector work of one stage (reference :82, :57): mu_n = x_n'mw, delta_n = y_n - mu_n, b += x_n delta_n / sigma^2,
// q += delta_n^2 / sigma^2, in the types of vector_kstep.  A zero column (beyond N) has y = 0 in ybuf and adds nothing.
// ColVecs: wave w takes observations 8 w .. 8 w + 7; lane = (observation lane >> 3, feature slice c = lane & 7); the lane holds
//   features 32 p + 4 c .. + 3, p < NB / 2, of its observation (NB / 2 reads of 8 bytes, 64 contiguous bytes per 8 lanes).
// RowVecs: wave w takes observation group g = w; lane = (r = lane & 15, h = lane >> 4) holds the 8 observations of features
//   16 (h + 4 j) + r; the eight partial means are reduce-scattered over lane bits 5, 4, 3 and all-reduced over bits 2 .. 0.
template <int NB, bool ROW>
struct X16Vec {
  static constexpr int NF = ROW ? (NB + 3) / 4 : 2 * NB;  // features per lane
  double bacc[NF];
  float mwf[NF];
  double qacc;

  __device__ __forceinline__ int feature(int lane, int f) const {
    if constexpr (ROW) return 16 * ((lane >> 4) + 4 * f) + (lane & 15);
    else return 32 * (f >> 2) + 4 * (lane & 7) + (f & 3);
  }
  __device__ __forceinline__ void init(const float* mwl, int lane) {
    qacc = 0.0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      bacc[f] = 0.0;
      const int d = feature(lane, f);
      mwf[f] = d < 16 * NB ? mwl[d] : 0.0f;
    }
  }

  template <int FMT>
  __device__ __forceinline__ void stage(BLR_LDS char* slot, const BLR_LDS float* yb, float wiso, int wave, int lane) {
    using XC = X16Cfg<NB>;
    if constexpr (!ROW) {
      const int o = 8 * wave + (lane >> 3), c = lane & 7;
      float x[NF];
#pragma unroll
      for (int p = 0; p < NB / 2; ++p) {
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        const u2 v = *reinterpret_cast<BLR_LDS u2*>(slot + XC::pad(o * XC::ROWB + 64 * p + 8 * c));
        widen2<FMT>(v[0], x[4 * p], x[4 * p + 1]);
        widen2<FMT>(v[1], x[4 * p + 2], x[4 * p + 3]);
      }
      float mu = 0.0f;
#pragma unroll
      for (int f = 0; f < NF; ++f) mu += x[f] * mwf[f];
      mu += dpp_mov<0xB1>(mu);   // the 8 lanes of an observation: quad_perm[1,0,3,2], quad_perm[2,3,0,1], row_half_mirror
      mu += dpp_mov<0x4E>(mu);
      mu += dpp_mov<0x141>(mu);
      const float delta = yb[o] - mu;  // :82  y - mean(fx)
      const float rn = delta * wiso;
      if (c == 0) qacc += (double)delta * (double)rn;
#pragma unroll
      for (int f = 0; f < NF; ++f) bacc[f] += (double)x[f] * (double)rn;
    } else {
      const int h = lane >> 4;
      float x[NF][8];
      float m[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) m[k] = 0.0f;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int I = h + 4 * f;
        const bool ok = I < NB;
        const x16_frag v = *reinterpret_cast<BLR_LDS x16_frag*>(slot + (ok ? I : 0) * XC::PIECE + (wave * 16 + (lane & 15)) * 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          widen2<FMT>(ok ? (unsigned)v[k] : 0u, x[f][2 * k], x[f][2 * k + 1]);
          m[2 * k] += x[f][2 * k] * mwf[f];
          m[2 * k + 1] += x[f][2 * k + 1] * mwf[f];
        }
      }
      // reduce-scatter: bit 5 picks observations 4 .. 7, bit 4 the upper two of those, bit 3 the upper one
      const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
      float m4[4], m2[2];
#pragma unroll
      for (int k = 0; k < 4; ++k) m4[k] = (b5 ? m[4 + k] : m[k]) + __shfl_xor(b5 ? m[k] : m[4 + k], 32, 64);
#pragma unroll
      for (int k = 0; k < 2; ++k) m2[k] = (b4 ? m4[2 + k] : m4[k]) + __shfl_xor(b4 ? m4[k] : m4[2 + k], 16, 64);
      float mu = (b3 ? m2[1] : m2[0]) + __shfl_xor(b3 ? m2[0] : m2[1], 8, 64);
      mu += dpp_mov<0xB1>(mu);
      mu += dpp_mov<0x4E>(mu);
      mu += dpp_mov<0x141>(mu);
      const int ko = (b5 ? 4 : 0) + (b4 ? 2 : 0) + (b3 ? 1 : 0);  // this lane's observation of the group
      const float delta = yb[8 * wave + ko] - mu;  // :82  y - mean(fx)
      const float rn = delta * wiso;
      if ((lane & 7) == 0) qacc += (double)delta * (double)rn;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float rk = readlane(rn, ((k >> 2) << 5) | (((k >> 1) & 1) << 4) | ((k & 1) << 3));
#pragma unroll
        for (int f = 0; f < NF; ++f) bacc[f] += (double)x[f][k] * (double)rk;
      }
    }
  }

  // partial sums of b -> red[wave][DP] (doubles)
  __device__ __forceinline__ void flush(double* red, int wave, int lane) {
    if constexpr (!ROW) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        double v = bacc[f];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 8) red[wave * 16 * NB + feature(lane, f)] = v;
      }
    } else {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int d = feature(lane, f);
        if (d < 16 * NB) red[wave * 16 * NB + d] = bacc[f];
      }
    }
  }
};

// ---- a stage through registers: 2-byte loads, zeros outside the matrix, written in the layout's image -----------------------------
template <int NB, bool ROW>
__device__ __forceinline__ void x16_stage_regs(BLR_LDS char* slot, BLR_LDS float* yb, const BLR_GLOBAL unsigned short* X, int64_t ldx,
                                               const BLR_GLOBAL float* y, int D, int N, int n0, int tid) {
  using XC = X16Cfg<NB>;
  constexpr int PER = XC::SO * XC::DP / kThreads;  // 2 NB
  asm volatile("" : "+v"(tid));  // keep the index arithmetic inside the stage loop (see stage_load)
  unsigned short v[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int idx = tid + kThreads * e;
    const int d = ROW ? idx / XC::SO : idx % XC::DP, o = ROW ? idx % XC::SO : idx / XC::DP;
    const bool ok = d < D && n0 + o < N;
    const int64_t addr = ROW ? (int64_t)d * ldx + (n0 + o) : (int64_t)(n0 + o) * ldx + d;
    const unsigned short x = X[ok ? addr : 0];  // unconditional load of a valid address, then select (N > 0 here)
    v[e] = ok ? x : (unsigned short)0;
  }
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int idx = tid + kThreads * e;
    const int d = ROW ? idx / XC::SO : idx % XC::DP, o = ROW ? idx % XC::SO : idx / XC::DP;
    const int off = ROW ? (d >> 4) * XC::PIECE + (((o >> 3) * 16 + (d & 15)) * 16) + 2 * (o & 7) : XC::pad(o * XC::ROWB + 2 * d);
    *reinterpret_cast<BLR_LDS unsigned short*>(slot + off) = v[e];
  }
  if (tid < XC::SO) yb[tid] = n0 + tid < N ? y[n0 + tid] : 0.0f;
}

// =========================================================================================================
// phase 1 on 16-bit features (noinline).  On exit: what phase_gram<float, NB, *> leaves.
// MODE: 0 ColVecs / 1 RowVecs through registers, 2 ColVecs / 3 RowVecs through the LDS-DMA ring
// =========================================================================================================
template <int FMT, int NB, int MODE>
BLR_PHASE void phase_gram_x16(char* smem, X16ArgPtr rp, int reg_in) {
  using C = SmallCfg<float, NB>;
  using XC = X16Cfg<NB>;
  using acc4 = Mfma<float>::acc4;
  constexpr bool ROW = (MODE & 1) != 0, FAST = MODE >= 2;
  BLR_LDS char* const lds = (BLR_LDS char*)smem;
  float* const P = reinterpret_cast<float*>(smem);
  double* const red = reinterpret_cast<double*>(smem);
  BLR_LDS float* const ybuf = reinterpret_cast<BLR_LDS float*>(lds + C::OFF_Y);  // [NS][32]
  float* const bvec = reinterpret_cast<float*>(smem + C::OFF_B);
  float* const mwl = reinterpret_cast<float*>(smem + C::OFF_MW);
  double* const scr = reinterpret_cast<double*>(smem + C::OFF_SCR);
  const RegCtx<float>* ctx = reinterpret_cast<const RegCtx<float>*>(smem + C::OFF_CTX);
  static_assert(XC::NS * XC::SO <= 128, "ybuf holds the y of every ring slot");

  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // nothing derived from tid may be hoisted above this phase
  const int lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int reg = uni(reg_in);
  const BLR_GLOBAL unsigned short* X = as_global(uni(rp->X + (int64_t)reg * rp->strideX));
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
  if (tid < C::DP) mwl[tid] = tid < D ? mw[tid] : 0.0f;
  __syncthreads();  // region 0 is free, mw is visible

  X16Vec<NB, ROW> vec;
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

  // A = Lw + X X' / sigma^2: prior precision in tile layout (phase_gram's load_prior), or the factor's pseudo-observations in fp32
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

  // A: accumulators -> packed lower triangle (the C layout of 16x16x32 is that of 16x16x4_f32)
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
  __syncthreads();
}

// The launch bounds are fused_small_kernel<float, NB, *>'s: the phase functions of this translation unit are compiled for the largest
// budget among their callers here.
template <int FMT, int NB, int MODE>
__global__ __launch_bounds__(kThreads, (NB <= 4 ? 4 : BLR_F32_WAVES_PER_SIMD)) void fused_x16_kernel(X16Args a_kernarg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const X16ArgPtr rp = (X16ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
  static_assert(offsetof(X16Args, p) == 0, "the glue of fused_small_kernel reads PosteriorArgs at the kernarg pointer");
  const KernArgPtr<float> ap = (KernArgPtr<float>)rp;
  const __attribute__((address_space(4))) PosteriorArgs<float>& a = *ap;
  for (int reg = blockIdx.x; reg < a.B; reg += gridDim.x) {
    if (glue_prior<float, NB>(smem, ap, reg) != 0) continue;           // prior (:78), context
    phase_gram_x16<FMT, NB, MODE>(smem, rp, reg);                      // streaming Gram on the 16-bit matrix cores -> P, bvec, scr[4..5]
    if (glue_after_gram<float, NB>(smem, ap, reg) != 0) continue;      // noise check (:79), Lw' (:92)
    const int info = phase_chol<float, NB>(smem, a.D, 1);              // :86
    if (info == 0) phase_backsolve<float, NB>(smem, a.D, a.T_post ? a.T_post + (int64_t)reg * a.strideT : (float*)nullptr, a.ldt);
    glue_finish<float, NB>(smem, ap, reg, info);
  }
}

#endif  // BLR_X16_DECLS_ONLY

// ---- host side of the instantiations (blr_fused_x16.hip), used by blr_abi.hip -------------------------------------------------------
// fmt: X16_BF16 / X16_F16; NB: 2, 4, 6, 8; mode: 0 .. 3.  NULL: this build lacks the instantiation.
const void* x16_kernel_ptr(int fmt, int NB, int mode);
size_t x16_kernel_lds(int NB);
void x16_kernel_launch(int fmt, int NB, int mode, unsigned grid, hipStream_t stream, const X16Args& a);

}  // namespace blr
