// Exact leave-one-out on 16-bit features (bf16 / fp16), D <= 128: blr_loo_batched_x16.
//   sigma2_n = |T^-T x_n|^2 (z_n: fp32 accumulation of exact products; its squares summed in double), m_n = x_n'mw' (double), then
//   loo_predictive (blr_loo.hpp) in double at the store.
//
// The planes are K32's (marg_planes_x16_kernel, MargX16Cfg: M = T^-1 split exactly into three bf16 pieces, fragment (J, s) of column block
// J and k-step s <= J / 2, 60 KiB per regressor), and so are the tile, its four loaders (MODE 0 ColVecs / 1 RowVecs by 2-byte loads,
// 2 ColVecs / 3 RowVecs by 16-byte loads), the RowVecs staging through ds_read_b64_tr_b16 and the fp16 split (blr_marg_x16.hpp).  A LOO
// call always has a factor and always needs mean and variance, so this kernel has neither a mean-only nor a diagonal-prior branch.
//
// New here -- the product runs PAIRED: column blocks 2p and 2p + 1 both have p + 1 k-steps and read the same tile fragments fr[0 .. p],
// so they run as two independent accumulator chains whose matrix instructions are issued alternately: no instruction waits for the
// one issued just before it, and a tile fragment is held once for two instructions.  With an odd number of column blocks the last
// pair has one chain.  Within a chain the order is K32's (k ascending; pieces l, m, h; fp16: m.lo, l.hi, h.lo, m.hi, h.hi) and the
// squares are added block by block (in double), so sigma2_n does not depend on the pairing.
// The prefetch of the next tile brings y_n (and s_n under diagonal noise) with it; the lanes that hold m_n and sigma2_n run the
// epilogue in double and store loo_mean / loo_var (fp32) and loo_logpdf (double): nothing N-long but the outputs reaches memory.  The
// epilogue is fenced from the next tile's product (sched_barrier: K12).  Degenerate observations are counted per wave.
#pragma once
#include "blr_common.hpp"
#include "blr_loo.hpp"
#include "blr_marg_x16.hpp"

namespace blr {

struct LooX16Args {
  const unsigned short* X; int64_t ldx, strideX;  // 16-bit elements; ldx and strideX in elements
  const float* mw; int64_t stridemw;              // the state's mean
  LooArgs<float> l;                               // y, s, the three outputs, the counter, info (indexed by the regressor), N
  const void* img;                                // the planes of regressor reg at img + reg * MargX16Cfg::IMG_BYTES
  int D;
  int reg0;  // first regressor of this launch (grid.y is limited to 65535)
};

// ---- host side of the instantiations (blr_loo_x16.hip), used by blr_abi.hip ---------------------------------------------------------
// fmt: BLR_X_BF16 (0) / BLR_X_F16 (1); mode: as marg_x16_launch
const void* loo_x16_kernel_ptr(int fmt, int mode);
void loo_x16_launch(int fmt, int mode, unsigned groups, unsigned nb, size_t lds, hipStream_t stream, const LooX16Args& a);

#ifndef BLR_X16_DECLS_ONLY
// (the operand types and conversions of blr_marg_x16.hpp, restated: that header's kernels may be defined in one unit only)
#define BLR_LX_LDS __attribute__((address_space(3)))

typedef int lx_frag __attribute__((ext_vector_type(4)));  // 8 16-bit values: one MFMA operand
typedef float lx_acc __attribute__((ext_vector_type(4)));

__device__ __forceinline__ lx_acc lx_mma(lx_frag a, lx_frag b, lx_acc c) {
  typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
}
template <int FMT>
__device__ __forceinline__ void lx_widen2(unsigned u, float& lo, float& hi) {
  if constexpr (FMT == 0) {
    lo = __uint_as_float(u << 16);
    hi = __uint_as_float(u & 0xffff0000u);
  } else {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 v = __builtin_bit_cast(h2, u);
    lo = (float)v[0];
    hi = (float)v[1];
  }
}

// One k-step of a pair of column blocks: the planes of fragment f0 (block 2p) and, if TWO, f1 (block 2p + 1) against the same tile
// fragment, the two chains' instructions alternating.  img: the image in LDS at this lane's 16 bytes.
template <int FMT, bool TWO>
__device__ __forceinline__ void lx_pair_step(BLR_LX_LDS char* img, int f0, int f1, lx_frag x, lx_frag xlo, lx_acc& c0, lx_acc& c1) {
  using C = MargX16Cfg;
  BLR_LX_LDS char* const p0 = img + f0 * (C::PLANES * 1024);
  BLR_LX_LDS char* const p1 = img + f1 * (C::PLANES * 1024);
  const lx_frag h0 = *reinterpret_cast<BLR_LX_LDS lx_frag*>(p0);
  const lx_frag m0 = *reinterpret_cast<BLR_LX_LDS lx_frag*>(p0 + 1024);
  const lx_frag l0 = *reinterpret_cast<BLR_LX_LDS lx_frag*>(p0 + 2048);
  lx_frag h1 = h0, m1 = m0, l1 = l0;
  if constexpr (TWO) {
    h1 = *reinterpret_cast<BLR_LX_LDS lx_frag*>(p1);
    m1 = *reinterpret_cast<BLR_LX_LDS lx_frag*>(p1 + 1024);
    l1 = *reinterpret_cast<BLR_LX_LDS lx_frag*>(p1 + 2048);
  }
  if constexpr (FMT == 1) {  // smallest terms first
    c0 = lx_mma(m0, xlo, c0);
    if constexpr (TWO) c1 = lx_mma(m1, xlo, c1);
    c0 = lx_mma(l0, x, c0);
    if constexpr (TWO) c1 = lx_mma(l1, x, c1);
    c0 = lx_mma(h0, xlo, c0);
    if constexpr (TWO) c1 = lx_mma(h1, xlo, c1);
  } else {
    c0 = lx_mma(l0, x, c0);
    if constexpr (TWO) c1 = lx_mma(l1, x, c1);
  }
  c0 = lx_mma(m0, x, c0);
  if constexpr (TWO) c1 = lx_mma(m1, x, c1);
  c0 = lx_mma(h0, x, c0);
  if constexpr (TWO) c1 = lx_mma(h1, x, c1);
}

// ---- the stream -----------------------------------------------------------------------------------------------------------------------
template <int FMT, int MODE>
__global__ __launch_bounds__(kThreads, 2) void loo_x16_kernel(LooX16Args a) {
  using C = MargX16Cfg;
  constexpr bool ROWV = (MODE & 1) != 0, VEC16 = MODE >= 2;
  constexpr int NK = kPB / 32;  // k-steps of 32 features
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(C::OFF_STAGE - C::OFF_MW >= kPB * (int)sizeof(double), "the mean as doubles in front of the staging tiles");
  double* const mwl = reinterpret_cast<double*>(smem + C::OFF_MW);
  BLR_LX_LDS char* const lds = (BLR_LX_LDS char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = a.D, N = a.l.N;
  const int nJ = (D + 15) >> 4, nK = (D + 31) >> 5;
  const int reg = a.reg0 + blockIdx.y;
  if (a.l.info[reg] != 0) return;
  const BLR_GLOBAL unsigned short* X = as_global(a.X + (int64_t)reg * a.strideX);
  const BLR_GLOBAL float* s = as_global(a.l.s + (int64_t)reg * a.l.strides);
  const BLR_GLOBAL float* y = as_global(a.l.y + (int64_t)reg * a.l.stridey);
  const int64_t ldx = a.ldx;
  const bool diag_noise = a.l.noise_kind == NOISE_DIAGONAL;
  const float s_iso = diag_noise ? 0.0f : s[0];
  const int ntiles = (N + 15) >> 4;
  const int t0 = blockIdx.x * kWaves + wave, tstep = gridDim.x * kWaves;
  const int g = lane >> 4, li = lane & 15;
  BLR_LX_LDS char* const stage = lds + C::OFF_STAGE + wave * C::STAGE_WAVE;

  // eight 2-byte loads -> one register-of-eight; idx(e) is the element index of entry e (always inside X), the first cnt entries count
  auto gather8 = [&](auto idx, int cnt) {
    unsigned short v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = X[idx(e)];
    lx_frag f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int keep = min(max(cnt - 2 * w, 0), 2);  // entries of this pair that count
      f[w] = (int)(((unsigned)v[2 * w] | ((unsigned)v[2 * w + 1] << 16)) & (unsigned)((1ull << (16 * keep)) - 1ull));
    }
    return f;
  };
  // ColVecs: dst[u] IS the fragment of k-step u.  RowVecs: dst[u] = eight inputs of feature (lane + 64 u) >> 1, staged through LDS.
  // Inputs >= N re-read input N - 1 (X, y and s alike) and are never stored.
  auto fetch = [&](int tile, lx_frag (&dst)[NK], float& yd, float& sd) {
    const int n0 = tile * 16;
#pragma unroll
    for (int u = 0; u < NK; ++u) {
      dst[u] = lx_frag{0, 0, 0, 0};
      if (u < nK) {  // wave-uniform
        if constexpr (!ROWV) {
          const int64_t row = (int64_t)min(n0 + li, N - 1) * ldx;
          const int d0 = 32 * u + 8 * g;
          if constexpr (VEC16) {  // (D is a multiple of 8: the eight features are inside or outside together)
            const lx_frag v = *reinterpret_cast<const BLR_GLOBAL lx_frag*>(X + row + (d0 < D ? d0 : 0));
            dst[u] = d0 < D ? v : lx_frag{0, 0, 0, 0};
          } else {
            dst[u] = gather8([&](int e) { return row + min(d0 + e, D - 1); }, D - d0);
          }
        } else {
          const int idx = lane + 64 * u, d = idx >> 1, nh = n0 + 8 * (idx & 1);
          const int64_t row = (int64_t)(d < D ? d : 0) * ldx;
          if (VEC16 && n0 + 16 <= N) {  // wave-uniform
            const lx_frag v = *reinterpret_cast<const BLR_GLOBAL lx_frag*>(X + row + nh);
            dst[u] = d < D ? v : lx_frag{0, 0, 0, 0};
          } else {
            const lx_frag v = gather8([&](int e) { return row + min(nh + e, N - 1); }, 8);
            dst[u] = d < D ? v : lx_frag{0, 0, 0, 0};
          }
        }
      }
    }
    const int n = min(n0 + li, N - 1);
    yd = y[n];
    sd = diag_noise ? s[n] : s_iso;
  };

  lx_frag av[NK], an[NK];
  float yv = 0.0f, yn = 0.0f, sv = 0.0f, sn = 0.0f;
  if (t0 < ntiles) fetch(t0, av, yv, sv);
  // once per workgroup: the state's mean and the planes of the column blocks that exist
  {
    const BLR_GLOBAL float* mw = as_global(a.mw + (int64_t)reg * a.stridemw);
    if (tid < kPB) mwl[tid] = tid < D ? (double)mw[tid] : 0.0;
    const BLR_GLOBAL lx_frag* src = reinterpret_cast<const BLR_GLOBAL lx_frag*>(as_global(static_cast<const char*>(a.img) + (int64_t)reg * C::IMG_BYTES));
    BLR_LX_LDS lx_frag* dst = reinterpret_cast<BLR_LX_LDS lx_frag*>(lds + C::off_img(ROWV));
    const int n16 = C::frag0(nJ) * C::PLANES * 64;
    for (int e = tid; e < n16; e += kThreads) dst[e] = src[e];
  }
  __syncthreads();
  BLR_LX_LDS char* const img = lds + C::off_img(ROWV) + 16 * lane;

  int ndeg = 0;
  for (int tile = t0; tile < ntiles; tile += tstep) {
    const bool more = tile + tstep < ntiles;
    if (more) fetch(tile + tstep, an, yn, sn);  // in flight during this tile's product
    // the fragments of this tile: fr[u], lane (li, g) = features 32 u + 8 g .. + 7 of input n0 + li
    lx_frag fr[NK];
    if constexpr (ROWV) {
#pragma unroll
      for (int u = 0; u < NK; ++u)
        if (u < nK) {
          const int b = 16 * lane + 1024 * u;  // feature (lane + 64 u) >> 1, half (lane & 1)
          *reinterpret_cast<BLR_LX_LDS lx_frag*>(stage + (b ^ (((b >> 8) & 1) << 7))) = av[u];
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: LDS runs in order; this keeps the compiler from mixing the two)
#pragma unroll
      for (int u = 0; u < NK; ++u) {
        fr[u] = lx_frag{0, 0, 0, 0};
        if (u < nK) {
          typedef short v4s __attribute__((ext_vector_type(4)));
          typedef short v8s __attribute__((ext_vector_type(8)));
          // source lane i of a 16-lane block addresses feature row i / 4 and the 4-input chunk i % 4 (K31's lane map)
          const int b0 = (32 * u + 8 * g + (li >> 2)) * 32 + 8 * (li & 3), b1 = b0 + 128;
          const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<BLR_LX_LDS v4s*>(stage + (b0 ^ (((b0 >> 8) & 1) << 7))));
          const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<BLR_LX_LDS v4s*>(stage + (b1 ^ (((b1 >> 8) & 1) << 7))));
          const v8s f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          fr[u] = __builtin_bit_cast(lx_frag, f);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the tile has left the staging area before the next one is written
    } else {
#pragma unroll
      for (int u = 0; u < NK; ++u) fr[u] = av[u];
    }

    // m_n = x_n'mw' on the widened registers, accumulated in double: the products are exact, so r_n = y_n - m_n (which the epilogue
    // divides by 1 - h_n) carries no rounding of a D-term sum -- an fp32 sum misses the float32 yardstick where y_n - r_n / (1 - h_n)
    // cancels
    double macc = 0.0;
#pragma unroll
    for (int u = 0; u < NK; ++u)
      if (u < nK) {
        const double* const mwp = mwl + 32 * u + 8 * g;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          float x0, x1;
          lx_widen2<FMT>((unsigned)fr[u][w], x0, x1);
          macc = fma((double)x0, mwp[2 * w], macc);
          macc = fma((double)x1, mwp[2 * w + 1], macc);
        }
      }
    macc += __shfl_xor(macc, 16, 64);
    macc += __shfl_xor(macc, 32, 64);

    // z' = M'x, two column blocks at a time on the bf16 matrix cores; sigma2_n = |z_n|^2
    lx_frag xl[NK];  // fp16: the low pieces (fr becomes the high pieces)
#pragma unroll
    for (int u = 0; u < NK; ++u) xl[u] = lx_frag{0, 0, 0, 0};
    if constexpr (FMT == 1) {
#pragma unroll
      for (int u = 0; u < NK; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          float x0, x1;
          lx_widen2<1>((unsigned)fr[u][w], x0, x1);
          const unsigned b0 = __float_as_uint(x0), b1 = __float_as_uint(x1);
          const float l0 = x0 - __uint_as_float(b0 & 0xffff0000u), l1 = x1 - __uint_as_float(b1 & 0xffff0000u);
          fr[u][w] = (int)((b0 >> 16) | (b1 & 0xffff0000u));
          xl[u][w] = (int)((__float_as_uint(l0) >> 16) | (__float_as_uint(l1) & 0xffff0000u));
        }
    }
    // The squares of the fp32 accumulators are exact in double and are summed there, block by block: sigma2_n reaches the epilogue
    // without the roundings of an fp32 sum and without being rounded to fp32 itself (the epilogue forms s_n - sigma2_n, and
    // loo_mean = y - r / (1 - h) can cancel: one fp32 ulp of sigma2_n is then several ulps of the output -- DESIGN.md K35)
    double sq = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (2 * p < nJ) {  // wave-uniform
        lx_acc c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = {0.0f, 0.0f, 0.0f, 0.0f};
        const int f0 = C::frag0(2 * p), f1 = C::frag0(2 * p + 1);
        const bool two = 2 * p + 1 < nJ;
        if (two) {
#pragma unroll
          for (int k = 0; k <= p; ++k) lx_pair_step<FMT, true>(img, f0 + k, f1 + k, fr[k], xl[k], c0, c1);
        } else {
#pragma unroll
          for (int k = 0; k <= p; ++k) lx_pair_step<FMT, false>(img, f0 + k, f0 + k, fr[k], xl[k], c0, c1);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) sq = fma((double)c0[v], (double)c0[v], sq);
        if (two) {
#pragma unroll
          for (int v = 0; v < 4; ++v) sq = fma((double)c1[v], (double)c1[v], sq);
        }
      }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);

    // the epilogue at the store, in double, fenced from the next tile's product
    __builtin_amdgcn_sched_barrier(0);
    const int n = tile * 16 + li;
    if (g == 0 && n < N && !loo_store<float>(a.l, (int64_t)reg, n, (double)yv, macc, sq, (double)sv)) ++ndeg;
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
#pragma unroll
      for (int u = 0; u < NK; ++u) av[u] = an[u];
      yv = yn;
      sv = sn;
    }
  }
  loo_count(ndeg, a.l.degenerate);
}

#endif  // BLR_X16_DECLS_ONLY

}  // namespace blr
