// Marginals on 16-bit features (bf16 / fp16), D <= 128: blr_marginals_batched_x16.
//   mean_n = x_n'mw (reference :33), var_n = |L^-1 x_n|^2 + s_n (:40-43), L = U'.
//
// The inputs are exactly 16-bit, so the fp32 triangular inverse M = L^-T (marg_image_kernel<float>, blr_marginals.hpp) is split EXACTLY
// into three bf16 pieces, M = h + m + l (each rounded to nearest from the remainder; bf16 has fp32's exponent range), and z' = M'x runs on
// v_mfma_f32_16x16x32_bf16: every product is exact, the accumulation is fp32 in a fixed order (column block by column block, k-step
// by k-step, pieces l, m, h).  60 matrix instructions per 16 inputs at D = 128 against 144 v_mfma_f32_16x16x4_f32.
//
//   marg_planes_x16_kernel  once per regressor: the three pieces in A-fragment order of the 16x16x32 instruction.  Fragment (J, s) --
//     column block J, k-step s <= J / 2 (the triangle: 1+1+2+2+3+3+4+4 = 20 fragments) -- is 64 lanes x 16 bytes: lane (r = lane & 15,
//     g = lane >> 4) holds M[32 s + 8 g + e][16 J + r], e = 0 .. 7.  Entries with k > column, k >= D or J >= ceil(D / 16) are zeros.
//     The three pieces of a fragment are neighbours: piece p of fragment f at 16-byte slot (3 f + p) 64 + lane; 60 KiB per regressor.
//   marginals_x16_kernel<FMT, MODE>  the stream.  A workgroup copies its regressor's image and mw into LDS once (two workgroups per
//     CU), then each wave walks tiles of 16 inputs with the next tile's loads in flight.  The product is computed transposed (image = A
//     operand, tile = B operand): lane (li, g) holds z[16 J + 4 g + v] of ITS input n0 + li, so the row sum of squares is two
//     cross-lane adds and the stores are one coalesced access of sixteen lanes.
//     A tile is four registers-of-eight per lane: lane (li, g), k-step s holds features 32 s + 8 g .. + 7 of input n0 + li.
//       ColVecs: those are 16 contiguous bytes of X -- MODE 2: one 16-byte load; MODE 0: eight 2-byte loads (any ldx, any base).
//       RowVecs: for a fixed feature the tile's sixteen inputs are 32 contiguous bytes.  Lane l fetches the two 16-byte halves
//         idx = l + 64 u of feature idx >> 1 (MODE 3: one 16-byte load for a whole tile, else as MODE 1: eight 2-byte loads), the wave
//         stages its D x 16 tile in LDS (32 bytes per feature; bit 7 of the byte address flipped for odd 8-row groups, so the 32 lanes
//         of one pass of a 64-bit read touch 32 different banks) and reads the fragment with two ds_read_b64_tr_b16 (lane map: K31).
//     Features >= D are zeros, inputs >= N re-read input N - 1 and are never stored.
//     fp16: x = hi + lo exactly, two bf16 values (the top 8 significand bits; the remaining <= 3), split in registers; lo x l is
//     2^-24 of |x||M| and is dropped: 5 instructions per (J, s).  (An Inf feature splits into hi = Inf, lo = Inf - Inf = NaN; a bf16
//     Inf meets the zero pieces of M: either way that input's var is NaN -- include/blr_mi355x.h, Numerics.)
//     mean: fp32 from the same registers (widened), mw from LDS.  Diagonal prior: var_n = sum x_d^2 / Lw_d + s_n on the vector ALU, no
//     image.  var == NULL: no image either, a pure stream.
#pragma once
#include "blr_common.hpp"
#include "blr_marg_image.hpp"

namespace blr {

struct MargX16Args {
  const unsigned short* X; int64_t ldx, strideX;  // 16-bit elements; ldx and strideX in elements
  const float* s; int64_t strides;
  const float* mw; int64_t stridemw;
  const float* dprior; int64_t stridedp;  // the diagonal of a diagonal prior (else unused)
  float* mean; int64_t stridemean;
  float* var; int64_t stridevar;
  const int32_t* info;  // per-regressor status of a preceding factorisation (may be NULL)
  const void* img;      // the planes of regressor reg at img + reg * IMG_BYTES (NULL: no factor)
  int noise_kind, prior_kind;
  int D, N;
  int reg0;  // first regressor of this launch (grid.y is limited to 65535)
};

struct MargX16Cfg {
  static constexpr int FRAGS = 20, PLANES = 3;
  static constexpr int IMG_BYTES = FRAGS * PLANES * 1024;  // 61440
  // LDS: mw, 1 / Lw (diagonal prior), the waves' RowVecs staging tiles, the image
  static constexpr int OFF_MW = 0, OFF_DI = 512, OFF_STAGE = 1024, STAGE_WAVE = kPB * 32;
  __host__ __device__ static constexpr int off_img(bool rowv) { return OFF_STAGE + (rowv ? kWaves * STAGE_WAVE : 0); }
  __host__ __device__ static constexpr int lds_bytes(bool rowv, bool image) { return off_img(rowv) + (image ? IMG_BYTES : 0); }
  __host__ __device__ static constexpr int frag0(int J) { return ((J + 1) / 2) * ((J + 2) / 2); }  // first fragment of column block J
};
static_assert(MargX16Cfg::frag0(8) == MargX16Cfg::FRAGS, "the triangle's fragments");
static_assert(2 * MargX16Cfg::lds_bytes(true, true) <= 160 * 1024, "two workgroups per CU");

// ---- host side of the instantiations (blr_marg_x16.hip), used by blr_abi.hip --------------------------------------------------------
// fmt: BLR_X_BF16 (0) / BLR_X_F16 (1); mode: 0 ColVecs / 1 RowVecs by 2-byte loads, 2 ColVecs / 3 RowVecs by 16-byte loads
const void* marg_x16_kernel_ptr(int fmt, int mode);
void marg_x16_launch(int fmt, int mode, unsigned groups, unsigned nb, size_t lds, hipStream_t stream, const MargX16Args& a);
// fp32 images (marg_image_kernel<float>) -> planes, regressors reg0 .. reg0 + nb - 1 (both addresses are indexed by the regressor)
void marg_x16_planes_launch(const float* img32, void* img16, const int32_t* info, int D, int reg0, unsigned nb, hipStream_t stream);

#ifndef BLR_X16_DECLS_ONLY
#define BLR_LDS __attribute__((address_space(3)))

typedef int mx_frag __attribute__((ext_vector_type(4)));  // 8 16-bit values: one MFMA operand
typedef float mx_acc __attribute__((ext_vector_type(4)));

__device__ __forceinline__ mx_acc mx_mma(mx_frag a, mx_frag b, mx_acc c) {
  typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
}
__device__ __forceinline__ unsigned mx_pk_bf16(float lo, float hi) {  // v_cvt_pk_bf16_f32: round to nearest even, `lo` to bits 15:0
  typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
  const bf2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}
template <int FMT>
__device__ __forceinline__ void mx_widen2(unsigned u, float& lo, float& hi) {
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

// ---- the planes: x = h + m + l per entry of M, in A-fragment order ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void marg_planes_x16_kernel(const float* __restrict__ img32, uint4* __restrict__ img16,
                                                                   const int32_t* __restrict__ info, int D, int reg0) {
  using G = MargGemmCfg<float>;
  using C = MargX16Cfg;
  const int reg = reg0 + blockIdx.x;
  if (info && info[reg] != 0) return;
  const float* const src = img32 + (int64_t)reg * G::IMG_ELEMS;
  uint4* const dst = img16 + (int64_t)reg * (C::IMG_BYTES / 16);
  const int nJ = (D + 15) >> 4;
  for (int item = threadIdx.x; item < C::FRAGS * 64; item += kThreads) {
    const int f = item >> 6, lane = item & 63, r = lane & 15, g = lane >> 4;
    int J = 0;
    while (C::frag0(J + 1) <= f) ++J;
    const int s = f - C::frag0(J), col = 16 * J + r;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 32 * s + 8 * g + e;
      const bool ok = k <= col && k < D && J < nJ;
      // M[k][col] in the fp32 image: fragment 4 (k / 16) + k % 4 of column block J, lane group (k % 16) / 4 (MargGemmCfg::d_of)
      const float v = src[ok ? (G::frag0(J) + 4 * (k >> 4) + (k & 3)) * 64 + 16 * ((k & 15) >> 2) + r : 0];
      x[e] = ok ? v : 0.0f;
    }
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float a = x[2 * w], b = x[2 * w + 1];
      h[w] = mx_pk_bf16(a, b);
      const float ar = a - __uint_as_float(h[w] << 16), br = b - __uint_as_float(h[w] & 0xffff0000u);
      m[w] = mx_pk_bf16(ar, br);
      const float al = ar - __uint_as_float(m[w] << 16), bl = br - __uint_as_float(m[w] & 0xffff0000u);
      l[w] = mx_pk_bf16(al, bl);
    }
    dst[(3 * f + 0) * 64 + lane] = make_uint4(h[0], h[1], h[2], h[3]);
    dst[(3 * f + 1) * 64 + lane] = make_uint4(m[0], m[1], m[2], m[3]);
    dst[(3 * f + 2) * 64 + lane] = make_uint4(l[0], l[1], l[2], l[3]);
  }
}

// ---- the stream -----------------------------------------------------------------------------------------------------------------------
template <int FMT, int MODE>
__global__ __launch_bounds__(kThreads, 2) void marginals_x16_kernel(MargX16Args a) {
  using C = MargX16Cfg;
  constexpr bool ROWV = (MODE & 1) != 0, VEC16 = MODE >= 2;
  constexpr int NK = kPB / 32;  // k-steps of 32 features
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const mwl = reinterpret_cast<float*>(smem + C::OFF_MW);
  float* const dil = reinterpret_cast<float*>(smem + C::OFF_DI);
  BLR_LDS char* const lds = (BLR_LDS char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = a.D, N = a.N;
  const int nJ = (D + 15) >> 4, nK = (D + 31) >> 5;
  const int reg = a.reg0 + blockIdx.y;
  if (a.info && a.info[reg] != 0) return;
  const BLR_GLOBAL unsigned short* X = as_global(a.X + (int64_t)reg * a.strideX);
  const BLR_GLOBAL float* s = as_global(a.s + (int64_t)reg * a.strides);
  const int64_t ldx = a.ldx;
  const bool want_mean = a.mean != nullptr, want_var = a.var != nullptr;
  const bool diag_prior = a.prior_kind == PRIOR_DIAGONAL;
  const bool use_img = want_var && !diag_prior;
  const bool diag_noise = a.noise_kind == NOISE_DIAGONAL;
  const float s_iso = (want_var && !diag_noise) ? s[0] : 0.0f;
  const int ntiles = (N + 15) >> 4;
  const int t0 = blockIdx.x * kWaves + wave, tstep = gridDim.x * kWaves;
  const int g = lane >> 4, li = lane & 15;
  BLR_LDS char* const stage = lds + C::OFF_STAGE + wave * C::STAGE_WAVE;

  // eight 2-byte loads -> one register-of-eight; idx(e) is the element index of entry e (always inside X), the first cnt entries count.
  // The rest is cleared by a mask computed in vector registers where it is applied: thirty-two lane masks kept in scalar registers
  // across the product would not fit.
  auto gather8 = [&](auto idx, int cnt) {
    unsigned short v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = X[idx(e)];
    mx_frag f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int keep = min(max(cnt - 2 * w, 0), 2);  // entries of this pair that count
      f[w] = (int)(((unsigned)v[2 * w] | ((unsigned)v[2 * w + 1] << 16)) & (unsigned)((1ull << (16 * keep)) - 1ull));
    }
    return f;
  };
  // ColVecs: dst[u] IS the fragment of k-step u.  RowVecs: dst[u] = eight inputs of feature (lane + 64 u) >> 1, staged through LDS.
  auto fetch = [&](int tile, mx_frag (&dst)[NK], float& sd) {
    const int n0 = tile * 16;
#pragma unroll
    for (int u = 0; u < NK; ++u) {
      dst[u] = mx_frag{0, 0, 0, 0};
      if (u < nK) {  // wave-uniform
        if constexpr (!ROWV) {
          const int64_t row = (int64_t)min(n0 + li, N - 1) * ldx;
          const int d0 = 32 * u + 8 * g;
          if constexpr (VEC16) {  // (D is a multiple of 8: the eight features are inside or outside together)
            const mx_frag v = *reinterpret_cast<const BLR_GLOBAL mx_frag*>(X + row + (d0 < D ? d0 : 0));
            dst[u] = d0 < D ? v : mx_frag{0, 0, 0, 0};
          } else {
            dst[u] = gather8([&](int e) { return row + min(d0 + e, D - 1); }, D - d0);
          }
        } else {
          const int idx = lane + 64 * u, d = idx >> 1, nh = n0 + 8 * (idx & 1);
          const int64_t row = (int64_t)(d < D ? d : 0) * ldx;
          if (VEC16 && n0 + 16 <= N) {  // wave-uniform
            const mx_frag v = *reinterpret_cast<const BLR_GLOBAL mx_frag*>(X + row + nh);
            dst[u] = d < D ? v : mx_frag{0, 0, 0, 0};
          } else {
            const mx_frag v = gather8([&](int e) { return row + min(nh + e, N - 1); }, 8);
            dst[u] = d < D ? v : mx_frag{0, 0, 0, 0};
          }
        }
      }
    }
    sd = (diag_noise && want_var) ? s[min(n0 + li, N - 1)] : s_iso;
  };

  mx_frag av[NK], an[NK];
  float sv = 0.0f, sn = 0.0f;
  if (t0 < ntiles) fetch(t0, av, sv);
  // once per workgroup: the prior mean, the reciprocal diagonal, the image
  {
    const BLR_GLOBAL float* mw = as_global(a.mw + (int64_t)reg * a.stridemw);
    if (tid < kPB) {
      mwl[tid] = tid < D ? mw[tid] : 0.0f;
      float di = 0.0f;
      if (want_var && diag_prior && tid < D) di = 1.0f / as_global(a.dprior + (int64_t)reg * a.stridedp)[tid];
      dil[tid] = di;
    }
    if (use_img) {
      const BLR_GLOBAL mx_frag* src = reinterpret_cast<const BLR_GLOBAL mx_frag*>(as_global(static_cast<const char*>(a.img) + (int64_t)reg * C::IMG_BYTES));
      BLR_LDS mx_frag* dst = reinterpret_cast<BLR_LDS mx_frag*>(lds + C::off_img(ROWV));
      const int n16 = C::frag0(nJ) * C::PLANES * 64;  // the column blocks that exist
      for (int e = tid; e < n16; e += kThreads) dst[e] = src[e];
    }
  }
  __syncthreads();
  BLR_LDS char* const img = lds + C::off_img(ROWV) + 16 * lane;

  for (int tile = t0; tile < ntiles; tile += tstep) {
    const bool more = tile + tstep < ntiles;
    if (more) fetch(tile + tstep, an, sn);  // in flight during this tile's product
    // the fragments of this tile: fr[u], lane (li, g) = features 32 u + 8 g .. + 7 of input n0 + li
    mx_frag fr[NK];
    if constexpr (ROWV) {
#pragma unroll
      for (int u = 0; u < NK; ++u)
        if (u < nK) {
          const int b = 16 * lane + 1024 * u;  // feature (lane + 64 u) >> 1, half (lane & 1)
          *reinterpret_cast<BLR_LDS mx_frag*>(stage + (b ^ (((b >> 8) & 1) << 7))) = av[u];
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: LDS runs in order; this keeps the compiler from mixing the two)
#pragma unroll
      for (int u = 0; u < NK; ++u) {
        fr[u] = mx_frag{0, 0, 0, 0};
        if (u < nK) {
          typedef short v4s __attribute__((ext_vector_type(4)));
          typedef short v8s __attribute__((ext_vector_type(8)));
          // source lane i of a 16-lane block addresses feature row i / 4 and the 4-input chunk i % 4 (K31's lane map)
          const int b0 = (32 * u + 8 * g + (li >> 2)) * 32 + 8 * (li & 3), b1 = b0 + 128;
          const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<BLR_LDS v4s*>(stage + (b0 ^ (((b0 >> 8) & 1) << 7))));
          const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<BLR_LDS v4s*>(stage + (b1 ^ (((b1 >> 8) & 1) << 7))));
          const v8s f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          fr[u] = __builtin_bit_cast(mx_frag, f);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the tile has left the staging area before the next one is written
    } else {
#pragma unroll
      for (int u = 0; u < NK; ++u) fr[u] = av[u];
    }

    // vector-ALU work on the widened registers: mean_n = x_n'mw (:33); diagonal prior: sum x_d^2 / Lw_d
    float macc = 0.0f, sq = 0.0f;
    if (want_mean || (want_var && diag_prior)) {
#pragma unroll
      for (int u = 0; u < NK; ++u)
        if (u < nK) {
          const float* const mwp = mwl + 32 * u + 8 * g;
          const float* const dip = dil + 32 * u + 8 * g;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            float x0, x1;
            mx_widen2<FMT>((unsigned)fr[u][w], x0, x1);
            macc += x0 * mwp[2 * w];
            macc += x1 * mwp[2 * w + 1];
            if (diag_prior) {  // (uniform; dil is all zeros for a mean-only call)
              sq += x0 * x0 * dip[2 * w];
              sq += x1 * x1 * dip[2 * w + 1];
            }
          }
        }
      macc += __shfl_xor(macc, 16, 64);
      macc += __shfl_xor(macc, 32, 64);
    }
    // z' = M'x column block by column block on the bf16 matrix cores; var_n = |z_n|^2
    if (use_img) {
      mx_frag xl[NK];  // fp16: the low pieces (fr becomes the high pieces)
      if constexpr (FMT == 1) {
#pragma unroll
        for (int u = 0; u < NK; ++u)
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            float x0, x1;
            mx_widen2<1>((unsigned)fr[u][w], x0, x1);
            const unsigned b0 = __float_as_uint(x0), b1 = __float_as_uint(x1);
            const float l0 = x0 - __uint_as_float(b0 & 0xffff0000u), l1 = x1 - __uint_as_float(b1 & 0xffff0000u);
            fr[u][w] = (int)((b0 >> 16) | (b1 & 0xffff0000u));
            xl[u][w] = (int)((__float_as_uint(l0) >> 16) | (__float_as_uint(l1) & 0xffff0000u));
          }
      }
#pragma unroll
      for (int J = 0; J < 8; ++J)
        if (J < nJ) {  // wave-uniform
          mx_acc acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int k = 0; k <= J / 2; ++k) {
            BLR_LDS char* const fp = img + (C::frag0(J) + k) * (C::PLANES * 1024);
            const mx_frag mh = *reinterpret_cast<BLR_LDS mx_frag*>(fp);
            const mx_frag mm = *reinterpret_cast<BLR_LDS mx_frag*>(fp + 1024);
            const mx_frag ml = *reinterpret_cast<BLR_LDS mx_frag*>(fp + 2048);
            if constexpr (FMT == 1) {  // smallest terms first
              acc = mx_mma(mm, xl[k], acc);
              acc = mx_mma(ml, fr[k], acc);
              acc = mx_mma(mh, xl[k], acc);
            } else {
              acc = mx_mma(ml, fr[k], acc);
            }
            acc = mx_mma(mm, fr[k], acc);
            acc = mx_mma(mh, fr[k], acc);
          }
#pragma unroll
          for (int v = 0; v < 4; ++v) sq += acc[v] * acc[v];
        }
    }
    if (want_var) {
      sq += __shfl_xor(sq, 16, 64);
      sq += __shfl_xor(sq, 32, 64);
    }
    const int n = tile * 16 + li;
    if (g == 0 && n < N) {
      if (want_mean) a.mean[(int64_t)reg * a.stridemean + n] = macc;
      if (want_var) a.var[(int64_t)reg * a.stridevar + n] = sq + sv;
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < NK; ++u) av[u] = an[u];
      sv = sn;
    }
  }
}

#endif  // BLR_X16_DECLS_ONLY

}  // namespace blr
