// Columns 1 .. S-1 of a batched multi-output posterior on 16-bit features (blr_posterior_multi_batched_x16).
//
// Step 1 is fused_x16_kernel on column 0 (blr_fused_x16.hpp): it leaves the factor T, column 0's mean, evidence and status.  What
// remains per further column s is K17's (blr_multi.hpp):
//   b_s = X (y_s - X'mw) / sigma^2     q_s = |y_s - X'mw|^2 / sigma^2     u_s = T^-T b_s     mw_s = mw + T^-1 u_s
//   logpdf_s = logpdf_0 + (q_0 - |u_0|^2) / 2 - (q_s - |u_s|^2) / 2
//
// multi_cols_x16_kernel<FMT, NB, MODE>: grid (regressors, column passes), 256 threads.  A pass has kMultiColsPerPass column slots, slot 0
// is always column 0.  X streams through K31's ring (four slots, a stage of 32 observations, the same LDS images, the same loaders:
// MODE 2 / 3 whole stages by LDS-DMA, MODE 0 / 1 and the partial last stage through registers); the targets of a stage travel with
// it (one 4-byte LDS-DMA piece per two slots, so that every wait of the loop stays a counted one; through registers where X does).
//   residuals   mu_n by X16Vec's split over the four waves (x16_mean), r_ns = (y_ns - mu_n) / sigma^2 in fp32, q_s in double.  r is split EXACTLY into three bf16 pieces
//               r = h + m + l (each rounded to nearest from the remainder, as marg_planes_x16_kernel) and written in B-fragment order:
//               lane = slot within a 16-column tile, lane group g = the eight observations K31's dealing gives group g of the X
//               fragment, so one ds_read_b128 is a fragment.  The tile of stage t + 1 is produced while stage t is multiplied: one
//               barrier per stage (the wait for a stage is one stage earlier than K31's).
//   product     Bacc[D x slots] += X_stage R_stage on v_mfma_f32_16x16x32_bf16: the A operand is K31's X fragment straight from the
//               ring slot, the B operand the pieces l, m, h in that order into one fp32 accumulator (3 instructions per row block,
//               column tile and stage).  fp16 X: x = hi + lo exactly in two bf16 values (K32's rule), lo x l dropped: 5 instructions.
//               Wave w owns row blocks w and w + 4 and every column tile in use: its accumulators stay in registers.
//   solve       K17's, on the fp32 factor as a packed triangle over the ring: one wave per right-hand side.
// Every sum has a fixed order and every column is computed from its own data only.
#pragma once
#include "blr_common.hpp"
#include "blr_fused_x16.hpp"
#include "blr_multi.hpp"

namespace blr {

struct MultiX16Args {
  const unsigned short* X; int64_t ldx, strideX;  // 16-bit elements
  const float* Y; int64_t ldY, strideY;
  const float* s; int64_t strides;
  const float* mw; int64_t stridemw;
  const float* Tf; int64_t ldt, strideT;  // the factor of every regressor (upper triangle read), as column 0's update wrote it
  const double* lp0;                      // [B] evidence of column 0
  const int32_t* info;                    // [B] status of the shared factorisation
  float* mw_post; int64_t ldmp, stride_mwpost;
  double* logpdf; int64_t stride_lp;
  int D, N, S;
};

// LDS: header (q[64], |u|^2[64] in double, mw[128], the per-wave partial q[4][64]), then stream and solve buffers over each other
constexpr int kMX16Header = 4096;
constexpr int kMX16YPiece = 256 + 32;          // two slots x 32 targets of a stage, padded (eight banks per piece)
constexpr int kMX16YStage = 8 * kMX16YPiece;   // ... per column tile
constexpr int kMX16RTile = 3 * 1024;           // the three pieces of a residual tile
// The targets of stage t are consumed one iteration before its X (the residual tile is made a stage ahead), so three slots carry
// them where X needs four -- and every LDS-DMA destination stays below 64 KiB at NB = 8 with four column tiles (4 + 33 + 27 KiB).
constexpr int kMX16YSlots = 3;
inline size_t multi_x16_lds_bytes(int NB, int D, int nslots) {
  const size_t NT = (size_t)((nslots + 15) / 16), DP = (size_t)16 * NB;
  const size_t stream = (size_t)4 * NB * 1056 + NT * (kMX16YSlots * kMX16YStage + 2 * kMX16RTile);
  const size_t solve = (((size_t)D * (D + 1) / 2 * sizeof(float) + 7) & ~(size_t)7) + (size_t)nslots * DP * sizeof(float);
  return kMX16Header + (stream > solve ? stream : solve);
}

// ---- host side of the instantiations (blr_multi_x16.hip), used by blr_abi.hip ------------------------------------------------------
const void* multi_x16_kernel_ptr(int fmt, int NB, int mode);  // NULL: this build lacks the instantiation
void multi_x16_kernel_launch(int fmt, int NB, int mode, unsigned B, unsigned passes, size_t lds, hipStream_t stream, const MultiX16Args& a);

#ifndef BLR_X16_DECLS_ONLY

// one 4-byte LDS-DMA piece with per-lane global addresses: lane l lands at lds_addr_uniform + 4 l (see glds16_nt)
__device__ __forceinline__ void glds4(uint64_t gaddr, unsigned lds_addr_uniform) {
  unsigned keep, base;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "v_readfirstlane_b32 %1, %2\n\t"
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %3, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep), "=&s"(base)
      : "v"(lds_addr_uniform), "v"(gaddr)
      : "memory");
}

// s_waitcnt vmcnt(n), wave-uniform n <= 20 = two stages of two X pieces and eight target pieces
__device__ __forceinline__ void wait_vm20(int n) {
#define BLR_WVM(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (n) {
    BLR_WVM(1) BLR_WVM(2) BLR_WVM(3) BLR_WVM(4) BLR_WVM(5) BLR_WVM(6) BLR_WVM(7) BLR_WVM(8) BLR_WVM(9) BLR_WVM(10)
    BLR_WVM(11) BLR_WVM(12) BLR_WVM(13) BLR_WVM(14) BLR_WVM(15) BLR_WVM(16) BLR_WVM(17) BLR_WVM(18) BLR_WVM(19) BLR_WVM(20)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
#undef BLR_WVM
}

// X16Vec keeps its mean inside stage() (splitting it there changes fused_x16_kernel's code object): the same reads, the same fp32
// products in the same order and the same reduction over the eight lanes of an observation, on X16Vec's mwf, without the b and q work.
template <bool ROW>
__device__ __forceinline__ int x16_obs(int wave, int lane) {  // the observation (of the stage's 32) whose mean this lane holds
  if constexpr (ROW) return 8 * wave + ((lane & 32) ? 4 : 0) + ((lane & 16) ? 2 : 0) + ((lane & 8) ? 1 : 0);
  else return 8 * wave + (lane >> 3);
}
template <int FMT, int NB, bool ROW>
__device__ __forceinline__ float x16_mean(const X16Vec<NB, ROW>& vec, BLR_LDS char* slot, int wave, int lane) {
  using XC = X16Cfg<NB>;
  constexpr int NF = X16Vec<NB, ROW>::NF;
  float mu;
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
    mu = 0.0f;
#pragma unroll
    for (int f = 0; f < NF; ++f) mu += x[f] * vec.mwf[f];
  } else {
    const int h = lane >> 4;
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
        float x0, x1;
        widen2<FMT>(ok ? (unsigned)v[k] : 0u, x0, x1);
        m[2 * k] += x0 * vec.mwf[f];
        m[2 * k + 1] += x1 * vec.mwf[f];
      }
    }
    // reduce-scatter: bit 5 picks observations 4 .. 7, bit 4 the upper two of those, bit 3 the upper one
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
    float m4[4], m2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) m4[k] = (b5 ? m[4 + k] : m[k]) + __shfl_xor(b5 ? m[k] : m[4 + k], 32, 64);
#pragma unroll
    for (int k = 0; k < 2; ++k) m2[k] = (b4 ? m4[2 + k] : m4[k]) + __shfl_xor(b4 ? m4[k] : m4[2 + k], 16, 64);
    mu = (b3 ? m2[1] : m2[0]) + __shfl_xor(b3 ? m2[0] : m2[1], 8, 64);
  }
  mu += dpp_mov<0xB1>(mu);  // the 8 lanes of an observation: quad_perm[1,0,3,2], quad_perm[2,3,0,1], row_half_mirror
  mu += dpp_mov<0x4E>(mu);
  mu += dpp_mov<0x141>(mu);
  return mu;
}

__device__ __forceinline__ unsigned short bf16_rn_bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }
__device__ __forceinline__ float bf16_bits_f32(unsigned short b) { return __uint_as_float((unsigned)b << 16); }

template <int FMT, int NB, int MODE>
__global__ __launch_bounds__(kThreads, 2) void multi_cols_x16_kernel(MultiX16Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using XC = X16Cfg<NB>;
  using acc4 = Mfma<float>::acc4;
  constexpr bool ROW = (MODE & 1) != 0, FAST = MODE >= 2;
  constexpr int NEW = kMultiColsPerPass - 1, DP = 16 * NB;
  constexpr int OFF_RING = kMX16Header, OFF_Y = OFF_RING + XC::NS * XC::STAGE;
  BLR_LDS char* const lds = (BLR_LDS char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const int64_t reg = blockIdx.x;
  const int pass = blockIdx.y;
  const int D = a.D, N = a.N;
  const int col_first = 1 + pass * NEW;                            // column of slot 1
  const int ncols = min(NEW, a.S - col_first);                     // this pass's own columns (0 only when S == 1)
  const int nslots = ncols + 1, NT = (nslots + 15) / 16;
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  double* const lp_out = a.logpdf ? a.logpdf + reg * a.stride_lp : nullptr;

  if (a.info[reg] != 0) {  // (block-uniform) the shared factorisation failed: NaN evidences, nothing else
    if (lp_out && tid < nslots && (tid > 0 || pass == 0)) lp_out[tid == 0 ? 0 : col_first + tid - 1] = kNaN;
    return;
  }
  if (ncols <= 0) {  // S == 1: the call is column 0's update
    if (lp_out && tid == 0 && pass == 0) lp_out[0] = a.lp0[reg];
    return;
  }

  double* const qS = reinterpret_cast<double*>(smem);
  double* const uuS = qS + kMultiColsPerPass;
  float* const mwS = reinterpret_cast<float*>(smem + 2 * kMultiColsPerPass * sizeof(double));
  double* const qW = reinterpret_cast<double*>(smem + 2048);       // [kWaves][64]
  const int ystage = NT * kMX16YStage, rbuf = NT * kMX16RTile;
  const int OFF_R = OFF_Y + kMX16YSlots * ystage;
  // solve buffers (over the stream's)
  float* const P = reinterpret_cast<float*>(smem + kMX16Header);   // packed factor: row i of L = T' at pidx(i, 0)
  float* const Bs = reinterpret_cast<float*>(smem + kMX16Header + (((size_t)D * (D + 1) / 2 * sizeof(float) + 7) & ~(size_t)7));  // [nslots][DP]

  const BLR_GLOBAL unsigned short* const X = as_global(a.X + reg * a.strideX);
  const BLR_GLOBAL float* const Yg = as_global(a.Y + reg * a.strideY);
  const BLR_GLOBAL float* const mwg = as_global(a.mw + reg * a.stridemw);
  const int64_t ldx = a.ldx, ldY = a.ldY;
  const float wiso = 1.0f / as_global(a.s + reg * a.strides)[0];
  if (tid < 128) mwS[tid] = tid < D ? mwg[tid] : 0.0f;
  __syncthreads();

  X16Vec<NB, ROW> vec;
  vec.init(mwS, lane);
  FragLane<NB, ROW> fl;
  fl.init(lane);

  const int nst = (N + XC::SO - 1) / XC::SO;
  const int nfull = FAST ? N / XC::SO : 0;  // stages 0 .. nfull - 1 travel by LDS-DMA
  // per-lane source of this wave's X pieces (piece p = wave + 4 j), as phase_gram_x16
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
  const int npw = (NB - wave + kWaves - 1) / kWaves;  // X pieces this wave issues per DMA stage (uniform)
  const int pwt = FAST ? npw + 2 * NT : 0;            // ... plus its target pieces (piece k = wave + 4 i holds slots 2 k, 2 k + 1)
  const unsigned lds_base = lds_addr_of(smem);
  const uint64_t zero_addr = (uint64_t)(uintptr_t)g_x16_zero;
  auto col_of = [&](int j) { return j == 0 ? 0 : col_first + j - 1; };
  auto yoff = [](int j, int o) { return (j >> 1) * kMX16YPiece + (j & 1) * 128 + 4 * o; };

  auto issue = [&](int t) {
    const int sl = t & (XC::NS - 1), n0 = t * XC::SO;
    if (FAST && t < nfull) {
      const uint64_t sbase = (uint64_t)(uintptr_t)X + (uint64_t)((ROW ? (int64_t)n0 : (int64_t)n0 * ldx) * 2);
#pragma unroll
      for (int j = 0; j < XC::PW; ++j) {
        const int p = wave + kWaves * j;
        if (p < NB) glds16_nt(pin[j] ? sbase + (uint64_t)poff[j] : zero_addr, lds_base + (unsigned)(OFF_RING + sl * XC::STAGE + p * XC::PIECE));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < 2 * NT) {  // (uniform) a slot outside the pass fetches zeros
          const int k = wave + kWaves * i, j = 2 * k + (lane >> 5);
          const uint64_t src = (uint64_t)(uintptr_t)Yg + (uint64_t)(((int64_t)col_of(j) * ldY + n0 + (lane & 31)) * 4);
          glds4(j < nslots ? src : zero_addr, lds_base + (unsigned)(OFF_Y + (t % kMX16YSlots) * ystage + k * kMX16YPiece));
        }
    } else {
      BLR_LDS char* const ysl = lds + OFF_Y + (t % kMX16YSlots) * ystage;
      x16_stage_regs<NB, ROW>(lds + OFF_RING + sl * XC::STAGE, reinterpret_cast<BLR_LDS float*>(ysl), X, ldx, Yg, D, N, n0, tid);
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < 2 * NT) {
          const int idx = tid + kThreads * e, j = idx >> 5, o = idx & 31;
          const bool ok = j > 0 && j < nslots && n0 + o < N;
          const float y = Yg[ok ? (int64_t)col_of(j) * ldY + n0 + o : 0];
          v[e] = ok ? y : 0.0f;
        }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < 2 * NT) {
          const int idx = tid + kThreads * e, j = idx >> 5, o = idx & 31;
          if (j > 0) *reinterpret_cast<BLR_LDS float*>(ysl + yoff(j, o)) = v[e];  // (slot 0 is x16_stage_regs')
        }
    }
  };

  // this lane's observation of a stage and its place (lane group g, element e) in the fragments
  const int ob = x16_obs<ROW>(wave, lane), c = lane & 7;
  const int og = ROW ? ob >> 3 : (((ob & 1) << 1) | (ob >> 4));
  const int oe = ROW ? ob & 7 : (((ob >> 2) & 3) | (((ob >> 1) & 1) << 2));
  double q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = 0.0;
  // residual tile of stage t -> R buffer t & 1: slots c, c + 8, .. of observation ob
  auto residuals = [&](int t) {
    const int sl = t & (XC::NS - 1);
    const float mu = x16_mean<FMT, NB, ROW>(vec, lds + OFF_RING + sl * XC::STAGE, wave, lane);
    BLR_LDS char* const ysl = lds + OFF_Y + (t % kMX16YSlots) * ystage;
    BLR_LDS char* const rb = lds + OFF_R + (t & 1) * rbuf;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < 2 * NT) {
        const int j = c + 8 * i;
        const float delta = *reinterpret_cast<BLR_LDS float*>(ysl + yoff(j, ob)) - mu;
        const float r = delta * wiso;
        q[i] += (double)delta * (double)r;
        const unsigned short h = bf16_rn_bits(r);
        const float r1 = r - bf16_bits_f32(h);
        const unsigned short m = bf16_rn_bits(r1);
        const unsigned short l = bf16_rn_bits(r1 - bf16_bits_f32(m));
        BLR_LDS char* const at = rb + (i >> 1) * 1024 + (og * 16 + (j & 15)) * 16 + 2 * oe;  // piece p of tile jt at (p NT + jt) KiB
        *reinterpret_cast<BLR_LDS unsigned short*>(at) = l;
        *reinterpret_cast<BLR_LDS unsigned short*>(at + NT * 1024) = m;
        *reinterpret_cast<BLR_LDS unsigned short*>(at + 2 * NT * 1024) = h;
      }
  };

  acc4 acc[2][4];
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[ib][jt] = acc4{0.0f, 0.0f, 0.0f, 0.0f};
  auto product = [&](int t) {
    BLR_LDS char* const slot = lds + OFF_RING + (t & (XC::NS - 1)) * XC::STAGE;
    BLR_LDS char* const rb = lds + OFF_R + (t & 1) * rbuf + lane * 16;
    x16_frag bl[4], bm[4], bh[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
      if (jt < NT) {
        bl[jt] = *reinterpret_cast<BLR_LDS x16_frag*>(rb + jt * 1024);
        bm[jt] = *reinterpret_cast<BLR_LDS x16_frag*>(rb + (NT + jt) * 1024);
        bh[jt] = *reinterpret_cast<BLR_LDS x16_frag*>(rb + (2 * NT + jt) * 1024);
      }
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
      const int I = wave + kWaves * ib;
      if (I < NB) {  // wave-uniform
        x16_frag fa = fl.read(slot, uni(I)), flo;
        if constexpr (FMT == X16_F16) {  // x = hi + lo, two bf16 values
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            float x0, x1;
            widen2<X16_F16>((unsigned)fa[w], x0, x1);
            const unsigned b0 = __float_as_uint(x0), b1 = __float_as_uint(x1);
            const float l0 = x0 - __uint_as_float(b0 & 0xffff0000u), l1 = x1 - __uint_as_float(b1 & 0xffff0000u);
            fa[w] = (int)((b0 >> 16) | (b1 & 0xffff0000u));
            flo[w] = (int)((__float_as_uint(l0) >> 16) | (__float_as_uint(l1) & 0xffff0000u));
          }
        }
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
          if (jt < NT) {  // smallest terms first
            acc4 v = acc[ib][jt];
            if constexpr (FMT == X16_F16) {
              v = mma16<X16_BF16>(flo, bm[jt], v);
              v = mma16<X16_BF16>(fa, bl[jt], v);
              v = mma16<X16_BF16>(flo, bh[jt], v);
            } else {
              v = mma16<X16_BF16>(fa, bl[jt], v);
            }
            v = mma16<X16_BF16>(fa, bm[jt], v);
            acc[ib][jt] = mma16<X16_BF16>(fa, bh[jt], v);
          }
      }
    }
  };

  // a stage is complete for this wave when at most the DMA stages issued after it are outstanding
  auto wait_stage = [&](int need, int issued_last) {
    wait_vm20(max(min(issued_last, nfull - 1) - need, 0) * pwt);
  };
  if (nst > 0) {
    for (int t = 0; t < XC::LA && t < nst; ++t) issue(t);
    wait_stage(0, min(XC::LA, nst) - 1);
    __syncthreads();
    residuals(0);
    for (int t = 0; t < nst; ++t) {
      if (t + 1 < nst) wait_stage(t + 1, min(t + XC::LA - 1, nst - 1));
      __syncthreads();  // stage t + 1 and the residual tile of stage t are visible; the slot of stage t - 1 and the other tile are free
      if (t + XC::LA < nst) issue(t + XC::LA);
      if (t + 1 < nst) residuals(t + 1);
      product(t);
    }
  }
  __syncthreads();  // the ring is dead

  // q_s: the observation lanes of a wave (fixed butterfly), then the waves 0 .. 3
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    double v = q[i];
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 8) qW[wave * kMultiColsPerPass + c + 8 * i] = v;
  }
  // B -> LDS, column by column; the factor -> packed triangle
#pragma unroll
  for (int ib = 0; ib < 2; ++ib) {
    const int I = wave + kWaves * ib;
    if (I < NB) {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = 16 * jt + (lane & 15);
        if (jt < NT && j < nslots) {
#pragma unroll
          for (int v = 0; v < 4; ++v) Bs[j * DP + 16 * I + Mfma<float>::crow(lane, v)] = acc[ib][jt][v];
        }
      }
    }
  }
  {
    const BLR_GLOBAL float* const Tg = as_global(a.Tf + reg * a.strideT);
    for (int cc = wave; cc < D; cc += kWaves)
      for (int r = lane; r <= cc; r += kWave) P[pidx(cc, r)] = Tg[(int64_t)cc * a.ldt + r];
  }
  __syncthreads();
  if (tid < kMultiColsPerPass) qS[tid] = ((qW[tid] + qW[64 + tid]) + qW[128 + tid]) + qW[192 + tid];

  {
    const int i0 = lane, i1 = lane + 64;
    const float r0 = i0 < D ? 1.0f / P[pidx(i0, i0)] : 0.0f;
    const float r1 = i1 < D ? 1.0f / P[pidx(i1, i1)] : 0.0f;
    for (int j = wave; j < nslots; j += kWaves) {
      float b0 = i0 < D ? Bs[j * DP + i0] : 0.0f;
      float b1 = i1 < D ? Bs[j * DP + i1] : 0.0f;
      multi_forward<float>(P, D, lane, r0, r1, b0, b1);
      const double uu = wave_allreduce((double)b0 * (double)b0 + (double)b1 * (double)b1);
      if (lane == 0) uuS[j] = uu;
      if (j > 0 && a.mw_post) {
        multi_backward<float>(P, D, lane, r0, r1, b0, b1);
        BLR_GLOBAL float* const out = as_global(a.mw_post + reg * a.stride_mwpost + (int64_t)(col_first + j - 1) * a.ldmp);
        if (i0 < D) out[i0] = mwS[i0] + b0;  // :68
        if (i1 < D) out[i1] = mwS[i1] + b1;
      }
    }
  }
  __syncthreads();
  if (lp_out && tid < nslots) {
    const double lp0 = a.lp0[reg];
    if (tid == 0) {
      if (pass == 0) lp_out[0] = lp0;
    } else {
      lp_out[col_first + tid - 1] = lp0 + 0.5 * ((qS[0] - uuS[0]) - (qS[tid] - uuS[tid]));
    }
  }
}

#endif  // BLR_X16_DECLS_ONLY

}  // namespace blr
