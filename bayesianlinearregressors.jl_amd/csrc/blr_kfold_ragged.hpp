// Exact leave-fold-out (K-fold) predictives for a batch whose regressors have UNEQUAL observation counts (blr_kfold_ragged_*,
// DESIGN.md K27): the formulas of blr_kfold.hpp on every regressor's own slice of the packed layout (blr_ragged.hpp): regressor b owns
// observations [offsets[b], offsets[b + 1]) of X, y, a diagonal s, kf_mean and kf_var, and the folds [fold_offsets[b],
// fold_offsets[b + 1]) of kf_logpdf.  Fold f of regressor b is [f F, min((f + 1) F, N_b)) of ITS slice.  Per chunk of regressors
// (blr_kfold_ragged_plan.hpp), after the status (loo_ragged_check_kernel) and the images (marg_image_kernel):
//
// kfold_ragged_whiten_kernel<T, LAYOUT>: one workgroup per work item of the K26 table (at most W observations of one regressor, from a
//   multiple of 64 of them).  cov_whiten_kernel's tile walk (blr_cov_batched.hpp) on the regressor's slice: 64 inputs through registers
//   into the rows of an LDS block with the next tile's loads in flight, the image and mw in LDS once per item; z_n = T^-T x_n goes to
//   row offsets[b] - offsets[b0] + n of the chunk's workspace (rows of DP = 16 ceil(D / 16) elements: 16-byte aligned whatever the
//   counts), x_n'mw beside it.  Stores are bounded by N_b: no padding rows between regressors.  X is read once.
// kfold_ragged_kernel<T>: a flat grid, one workgroup per fold pack; the pack's regressor by a binary search in pack_offsets.  The
//   pack's work is kfold_pack (blr_kfold.hpp), the body kfold_kernel runs: the same instructions on the same rows.
// Totals: loo_ragged_total_kernel (blr_marg_ragged.hpp) over fold_offsets.
//
// Bits: a row of Z and its x'mw involve no other row and every tile starts at a multiple of 64 observations of ITS regressor, as in
// cov_whiten_kernel; a pack starts at a multiple of floor(64 / F) F observations of its regressor, as in kfold_kernel, and kfold_pack
// bounds every index to the fold's own rows.  So every output of regressor b has the bits blr_kfold_batched_* with B = 1 gives on
// that slice: they depend neither on B, on the neighbours, on the chunking, on the cut into items nor on the outputs requested.
#pragma once
#include "blr_kfold.hpp"
#include "blr_kfold_ragged_plan.hpp"

namespace blr {

static_assert(kFoldRaggedMaxF == kFoldMax, "the planner's pack size");
static_assert(kRaggedRows == kCovTile, "items start at multiples of the whitening tile");

template <typename T>
struct KfoldRaggedArgs {
  const T* X; int64_t ldx;           // packed inputs
  const T* y;                        // packed targets
  const T* s; int64_t strides; int noise_kind;  // diagonal noise: packed; isotropic: one value per regressor, strides apart
  const T* mw; int64_t stridemw;
  const T* img;                      // images of L^-T, IMG_ELEMS apart, indexed by the global regressor (MargImages::launch)
  const int32_t* info;               // [B] status: a regressor with info != 0 is skipped
  const int64_t* offsets;            // [B + 1], device
  const int64_t* pack_offsets;       // [B + 1], device
  const int64_t* fold_offsets;       // [B + 1], device
  const RaggedItem* items;           // the launch's items, device
  T* Z;                              // the chunk's rows: row offsets[b] - offsets[b0] + n
  T* m;                              // the chunk's x_n'mw, indexed as the rows are
  T* km; T* kv; double* kl;          // packed outputs (may be NULL): km, kv by observations, kl by folds
  unsigned long long* degenerate;
  int D, F;
  int b0, nb;                        // the launch's regressors
};

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void kfold_ragged_whiten_kernel(KfoldRaggedArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Mf = Mfma<T>;
  using G = MargGemmCfg<T>;
  using acc4 = typename Mf::acc4;
  constexpr int TN = kCovTile, VEC = Mf::VEC;
  typedef T vecT __attribute__((ext_vector_type(Mf::VEC)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const RaggedItem it = a.items[blockIdx.x];
  const int reg = it.reg;
  if (a.info[reg] != 0) return;  // (block-uniform) nothing of this regressor is read by the fold kernel
  const int64_t o0 = a.offsets[reg];
  const int N = (int)(a.offsets[reg + 1] - o0);  // the regressor's count: the bound of its last tile
  const int64_t row0 = o0 - a.offsets[a.b0];     // its first row of the chunk's workspace
  const int D = a.D;
  const int NB = (D + 15) / 16, DP = 16 * NB, LDX = cov_ldz<T>(DP);

  T* const Xs = reinterpret_cast<T*>(smem);  // [TN][LDX]
  T* const mws = Xs + TN * LDX;              // [128]
  T* const img = mws + 2 * kCovMaxD;         // [2 NB (NB + 1)][64] (cov_whiten_lds_bytes: the second 128 is a diagonal prior's, unused)

  const BLR_GLOBAL T* const Xg = as_global(a.X + (LAYOUT == LAYOUT_COLVECS ? o0 * a.ldx : o0));
  BLR_GLOBAL T* const Zg = as_global(a.Z + row0 * DP);
  BLR_GLOBAL T* const mg = as_global(a.m + row0);
  // the item's tiles of 64 inputs: it starts at a multiple of 64 observations of the regressor (blr_ragged_items.hpp)
  const int t0 = it.first_tile * kRaggedTile / TN;
  const int tend = (min((it.first_tile + it.ntiles) * kRaggedTile, N) + TN - 1) / TN;

  // ---- the tile through registers, as in cov_whiten_kernel ----
  const int xcnt = DP / 4;
  // RowVecs: element tid + 256 i is input `lane` of feature wave + 4 i, so d < D is the same for the whole wave.  Saying so (wave
  // through v_readfirstlane) leaves one lane mask, n0 + lane < N, for the 32 loads instead of one each: those did not fit the
  // scalar file
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  T xreg[32];
  auto prefetch = [&](int tile) {
    const int n0 = tile * TN;
    if (LAYOUT == LAYOUT_COLVECS) {
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        if (i < xcnt) {
          const int d = (tid & 15) + 16 * (i >> 2), n = (tid >> 4) + 16 * (i & 3);
          const bool ok = d < D && n0 + n < N;  // (never past the regressor's slice)
          xreg[i] = ok ? Xg[(int64_t)d + (int64_t)(n0 + n) * a.ldx] : T(0);
        }
      }
    } else {
      const bool nok = n0 + lane < N;  // (never past the regressor's slice)
      int cnt = (D - wave_u + 3) / 4;  // the features wave + 4 i < D (at most xcnt of them)
      int64_t step = 4 * a.ldx;
      asm volatile("" : "+s"(cnt), "+s"(step));  // (per call: 32 conditions or 32 feature bases kept across the tile loop would not fit the scalar file either)
      int64_t at = (int64_t)wave_u * a.ldx + n0;  // input n0 of feature wave + 4 i
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        xreg[i] = (nok && i < cnt) ? Xg[at + lane] : T(0);
        at += step;
      }
    }
  };
  if (t0 < tend) prefetch(t0);

  // ---- once per item ----
  {
    const BLR_GLOBAL vecT* const src = reinterpret_cast<const BLR_GLOBAL vecT*>(as_global(a.img + (int64_t)reg * G::IMG_ELEMS));
    vecT* const dst = reinterpret_cast<vecT*>(img);
    const int nvec = G::frag0(NB) * 64 / VEC;
    for (int e = tid; e < nvec; e += kThreads) dst[e] = src[e];
  }
  if (tid < kCovMaxD) mws[tid] = tid < D ? as_global(a.mw + (int64_t)reg * a.stridemw)[tid] : T(0);

  const int row = 16 * wave + li;  // this lane's input of the tile (the same in its four lane groups)
  for (int tile = t0; tile < tend; ++tile) {
    const int n0 = tile * TN;
    __syncthreads();  // the previous tile's readers of Xs are done (first tile: nothing pending)
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      if (i < xcnt) {
        const int e = tid + kThreads * i;
        int d, n;
        if (LAYOUT == LAYOUT_COLVECS) { d = (tid & 15) + 16 * (i >> 2); n = (tid >> 4) + 16 * (i & 3); } else { n = e % TN; d = e / TN; }
        Xs[n * LDX + d] = xreg[i];
      }
    }
    __syncthreads();  // (also: image and mw in place)
    if (tile + 1 < tend) prefetch(tile + 1);  // in flight during this tile's products
    const int n = n0 + row;
    const T* const xr = Xs + row * LDX;

    // x_n'mw: cov_whiten_kernel's order (the four lane groups take d = g mod 4, then a fixed two-step butterfly)
    {
      T m = T(0);
      for (int d = g; d < DP; d += 4) m = fused_madd(xr[d], mws[d], m);
      m += __shfl_xor(m, 16, 64);
      m += __shfl_xor(m, 32, 64);
      if (g == 0 && n < N) mg[n] = m;
    }
    // z_n = L^-1 x_n, column block by column block from the image; stored for n < N_b only
    BLR_GLOBAL T* const zr = Zg + (int64_t)n * DP;
#pragma unroll 1
    for (int J = 0; J < NB; ++J) {
      acc4 acc = {T(0), T(0), T(0), T(0)};
      const T* const fb = img + G::frag0(J) * 64 + lane;
#pragma unroll 4
      for (int mm = 0; mm < 4 * (J + 1); ++mm) acc = Mf::mma(fb[mm * 64], xr[G::d_of(mm, g)], acc);
      if (n < N) {
#pragma unroll
        for (int v = 0; v < 4; ++v) zr[16 * J + Mf::crow(lane, v)] = acc[v];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads, 2) void kfold_ragged_kernel(KfoldRaggedArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // the pack's regressor: the last j < nb with pack_offsets[b0 + j] <= this pack (empty regressors own no pack)
  const int64_t* const tbl = a.pack_offsets + a.b0;
  const int64_t pack = tbl[0] + blockIdx.x;
  int lo = 0, hi = a.nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tbl[mid] <= pack) lo = mid; else hi = mid;
  }
  const int64_t reg = (int64_t)a.b0 + lo;
  if (a.info[reg] != 0) return;  // (block-uniform) outputs untouched
  const int64_t o0 = a.offsets[reg];
  const int N = (int)(a.offsets[reg + 1] - o0);
  const int64_t zrow = o0 - a.offsets[a.b0];
  const int PF = (kFoldMax / a.F) * a.F;         // rows of a full pack
  const int row0 = (int)(pack - tbl[lo]) * PF;   // first observation of this pack within the regressor (< N_b)
  const int DP = 16 * ((a.D + 15) / 16);
  KfoldPack<T> p;
  p.Zg = as_global(a.Z + (zrow + row0) * DP);
  p.C = nullptr; p.ldc = 0;
  p.yg = as_global(a.y + o0);
  p.diag = a.noise_kind == NOISE_DIAGONAL;
  p.sg = as_global(p.diag ? a.s + o0 : a.s + reg * a.strides);  // (diagonal noise: the index counts within the slice)
  p.mg = as_global(a.m + zrow);
  p.km = a.km ? a.km + o0 : nullptr;
  p.kv = a.kv ? a.kv + o0 : nullptr;
  p.kl = a.kl ? a.kl + a.fold_offsets[reg] : nullptr;
  p.degenerate = a.degenerate;
  p.D = a.D; p.F = a.F; p.row0 = row0; p.nrows = min(PF, N - row0);  // the regressor's last pack: bounded by N_b
  kfold_pack<T>(smem, p);
}

// the instantiations the library uses, defined in blr_kfold_ragged.hip
#define BLR_KFOLD_RAGGED_INSTANCES(X, T)                                                  \
  X __global__ void kfold_ragged_whiten_kernel<T, LAYOUT_COLVECS>(KfoldRaggedArgs<T>);    \
  X __global__ void kfold_ragged_whiten_kernel<T, LAYOUT_ROWVECS>(KfoldRaggedArgs<T>);    \
  X __global__ void kfold_ragged_kernel<T>(KfoldRaggedArgs<T>);
BLR_KFOLD_RAGGED_INSTANCES(extern template, double)
BLR_KFOLD_RAGGED_INSTANCES(extern template, float)

}  // namespace blr
