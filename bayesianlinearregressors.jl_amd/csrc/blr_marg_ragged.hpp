// Marginals and exact leave-one-out for a batch whose regressors have UNEQUAL observation counts (blr_marginals_ragged_*,
// blr_loo_ragged_*): reference src/bayesian_linear_regression.jl:33 (mean), :40-43 (var), :47 (both) and the
// leave-one-out closed form of blr_loo.hpp, under a map over fxs of different lengths.  The packed layout is K14's
// (blr_ragged.hpp): regressor b owns observations [offsets[b], offsets[b+1]) of X, y, a diagonal s -- and of every per-observation
// output.
//
// Once a regressor's triangular inverse exists its observations are independent, so the unit of work is not the regressor but an
// ITEM of the host's table (blr_ragged_items.hpp): at most W observations of one regressor.  One workgroup per item, on grid.x:
//   marg_ragged_gemm_kernel<T, ROWV, LOO>   D = 128 with a factor; ColVecs with 16-byte aligned X and ldx, or RowVecs.  The body is
//       marginals_gemm_kernel's product stream (blr_marginals.hpp): the regressor's image and mw in LDS (two workgroups per CU),
//       a wave per 16-input tile with the next tile's loads in flight; the tiles are the item's, the bound of the last one is N_b.
//       A mean-only call of such a shape runs here too, without image and product: its mean then has the bits the same call gives
//       with the variance requested.
//   marg_ragged_rows_kernel<T, LOO>         every other D <= 128 shape (any D, unaligned ColVecs, diagonal priors and their mean-only calls): the
//       sweep of marginals_mfma_kernel (blr_large.hpp) over LDS-resident tiles of 64 inputs as rows.  The sweep, not the image
//       product at one column: it takes L = U' straight from the caller's factor (no image launch at all on this route), serves
//       diagonal priors and mean-only calls from the same tile loop, and is the code whose accuracy the equal-count tests of
//       every D < 128 already pin.
// Under LOO both fetch y_n with the tile and run the double-precision epilogue of blr_loo.hpp (loo_store, loo_count) at the store:
// no workspace of means and variances, no loo_finish_kernel.
//
// Bits: a tile always starts at a multiple of 64 (rows kernel) / 16 (gemm kernel) observations of its regressor whatever the item
// size, a row's arithmetic involves no other row, and which wave or workgroup takes a tile changes nothing it computes -- so the
// bits of observation n of regressor b depend on that regressor's slice and state alone: not on B, the neighbours, the chunking
// or the cut into items.
#pragma once
#include "blr_marginals.hpp"
#include "blr_ragged_items.hpp"

namespace blr {

static_assert(kRaggedImageElems == MargGemmCfg<double>::IMG_ELEMS && kRaggedImageElems == MargGemmCfg<float>::IMG_ELEMS, "the planner's image size");
static_assert(kRaggedRows == TrsmCfg<double>::RB && kRaggedRows == TrsmCfg<float>::RB && kRaggedRows % kRaggedTile == 0, "the planner's tile sizes");

template <typename T>
struct MargRaggedArgs {
  const T* X; int64_t ldx;        // packed inputs
  const T* y;                     // packed targets (LOO)
  const T* s; int64_t strides;    // diagonal noise: packed; isotropic: one value per regressor, strides apart
  const T* mw; int64_t stridemw;
  const T* U; int64_t ldu, strideU;  // rows kernel: the upper factor, or the diagonal of the precision (ldu unused)
  T* mean; T* var;                // marginals: packed outputs (may be NULL)
  T* lm; T* lv; double* ll;       // LOO: packed outputs (may be NULL)
  unsigned long long* degenerate;  // LOO: counter of degenerate leverages
  const int32_t* info;            // per-regressor status (may be NULL): a regressor with info != 0 is skipped
  const int64_t* offsets;         // [B + 1], device
  const RaggedItem* items;        // the launch's items, device
  int layout, noise_kind, prior_kind, D;
};

// the LOO outputs of one regressor's slice, in the form loo_store takes (regressor 0, no strides)
template <typename T>
__device__ __forceinline__ LooArgs<T> ragged_loo_slice(const MargRaggedArgs<T>& a, int64_t o0) {
  LooArgs<T> l{};
  l.lm = a.lm ? a.lm + o0 : nullptr;
  l.lv = a.lv ? a.lv + o0 : nullptr;
  l.ll = a.ll ? a.ll + o0 : nullptr;
  return l;
}

// ---- D = 128, factor: the product stream over an item's tiles ---------------------------------------------------------------------
template <typename T, bool ROWV, bool LOO>
__global__ __launch_bounds__(kThreads, 2) void marg_ragged_gemm_kernel(MargRaggedArgs<T> a, const T* __restrict__ img_all) {
  using G = MargGemmCfg<T>;
  using acc4 = typename Mfma<T>::acc4;
  constexpr int VEC = G::VEC, NL = G::NLOAD;
  typedef T vecT __attribute__((ext_vector_type(Mfma<T>::VEC)));
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* const img = reinterpret_cast<T*>(smem);
  T* const mwl = reinterpret_cast<T*>(smem + G::OFF_MW);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const RaggedItem it = a.items[blockIdx.x];
  const int reg = it.reg;
  if (a.info && a.info[reg] != 0) return;
  const int64_t o0 = a.offsets[reg];
  const int N = (int)(a.offsets[reg + 1] - o0);  // the regressor's count: the bound of its last tile
  const bool diag_noise = a.noise_kind == NOISE_DIAGONAL;
  const BLR_GLOBAL T* X = as_global(a.X + (ROWV ? o0 : o0 * a.ldx));
  const BLR_GLOBAL T* s = as_global(diag_noise ? a.s + o0 : a.s + (int64_t)reg * a.strides);
  const BLR_GLOBAL T* mw = as_global(a.mw + (int64_t)reg * a.stridemw);
  const int tend = min(it.first_tile + it.ntiles, (N + 15) >> 4);
  const int t0 = it.first_tile + wave;
  const int g = lane >> 4, li = lane & 15;
  // this lane's slice of a tile: input n0 + li, entries d = 4 VEC m' + VEC g .. + VEC of it, m' = 0 .. NL - 1
  vecT av[NL], an[NL];
  const bool want_var = LOO || a.var;
  const T s_iso = (diag_noise || !want_var) ? T(0) : s[0];
  T sv = T(0), sn = T(0);
  T yv = T(0), yn = T(0);
  const BLR_GLOBAL T* yg = nullptr;
  if constexpr (LOO) yg = as_global(a.y + o0);
  auto fetch = [&](int tile, vecT (&dst)[NL], T& sd, T& yd) {
    const int n = min(tile * 16 + li, N - 1);  // (inputs past the regressor's end re-read ITS last one; never stored)
    if constexpr (ROWV) {
      const BLR_GLOBAL T* p = X + n + (int64_t)(VEC * g) * a.ldx;
#pragma unroll
      for (int u = 0; u < NL; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) dst[u][e] = p[(int64_t)(4 * VEC * u + e) * a.ldx];
    } else {
      const BLR_GLOBAL vecT* p = reinterpret_cast<const BLR_GLOBAL vecT*>(X + (int64_t)n * a.ldx + VEC * g);
#pragma unroll
      for (int u = 0; u < NL; ++u) dst[u] = p[4 * u];  // (4 VEC elements = 4 vectors apart)
    }
    sd = (diag_noise && want_var) ? s[n] : s_iso;
    if constexpr (LOO) yd = yg[n];
  };
  if (t0 < tend) fetch(t0, av, sv, yv);
  // the regressor's image and prior mean: once per item
  {
    const BLR_GLOBAL vecT* src = reinterpret_cast<const BLR_GLOBAL vecT*>(as_global(img_all + (int64_t)reg * G::IMG_ELEMS));
    vecT* dst = reinterpret_cast<vecT*>(img);
    for (int e = tid; want_var && e < G::IMG_ELEMS / VEC; e += kThreads) dst[e] = src[e];  // (a mean-only call has no image)
    if (tid < kPB) mwl[tid] = mw[tid];
  }
  __syncthreads();
  LooArgs<T> l{};
  if constexpr (LOO) l = ragged_loo_slice(a, o0);
  T* const mean_out = a.mean ? a.mean + o0 : nullptr;
  T* const var_out = a.var ? a.var + o0 : nullptr;
  int ndeg = 0;  // (LOO: degenerate leverages this lane stored)
  for (int tile = t0; tile < tend; tile += kWaves) {
    const bool more = tile + kWaves < tend;
    if (more) fetch(tile + kWaves, an, sn, yn);  // in flight during this tile's 144 MFMAs
    T macc = T(0);
    if (LOO || a.mean) {  // mean_n = x_n'mw (:33)
#pragma unroll
      for (int u = 0; u < NL; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) macc += av[u][e] * mwl[4 * VEC * u + VEC * g + e];
      macc += __shfl_xor(macc, 16, 64);
      macc += __shfl_xor(macc, 32, 64);
    }
    T sq = T(0);
    if (want_var) {  // z = x'M column block by column block; |z_n|^2 (:41-43)
#pragma unroll
      for (int J = 0; J < 8; ++J) {
        acc4 acc = {T(0), T(0), T(0), T(0)};
        const T* fb = img + G::frag0(J) * 64 + lane;
#pragma unroll
        for (int m = 0; m < 4 * (J + 1); ++m) acc = Mfma<T>::mma(fb[m * 64], av[m / VEC][m % VEC], acc);
#pragma unroll
        for (int v = 0; v < 4; ++v) sq += acc[v] * acc[v];
      }
      sq += __shfl_xor(sq, 16, 64);
      sq += __shfl_xor(sq, 32, 64);
    }
    const int n0 = tile * 16;
    if (g == 0 && n0 + li < N) {
      if constexpr (LOO) {
        // (fenced, as in marginals_gemm_kernel: the epilogue's double log and divisions stay out of the next tile's product)
        __builtin_amdgcn_sched_barrier(0);
        if (!loo_store(l, 0, n0 + li, (double)yv, (double)macc, (double)sq, (double)sv)) ++ndeg;
        __builtin_amdgcn_sched_barrier(0);
      } else {
        if (mean_out) mean_out[n0 + li] = macc;
        if (var_out) var_out[n0 + li] = sq + sv;
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < NL; ++u) av[u] = an[u];
      sv = sn;
      if constexpr (LOO) yv = yn;
    }
  }
  if constexpr (LOO) loo_count(ndeg, a.degenerate);
}

// ---- every other D <= 128 shape: the sweep over LDS-resident tiles of 64 inputs as rows -------------------------------------------------
// LDS with a factor: [P | Xs | dinv | Linv | mw]; mean-only / diagonal prior: [Xs | dinv | mw] (marginals_mfma_kernel's two images)
template <typename T>
struct MargRaggedRowsCfg {
  using Cfg = TrsmCfg<T>;
  static constexpr int XS_BYTES = (Cfg::RB * Cfg::LDX * (int)sizeof(T) + 15) & ~15;
  static constexpr int LDS_FACTOR = Cfg::LDS_BYTES + kPB * (int)sizeof(T);
  static constexpr int LDS_STREAM = XS_BYTES + 2 * kPB * (int)sizeof(T) + 16;
};

template <typename T, bool LOO>
__global__ __launch_bounds__(kThreads) void marg_ragged_rows_kernel(MargRaggedArgs<T> a) {
  using Cfg = TrsmCfg<T>;
  using RC = MargRaggedRowsCfg<T>;
  constexpr int VEC = Mfma<T>::VEC;
  typedef T vecT __attribute__((ext_vector_type(Mfma<T>::VEC)));
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool want_var = LOO || a.var != nullptr;
  const bool use_factor = want_var && a.prior_kind == PRIOR_UPPER_FACTOR;
  const bool diag_prior = want_var && a.prior_kind == PRIOR_DIAGONAL;
  T* const P = reinterpret_cast<T*>(smem);
  T* const Xs = reinterpret_cast<T*>(smem + (use_factor ? Cfg::OFF_X : 0));
  T* const dinv = reinterpret_cast<T*>(smem + (use_factor ? Cfg::OFF_DI : RC::XS_BYTES));
  T* const Linv = reinterpret_cast<T*>(smem + Cfg::OFF_LI);
  T* const mwl = reinterpret_cast<T*>(smem + (use_factor ? Cfg::LDS_BYTES : RC::XS_BYTES + kPB * (int)sizeof(T)));  // [128]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uni(tid >> 6);
  const RaggedItem it = a.items[blockIdx.x];
  const int reg = it.reg;
  if (a.info && a.info[reg] != 0) return;
  const int D = a.D;
  const int64_t o0 = a.offsets[reg];
  const int N = (int)(a.offsets[reg + 1] - o0);
  const bool diag_noise = a.noise_kind == NOISE_DIAGONAL;
  const bool colv = a.layout == LAYOUT_COLVECS;
  const T* X = a.X + (colv ? o0 * a.ldx : o0);
  const T* U = a.U + (int64_t)reg * a.strideU;
  const T* s = diag_noise ? a.s + o0 : a.s + (int64_t)reg * a.strides;
  const T* mw = a.mw + (int64_t)reg * a.stridemw;
  const int nchunks = (D + 15) >> 4, DPc = nchunks * 16;
  // the item's rows [r_begin, r_end) of the regressor, in tiles of RB that start at multiples of RB (the planner's W is one)
  const int r_begin = it.first_tile * kRaggedTile;
  const int r_end = min((it.first_tile + it.ntiles) * kRaggedTile, N);

  // ---- the first tile's inputs go in flight before anything else (vector path: ColVecs, whole 16-byte vectors)
  const bool vec = colv && D == kPB && (a.ldx % VEC) == 0 && ((uintptr_t)X % 16) == 0;
  constexpr int VPR = kPB / VEC;                           // vectors per input (row of Xs)
  constexpr int NVT = Cfg::RB * kPB / (VEC * kThreads);    // vectors per thread per tile
  vecT pre[NVT];
  auto prefetch = [&](int n0) {
#pragma unroll
    for (int u = 0; u < NVT; ++u) {
      const int vi = u * kThreads + tid;
      const int r = vi / VPR, c0 = (vi % VPR) * VEC;
      pre[u] = (n0 + r < r_end) ? *reinterpret_cast<const vecT*>(X + (int64_t)(n0 + r) * a.ldx + c0) : vecT(T(0));
    }
  };
  if (vec && r_begin < r_end) prefetch(r_begin);

  // ---- once per item: L = U' packed (padding: unit diagonal), reciprocal pivots, inverse blocks, mw
  const bool uvec = use_factor && D == kPB && (a.ldu % VEC) == 0 && ((uintptr_t)U % 16) == 0;
  if (uvec) load_upper_block_to_packed(P, U, a.ldu, tid);
#pragma unroll 1
  for (int base = 0; use_factor && !uvec && base < DPc * DPc; base += kThreads * 8) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * kThreads + tid;
      const int r = idx / DPc, c = idx % DPc;  // L[r][c] = U[c, r]: consecutive threads -> consecutive c
      const bool ok = idx < DPc * DPc && c <= r && r < D;
      v[u] = U[ok ? (int64_t)r * a.ldu + c : 0];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * kThreads + tid;
      const int r = idx / DPc, c = idx % DPc;
      if (idx < DPc * DPc && c <= r) P[pidx(r, c)] = (r < D) ? v[u] : (r == c ? T(1) : T(0));
    }
  }
  if (tid < kPB) mwl[tid] = (tid < D) ? mw[tid] : T(0);
  __syncthreads();
  if (use_factor && tid < DPc) dinv[tid] = T(1) / P[pidx(tid, tid)];
  if (diag_prior && tid < kPB) dinv[tid] = (tid < D) ? T(1) / U[tid] : T(0);  // U = the diagonal of the precision
  __syncthreads();
  if (use_factor) trsm_prepare<T>(P, dinv, Linv, nchunks, tid);

  LooArgs<T> l{};
  if constexpr (LOO) l = ragged_loo_slice(a, o0);
  T* const mean_out = a.mean ? a.mean + o0 : nullptr;
  T* const var_out = a.var ? a.var + o0 : nullptr;
  int ndeg = 0;
  for (int n0 = r_begin; n0 < r_end; n0 += Cfg::RB) {
    const int nt = min(Cfg::RB, r_end - n0);
    __syncthreads();  // the previous tile's readers of Xs are done
    if (vec) {
#pragma unroll
      for (int u = 0; u < NVT; ++u) {
        const int vi = u * kThreads + tid;
        const int r = vi / VPR, c0 = (vi % VPR) * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) Xs[r * Cfg::LDX + c0 + e] = pre[u][e];
      }
      if (n0 + Cfg::RB < r_end) prefetch(n0 + Cfg::RB);  // in flight during this tile's sweep
    } else {
#pragma unroll 1
      for (int base = 0; base < Cfg::RB * DPc; base += kThreads * 8) {
        T v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = base + u * kThreads + tid;
          int r, c;
          if (colv) { c = idx % DPc; r = idx / DPc; }
          else      { r = idx % Cfg::RB; c = idx / Cfg::RB; }
          const bool ok = idx < Cfg::RB * DPc && r < nt && c < D;  // (never past the regressor's slice)
          const int64_t addr = colv ? (int64_t)(n0 + r) * a.ldx + c : (int64_t)c * a.ldx + n0 + r;
          v[u] = X[ok ? addr : 0];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = base + u * kThreads + tid;
          int r, c;
          if (colv) { c = idx % DPc; r = idx / DPc; }
          else      { r = idx % Cfg::RB; c = idx / Cfg::RB; }
          if (idx < Cfg::RB * DPc) Xs[r * Cfg::LDX + c] = (r < nt && c < D) ? v[u] : T(0);
        }
      }
    }
    __syncthreads();
    // TPR threads per input row (all 256 threads busy), partial sums combined by a shuffle inside the 4-lane group
    constexpr int TPR = kThreads / Cfg::RB;
    const int prow = tid / TPR, ppart = tid % TPR;
    T m = T(0);
    if (LOO || a.mean) {
      const T* xr = Xs + prow * Cfg::LDX;
      T m0 = T(0), m1 = T(0);
      for (int c = 2 * ppart; c + 1 < DPc; c += 2 * TPR) { m0 += xr[c] * mwl[c]; m1 += xr[c + 1] * mwl[c + 1]; }
      m = m0 + m1;
#pragma unroll
      for (int o = 1; o < TPR; o <<= 1) m += __shfl_xor(m, o, 64);
    }
    if (use_factor) {
      __syncthreads();  // mean reads rows across the waves' tiles before the sweep rewrites them
      trsm_sweep<T, false>(Xs, P, Linv, nchunks, lane, wave);
    }
    T v = T(0);
    if (want_var) {
      const T* xr = Xs + prow * Cfg::LDX;
      T v0 = T(0), v1 = T(0);
      if (use_factor) {
        for (int c = 2 * ppart; c + 1 < DPc; c += 2 * TPR) { v0 += xr[c] * xr[c]; v1 += xr[c + 1] * xr[c + 1]; }
      } else {  // diagonal precision: var_n = sum_d x_dn^2 / d_d
        for (int c = 2 * ppart; c + 1 < DPc; c += 2 * TPR) { v0 += xr[c] * xr[c] * dinv[c]; v1 += xr[c + 1] * xr[c + 1] * dinv[c + 1]; }
      }
      v = v0 + v1;
#pragma unroll
      for (int o = 1; o < TPR; o <<= 1) v += __shfl_xor(v, o, 64);
    }
    if (ppart == 0 && prow < nt) {
      const int n = n0 + prow;
      if constexpr (LOO) {
        if (!loo_store(l, 0, n, (double)a.y[o0 + n], (double)m, (double)v, (double)(diag_noise ? s[n] : s[0]))) ++ndeg;
      } else {
        if (mean_out) mean_out[n] = m;
        if (var_out) var_out[n] = v + (diag_noise ? s[n] : s[0]);
      }
    }
  }
  if constexpr (LOO) loo_count(ndeg, a.degenerate);
}

// ---- status of a ragged LOO call: loo_check_kernel's rule and order, the noise scan on the regressor's slice ------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void loo_ragged_check_kernel(const T* __restrict__ Tf, int64_t ldt, int64_t strideT, int D,
                                                                    const T* __restrict__ s, int64_t strides, int noise_kind,
                                                                    const int64_t* __restrict__ offsets, int32_t* __restrict__ info) {
  __shared__ int bad[2];
  const int tid = threadIdx.x;
  const int64_t reg = blockIdx.x;
  if (tid == 0) { bad[0] = 0x7fffffff; bad[1] = 0x7fffffff; }
  __syncthreads();
  const T* Tg = Tf + reg * strideT;
  for (int j = tid; j < D; j += kThreads)
    if (!(Tg[(int64_t)j * ldt + j] > T(0))) atomicMin(&bad[0], j + 1);
  const int64_t o0 = offsets[reg];
  const int N = (int)(offsets[reg + 1] - o0);
  const bool diag = noise_kind == NOISE_DIAGONAL;
  const int ns = diag ? N : (N > 0 ? 1 : 0);
  const T* sg = diag ? s + o0 : s + reg * strides;
  for (int i = tid; i < ns; i += kThreads)
    if (!(sg[i] > T(0))) atomicMin(&bad[1], i + 1);  // (i: within the regressor's slice)
  __syncthreads();
  if (tid == 0) info[reg] = bad[0] != 0x7fffffff ? bad[0] : (bad[1] != 0x7fffffff ? bad[1] : 0);
}

// ---- loo_total[reg] = the fixed-order sum of the regressor's log densities ll[offsets[reg] .. offsets[reg + 1]): one order per count ------
// (a plain kernel: declared here, defined in blr_marg_ragged.hip)
__global__ __launch_bounds__(kThreads) void loo_ragged_total_kernel(const double* __restrict__ ll, const int64_t* __restrict__ offsets,
                                                                    double* __restrict__ total, const int32_t* __restrict__ info);

// the instantiations the library uses, defined in blr_marg_ragged.hip
#define BLR_MARG_RAGGED_INSTANCES(X, T)                                                              \
  X __global__ void marg_ragged_gemm_kernel<T, false, false>(MargRaggedArgs<T>, const T*);           \
  X __global__ void marg_ragged_gemm_kernel<T, true, false>(MargRaggedArgs<T>, const T*);            \
  X __global__ void marg_ragged_gemm_kernel<T, false, true>(MargRaggedArgs<T>, const T*);            \
  X __global__ void marg_ragged_gemm_kernel<T, true, true>(MargRaggedArgs<T>, const T*);             \
  X __global__ void marg_ragged_rows_kernel<T, false>(MargRaggedArgs<T>);                            \
  X __global__ void marg_ragged_rows_kernel<T, true>(MargRaggedArgs<T>);                             \
  X __global__ void loo_ragged_check_kernel<T>(const T*, int64_t, int64_t, int, const T*, int64_t, int, const int64_t*, int32_t*);
BLR_MARG_RAGGED_INSTANCES(extern template, double)
BLR_MARG_RAGGED_INSTANCES(extern template, float)

}  // namespace blr
