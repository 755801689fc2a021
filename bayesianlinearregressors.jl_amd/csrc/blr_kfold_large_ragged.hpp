// Exact leave-fold-out (K-fold) predictives for LARGE folds of a batch whose regressors have UNEQUAL observation counts and their
// own fold sizes (blr_kfold_large_ragged_*): the formulas, the precision and the launch list of blr_kfold_large.hpp
// (K24) on every regressor's slice of the packed layout (blr_ragged.hpp).  Regressor b owns observations [offsets[b], offsets[b + 1])
// of X, y, a diagonal s, kf_mean and kf_var and the folds [fold_offsets[b], fold_offsets[b + 1]) of kf_logpdf; its fold f is
// [f F_b, min((f + 1) F_b, N_b)) of ITS slice.  Where K24's grids are (fold x S, regressor) rectangles, these are flat and driven
// by the tables of blr_kfold_large_ragged_plan.hpp; per chunk of regressors, after the status (loo_ragged_check_kernel):
//   kfl_state_kernel      (blr_kfold_large.hpp, as it is) one workgroup per regressor: A = T'T, logdet A
//   kflr_stats_kernel     one workgroup per statistics item (regressor, fold, column block): kfl_stats_body
//   kflr_stats32_kernel   the same grid in fp32: kfl_stats32_body
//   kflr_reduce_kernel    one workgroup per fold with more than one block: kfl_reduce_body
//   kflr_factor_kernel    one workgroup per fold of the chunk, its regressor by a binary search in fold_offsets: kfl_factor_body
//   marg_image_kernel     over the chunk's factors U_f
//   kflr_predict_kernel   one workgroup per predict item (regressor, fold, tile group): kfl_predict_body
// and the totals (loo_ragged_total_kernel over fold_offsets).  Every kernel fills a KflFold with the fold's pointers and runs the
// body the rectangular kernel of K24 runs: the same instructions on the same rows.  A fold's column blocks follow from its own row
// count (kfl_splits), its tiles start at multiples of 64 of ITS rows, a tile's result does not depend on the group that takes it
// and rows are bounded by n_f structurally.  So every output of regressor b has the bits blr_kfold_large_batched_* with B = 1,
// N = N_b, F = F_b gives on that slice: they depend neither on B, on the neighbours, on the chunking nor on the outputs requested.
#pragma once
#include "blr_kfold_large.hpp"
#include "blr_kfold_large_ragged_plan.hpp"

namespace blr {

static_assert(kKflrMaxFolds == kFoldLargeMaxFolds, "the planner's fold bound");
static_assert(kKflrImageElems == MargGemmCfg<double>::IMG_ELEMS && kKflrImageElems == MargGemmCfg<float>::IMG_ELEMS, "the planner's image size");
static_assert(kKflrTile == kCovTile, "the planner's predict tile");

template <typename T>
struct KflrArgs {
  const T* X; int64_t ldx;           // packed inputs
  const T* y;                        // packed targets
  const T* s; int64_t strides;       // diagonal noise: packed; isotropic: one value per regressor, strides apart
  const T* mw; int64_t stridemw;
  const int32_t* info;               // [B] status: a regressor with info != 0 is skipped
  const KflrReg* regs;               // [B], device
  const int64_t* fold_offsets;       // [B + 1], device
  const KflrItem* items;             // the launch's items, device
  T* km; T* kv; double* kl;          // packed outputs (may be NULL): km, kv by observations, kl by folds
  unsigned long long* degenerate;
  // workspace of one chunk: A, ldA by the chunk-local regressor; stats, scal by (slot - slot0); U, mwf, finfo, img by (fold - fold0)
  double* A; double* ldA; double* stats; double* scal;
  T* U; T* mwf; int32_t* finfo; const T* img;
  int64_t fold0, slot0;
  int layout, noise_kind, D;
  int b0, nb;                        // the chunk's regressors
};

// the view's inputs of rows [n0, n0 + n) of regressor `reg`
template <typename T>
__device__ __forceinline__ void kflr_rows(const KflrArgs<T>& a, const KflrReg& rg, int64_t reg, int n0, int n, KflFold<T>& v) {
  const int64_t o = rg.row0 + n0;
  v.X = a.X + (a.layout == LAYOUT_COLVECS ? o * a.ldx : o);
  v.y = a.y + o;
  v.s = a.noise_kind == NOISE_DIAGONAL ? a.s + o : a.s + reg * a.strides;  // (diagonal noise: the index counts within the slice)
  v.mw = a.mw + reg * a.stridemw;
  v.ldx = a.ldx; v.D = a.D; v.noise_kind = a.noise_kind; v.n = n;
}

// rows of fold f of a regressor
__device__ __forceinline__ int kflr_fold_rows(const KflrReg& rg, int f) { return min(rg.F, rg.n - f * rg.F); }

// the item's column block -> false: its regressor is skipped
template <typename T>
__device__ __forceinline__ bool kflr_block(const KflrArgs<T>& a, int SZ, KflFold<T>& v) {
  const KflrItem it = a.items[blockIdx.x];
  if (a.info[it.reg] != 0) return false;  // (block-uniform)
  const KflrReg rg = a.regs[it.reg];
  const int nf = kflr_fold_rows(rg, it.fold);
  int Sf, chunk;
  kfl_splits(nf, &Sf, &chunk);
  kflr_rows(a, rg, it.reg, it.fold * rg.F + it.part * chunk, max(0, min(chunk, nf - it.part * chunk)), v);
  const int64_t slot = rg.slot0 - a.slot0 + (int64_t)it.fold * rg.S + it.part;
  v.stats = a.stats + slot * SZ;
  v.scal = a.scal + 2 * slot;
  return true;
}

template <typename T, int NB, int MODE>
__global__ BLR_KFL_BOUNDS(T, NB) void kflr_stats_kernel(KflrArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  KflFold<T> v;
  if (!kflr_block(a, kfl_stat_elems<T, NB>(), v)) return;
  kfl_stats_body<T, NB, MODE>(smem, v);
}

template <int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void kflr_stats32_kernel(KflrArgs<float> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double scr[kWaves];
  const int DP = 16 * ((a.D + 15) / 16);
  KflFold<float> v;
  if (!kflr_block(a, DP * (DP + 1) / 2 + DP, v)) return;
  kfl_stats32_body<LAYOUT>(smem, scr, v);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void kflr_reduce_kernel(KflrArgs<T> a, int SZ) {
  const KflrItem it = a.items[blockIdx.x];  // a fold of nparts > 1 blocks
  if (a.info[it.reg] != 0) return;
  const KflrReg rg = a.regs[it.reg];
  const int64_t slot = rg.slot0 - a.slot0 + (int64_t)it.fold * rg.S;
  kfl_reduce_body(a.stats + slot * SZ, a.scal + 2 * slot, it.nparts, SZ, threadIdx.x, kThreads, threadIdx.x == 0);
}

template <typename T, int NB>
__global__ __launch_bounds__(kThreads, 2) void kflr_factor_kernel(KflrArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = SmallCfg<T, NB>;
  // the fold's regressor: the last j < nb with fold_offsets[b0 + j] <= this fold (empty regressors own no fold)
  const int64_t* const tbl = a.fold_offsets + a.b0;
  const int64_t fold = a.fold0 + blockIdx.x, rf = blockIdx.x;
  int lo = 0, hi = a.nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tbl[mid] <= fold) lo = mid; else hi = mid;
  }
  const int64_t reg = (int64_t)a.b0 + lo;
  if (a.info[reg] != 0) {  // (block-uniform) nothing of this regressor is computed: no image, no prediction
    if (threadIdx.x == 0) a.finfo[rf] = 1;
    return;
  }
  const KflrReg rg = a.regs[reg];
  const int f = (int)(fold - rg.fold0);
  const int64_t slot = rg.slot0 - a.slot0 + (int64_t)f * rg.S;
  KflFold<T> v;
  v.mw = a.mw + reg * a.stridemw;
  v.D = a.D; v.n = kflr_fold_rows(rg, f);
  v.stats = a.stats + slot * kfl_stat_elems<T, NB>();
  v.scal = a.scal + 2 * slot;
  v.A = a.A + (int64_t)lo * C::PACKED;
  v.ldA = a.ldA + lo;
  v.U = a.U + rf * (int64_t)a.D * a.D;
  v.mwf = a.mwf + rf * a.D;
  v.finfo = a.finfo + rf;
  v.kl = a.kl ? a.kl + fold : nullptr;
  v.degenerate = a.degenerate;
  kfl_factor_body<T, NB>(smem, v);
}

template <typename T, int LAYOUT /* LAYOUT_COLVECS | LAYOUT_ROWVECS */>
__global__ __launch_bounds__(kThreads, 2) void kflr_predict_kernel(KflrArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const KflrItem it = a.items[blockIdx.x];
  if (a.info[it.reg] != 0) return;  // (block-uniform) outputs untouched
  const KflrReg rg = a.regs[it.reg];
  const int64_t rf = rg.fold0 - a.fold0 + it.fold;
  const int f0 = it.fold * rg.F;
  KflFold<T> v;
  kflr_rows(a, rg, it.reg, f0, kflr_fold_rows(rg, it.fold), v);
  v.mwf = a.mwf + rf * a.D;
  v.finfo = a.finfo + rf;
  v.img = a.img + rf * MargGemmCfg<T>::IMG_ELEMS;
  v.km = a.km ? a.km + rg.row0 + f0 : nullptr;
  v.kv = a.kv ? a.kv + rg.row0 + f0 : nullptr;
  v.grp = it.part; v.ngroups = it.nparts;
  kfl_predict_body<T, LAYOUT>(smem, v);
}

// the instantiations the library uses, defined in blr_kfold_large_ragged.hip
#define BLR_KFLR_STATS(X, NB)                                                  \
  X __global__ void kflr_stats_kernel<double, NB, 0>(KflrArgs<double>);        \
  X __global__ void kflr_stats_kernel<double, NB, 1>(KflrArgs<double>);        \
  X __global__ void kflr_stats_kernel<double, NB, 4>(KflrArgs<double>);
#define BLR_KFLR_NB(X, T, NB) X __global__ void kflr_factor_kernel<T, NB>(KflrArgs<T>);
#define BLR_KFLR_INSTANCES(X, T)                                                                                              \
  BLR_KFLR_NB(X, T, 1) BLR_KFLR_NB(X, T, 2) BLR_KFLR_NB(X, T, 3) BLR_KFLR_NB(X, T, 4) BLR_KFLR_NB(X, T, 5) BLR_KFLR_NB(X, T, 6) \
  BLR_KFLR_NB(X, T, 7) BLR_KFLR_NB(X, T, 8)                                                                                   \
  X __global__ void kflr_reduce_kernel<T>(KflrArgs<T>, int);                                                                  \
  X __global__ void kflr_predict_kernel<T, LAYOUT_COLVECS>(KflrArgs<T>);                                                      \
  X __global__ void kflr_predict_kernel<T, LAYOUT_ROWVECS>(KflrArgs<T>);
#define BLR_KFLR_ALL(X)                                                                                              \
  BLR_KFLR_STATS(X, 1) BLR_KFLR_STATS(X, 2) BLR_KFLR_STATS(X, 3) BLR_KFLR_STATS(X, 4) BLR_KFLR_STATS(X, 5)           \
  BLR_KFLR_STATS(X, 6) BLR_KFLR_STATS(X, 7) BLR_KFLR_STATS(X, 8)                                                     \
  X __global__ void kflr_stats32_kernel<LAYOUT_COLVECS>(KflrArgs<float>);                                            \
  X __global__ void kflr_stats32_kernel<LAYOUT_ROWVECS>(KflrArgs<float>);                                            \
  BLR_KFLR_INSTANCES(X, double)                                                                                      \
  BLR_KFLR_INSTANCES(X, float)
BLR_KFLR_ALL(extern template)

}  // namespace blr
