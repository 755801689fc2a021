// The host plan of the ragged large-fold leave-fold-out predictives (blr_kfold_large_ragged_*): from `offsets`,
// `fold_sizes`, D, the CU count, the element size and the handle's options alone.  Host arithmetic only -- no HIP call and no handle --
// so the plan can be checked without a device (tools/kfold_large_ragged_plan_dump.cpp, tests/test_kfold_large_ragged_cpu.py).
// kfold_large_ragged (blr_abi.hip) uploads its tables and turns it into launches.
//   regs[B]     per regressor: its first observation, N_b, F_b (clamped to N_b: a fold size beyond the count is one fold), nfolds_b,
//               the first fold of kf_logpdf it owns (fold_offsets[b]) and its first statistics slot; fold f of the regressor has
//               kfl_splits(n_f) slots from slot0 + f S_b on, S_b the slots of a FULL fold: a short last fold takes the slots it uses
//               and no more, so the regressor owns (nfolds_b - 1) S_b + S_last slots;
//   stat        the statistics pass's work items (regressor, fold, column block), regressor-major, folds and blocks ascending;
//   red         the folds with more than one column block: (regressor, fold), `nparts` their block count;
//   pred        the predict pass's work items (regressor, fold, tile group): group g of `nparts` takes the 64-row tiles g, g + nparts,
//               ... of its fold; a group amortises the fold's image over about `tiles_per_group` tiles;
//   chunks      consecutive regressors whose statistics, factors U_f, means mw_f and images stay within 256 MiB each, whose flat grids
//               stay within kKflrMaxGrid workgroups, at most 65535 of them and at most option MAX_CHUNK -- never fewer than one.
// Folds, slots and items of a chunk are contiguous in the call's numbering: the kernels index a chunk's workspace by (fold -
// chunk.fold0) and (slot - chunk.slot0).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "blr_host.hpp"  // BlrOptions
#include "blr_kfold_large_splits.hpp"

namespace blr {

constexpr int64_t kKflrMaxFolds = 1024;               // = kFoldLargeMaxFolds (asserted in blr_kfold_large_ragged.hpp)
constexpr int64_t kKflrBytes = (int64_t)256 << 20;    // each per-chunk workspace
constexpr int64_t kKflrMaxRegs = 65535;               // regressors of a chunk
constexpr int64_t kKflrMaxGrid = (int64_t)1 << 23;    // workgroups of a flat launch (256 threads each: below 2^32 threads)
constexpr int64_t kKflrImageElems = 4 * 36 * 64;      // MargGemmCfg<T>::IMG_ELEMS (asserted in blr_kfold_large_ragged.hpp)
constexpr int64_t kKflrTile = 64;                     // rows of a predict tile = kCovTile
constexpr int64_t kKflrMinTiles = 4;                  // tiles a predict group takes at least: the image is 74 KB, a tile 64 KB

struct KflrReg {
  int64_t row0;    // offsets[b]
  int64_t fold0;   // fold_offsets[b]
  int64_t slot0;   // first statistics slot
  int32_t n, F;    // N_b; min(F_b, max(N_b, 1))
  int32_t nfolds;  // ceil(N_b / F)
  int32_t S;       // slots of a full fold: kfl_blocks(F)
};

struct KflrItem {
  int32_t reg, fold;
  int32_t part, nparts;  // statistics: column block of S_f; reduce: 0 of S_f; predict: tile group of the fold's groups
};

struct KflrChunk {
  int64_t b0, nb;
  int64_t fold0, nfolds;  // the chunk's folds: [fold0, fold0 + nfolds) of the call
  int64_t slot0, nslots;
  int64_t stat0, nstat, red0, nred, pred0, npred;  // its items in the three tables
};

struct KflrPlan {
  std::vector<KflrReg> regs;
  std::vector<int64_t> fold_offsets;  // [B + 1]
  std::vector<KflrItem> stat, red, pred;
  std::vector<KflrChunk> chunks;
  int64_t tiles_per_group = 0;
  int64_t max_nb = 0, max_folds = 0, max_slots = 0;  // the most of any chunk: what the per-chunk workspace is sized for
  int64_t last_chunks = 0;
};

inline int64_t kflr_folds(int64_t n, int64_t F) { return n == 0 ? 0 : (F >= n ? 1 : (n + F - 1) / F); }

// F_b = max(1, ceil(N_b / K)) (blr_kfold_large_ragged_fold_sizes)
inline void kflr_fold_sizes(const int64_t* offsets, int64_t B, int64_t K, int64_t* out) {
  for (int64_t b = 0; b < B; ++b) out[b] = std::max<int64_t>(1, (offsets[b + 1] - offsets[b] + K - 1) / K);
}
// out[0] = 0, out[b + 1] = out[b] + nfolds_b (blr_kfold_large_ragged_fold_offsets)
inline void kflr_fold_offsets(const int64_t* offsets, const int64_t* fold_sizes, int64_t B, int64_t* out) {
  out[0] = 0;
  for (int64_t b = 0; b < B; ++b) out[b + 1] = out[b] + kflr_folds(offsets[b + 1] - offsets[b], fold_sizes[b]);
}

// offsets: B + 1 entries, non-decreasing, every count <= 2^30; fold_sizes: B entries >= 1 with at most 1024 folds each; 1 <= D <= 128
// (the entry points have checked)
inline void plan_kfold_large_ragged(const int64_t* offsets, const int64_t* fold_sizes, int64_t B, int D, int cus, int elem, const BlrOptions& opt,
                                    KflrPlan& p) {
  p = KflrPlan();
  p.regs.resize((size_t)B);
  p.fold_offsets.assign((size_t)B + 1, 0);
  int64_t slot = 0, tiles = 0;
  for (int64_t b = 0; b < B; ++b) {
    KflrReg& r = p.regs[(size_t)b];
    const int64_t n = offsets[b + 1] - offsets[b];
    r.row0 = offsets[b];
    r.n = (int32_t)n;
    r.F = (int32_t)std::min<int64_t>(fold_sizes[b], std::max<int64_t>(n, 1));
    r.nfolds = (int32_t)kflr_folds(n, r.F);
    r.S = kfl_blocks(r.F);
    r.fold0 = p.fold_offsets[(size_t)b];
    r.slot0 = slot;
    p.fold_offsets[(size_t)b + 1] = r.fold0 + r.nfolds;
    if (r.nfolds > 0) {
      const int64_t last = n - (int64_t)(r.nfolds - 1) * r.F;
      slot += (int64_t)(r.nfolds - 1) * r.S + kfl_blocks((int)last);
      tiles += (int64_t)(r.nfolds - 1) * ((r.F + kKflrTile - 1) / kKflrTile) + (last + kKflrTile - 1) / kKflrTile;
    }
  }
  // about one round of resident workgroups (two per CU) over the call's tiles, and never so few tiles that the image dominates
  const int64_t slots2 = 2 * (int64_t)std::max(cus, 1);
  p.tiles_per_group = std::max<int64_t>(kKflrMinTiles, (tiles + slots2 - 1) / slots2);

  const int64_t DP = 16 * (((int64_t)D + 15) / 16);
  const int64_t stat_bytes = (DP * (DP + 1) / 2 + DP) * (int64_t)sizeof(double), u_bytes = (int64_t)D * D * elem, img_bytes = kKflrImageElems * elem;
  const int64_t max_slots = kKflrBytes / stat_bytes, max_folds = std::min(kKflrBytes / u_bytes, kKflrBytes / img_bytes);
  int64_t most = std::min<int64_t>(std::max<int64_t>(B, 1), kKflrMaxRegs);
  if (opt.max_chunk > 0) most = std::min<int64_t>(most, opt.max_chunk);
  for (int64_t b0 = 0; b0 < B;) {
    KflrChunk c{};
    c.b0 = b0;
    c.fold0 = p.regs[(size_t)b0].fold0; c.slot0 = p.regs[(size_t)b0].slot0;
    c.stat0 = (int64_t)p.stat.size(); c.red0 = (int64_t)p.red.size(); c.pred0 = (int64_t)p.pred.size();
    for (int64_t b = b0; b < B && c.nb < most; ++b) {
      const KflrReg& r = p.regs[(size_t)b];
      const int64_t nslots = (b + 1 < B ? p.regs[(size_t)b + 1].slot0 : slot) - r.slot0;
      int64_t ngroups = 0;  // of the regressor's folds
      for (int32_t f = 0; f < r.nfolds; ++f) {
        const int64_t nt = (std::min<int64_t>(r.F, r.n - (int64_t)f * r.F) + kKflrTile - 1) / kKflrTile;
        ngroups += (nt + p.tiles_per_group - 1) / p.tiles_per_group;
      }
      if (c.nb > 0 && (c.nslots + nslots > max_slots || c.nfolds + r.nfolds > max_folds || c.nstat + nslots > kKflrMaxGrid ||
                       c.npred + ngroups > kKflrMaxGrid))
        break;
      ++c.nb;
      c.nfolds += r.nfolds; c.nslots += nslots;
      for (int32_t f = 0; f < r.nfolds; ++f) {
        const int64_t nf = std::min<int64_t>(r.F, r.n - (int64_t)f * r.F);
        const int32_t Sf = kfl_blocks((int)nf);
        for (int32_t sp = 0; sp < Sf; ++sp) p.stat.push_back(KflrItem{(int32_t)b, f, sp, Sf});
        if (Sf > 1) p.red.push_back(KflrItem{(int32_t)b, f, 0, Sf});
        const int64_t nt = (nf + kKflrTile - 1) / kKflrTile;
        const int32_t ng = (int32_t)((nt + p.tiles_per_group - 1) / p.tiles_per_group);
        for (int32_t g = 0; g < ng; ++g) p.pred.push_back(KflrItem{(int32_t)b, f, g, ng});
      }
      c.nstat = (int64_t)p.stat.size() - c.stat0; c.nred = (int64_t)p.red.size() - c.red0; c.npred = (int64_t)p.pred.size() - c.pred0;
    }
    p.chunks.push_back(c);
    p.max_nb = std::max(p.max_nb, c.nb);
    p.max_folds = std::max(p.max_folds, c.nfolds);
    p.max_slots = std::max(p.max_slots, c.nslots);
    b0 += c.nb;
  }
  p.last_chunks = (int64_t)p.chunks.size();
}

}  // namespace blr
