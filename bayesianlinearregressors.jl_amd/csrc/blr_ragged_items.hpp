// The work items of the ragged marginal stream and the ragged leave-one-out (blr_marginals_ragged_*, blr_loo_ragged_*):
// from `offsets`, the CU count, the element size and the handle's options alone.  Host arithmetic only -- no HIP call and no
// handle -- so the plan can be checked without a device (tools/ragged_items_dump.cpp, tests/test_marg_ragged_cpu.py).
// marg_ragged_plan (blr_abi.hip) uploads a plan's items, marg_ragged_launch turns it into launches.  plan_ragged is also the chunk walk
// and the item cut of the ragged leave-fold-out predictives (blr_kfold_ragged_plan.hpp), which bound a chunk's observations as well.
//
// A regressor's observations are independent once its triangular inverse exists, so a long regressor is cut into items of at
// most W observations and the items -- not the regressors -- are what workgroups take: one workgroup per item.  The bits of an
// observation do not depend on the cut (blr_marg_ragged.hpp), so W is a matter of speed alone:
//   - a whole number of the kernels' tiles: both kernels walk an item in tiles that start at multiples of 64 observations of the
//     regressor (marg_ragged_rows_kernel: one tile of 64 rows; marg_ragged_gemm_kernel: four tiles of 16), so W % 64 == 0;
//   - at least kRaggedMinItem = 256: a workgroup copies the regressor's 74 KB image once -- four 16-input tiles per wave, the
//     bound MargProduct::launch argues for the equal-count stream;
//   - about one round of resident workgroups (two per CU) over the call's observations: ceil(total / (2 CUs)) rounded up.
// Option RAGGED_ITEM (tests) forces W, rounded up to 64.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "blr_host.hpp"  // BlrOptions

namespace blr {

constexpr int kRaggedTile = 16;          // observations per tile of the item table (one MFMA tile of inputs)
constexpr int kRaggedRows = 64;          // observations per tile of the rows kernel = TrsmCfg<T>::RB; items start at multiples of it
constexpr int64_t kRaggedMinItem = 256;  // observations: four 16-input tiles for each of the four waves
constexpr int64_t kRaggedMaxRegs = 65535;                 // regressors of a chunk
constexpr int64_t kRaggedImageBytes = (int64_t)256 << 20;  // images of a chunk
constexpr int64_t kRaggedImageElems = 4 * 36 * 64;         // MargGemmCfg<T>::IMG_ELEMS (asserted in blr_marg_ragged.hpp)

struct RaggedItem {
  int32_t reg;         // regressor (index into the call's batch)
  int32_t first_tile;  // first 16-observation tile of the regressor this item covers
  int32_t ntiles;      // tiles it covers; the regressor's last tile may be partial
};

struct RaggedChunk {
  int64_t b0, nb;        // regressors b0 .. b0 + nb - 1
  int64_t item0, nitems;  // their items: items[item0 .. item0 + nitems - 1]
};

struct RaggedPlan {
  int64_t W = 0;  // observations per item
  std::vector<RaggedChunk> chunks;
  std::vector<RaggedItem> items;  // regressor-major, tiles ascending
  int64_t max_rows = 0, max_nb = 0;  // the most observations / regressors of any chunk: what a per-chunk workspace is sized for
  int64_t last_chunks = 0;
};

inline int64_t ragged_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// observations per item
inline int64_t ragged_item_size(const int64_t* offsets, int64_t B, int cus, const BlrOptions& opt) {
  if (opt.ragged_item > 0) return ragged_round_up(opt.ragged_item, kRaggedRows);
  const int64_t total = B > 0 ? offsets[B] - offsets[0] : 0;
  const int64_t slots = 2 * (int64_t)std::max(cus, 1);
  return std::max<int64_t>(kRaggedMinItem, ragged_round_up((total + slots - 1) / slots, kRaggedRows));
}

// regressors per chunk: grid and image bounds, option MAX_CHUNK; never fewer than one
inline int64_t ragged_chunk_size(int64_t B, int elem, const BlrOptions& opt) {
  int64_t chunk = std::min<int64_t>(std::max<int64_t>(B, 1), kRaggedMaxRegs);
  chunk = std::min<int64_t>(chunk, kRaggedImageBytes / (kRaggedImageElems * (int64_t)elem));
  if (opt.max_chunk > 0) chunk = std::min<int64_t>(chunk, opt.max_chunk);
  return std::max<int64_t>(chunk, 1);
}

// offsets: B + 1 entries, non-decreasing, every count <= 2^30 (the entry points have checked).  row_bound: the most observations of
// a chunk (blr_kfold_ragged_plan.hpp: its rows of Z) -- a chunk never has fewer than one regressor
inline void plan_ragged(const int64_t* offsets, int64_t B, int cus, int elem, const BlrOptions& opt, RaggedPlan& p, int64_t row_bound = INT64_MAX) {
  p.W = ragged_item_size(offsets, B, cus, opt);
  p.chunks.clear();
  p.items.clear();
  p.max_rows = p.max_nb = 0;
  const int64_t most = ragged_chunk_size(B, elem, opt);
  const int64_t wt = p.W / kRaggedTile;  // tiles per full item
  for (int64_t b0 = 0; b0 < B;) {
    RaggedChunk c{b0, 0, (int64_t)p.items.size(), 0};
    int64_t rows = 0;
    for (int64_t b = b0; b < B && c.nb < most; ++b) {
      const int64_t n = offsets[b + 1] - offsets[b];
      if (c.nb > 0 && n > row_bound - rows) break;
      rows += n;
      ++c.nb;
      const int64_t nt = (n + kRaggedTile - 1) / kRaggedTile;
      for (int64_t t = 0; t < nt; t += wt) p.items.push_back(RaggedItem{(int32_t)b, (int32_t)t, (int32_t)std::min<int64_t>(wt, nt - t)});
    }
    c.nitems = (int64_t)p.items.size() - c.item0;
    p.chunks.push_back(c);
    p.max_rows = std::max(p.max_rows, rows);
    p.max_nb = std::max(p.max_nb, c.nb);
    b0 += c.nb;
  }
  p.last_chunks = (int64_t)p.chunks.size();
}

}  // namespace blr
