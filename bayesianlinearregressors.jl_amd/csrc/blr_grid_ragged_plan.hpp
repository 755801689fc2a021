// The host plan of the ragged evidence grid (blr_logpdf_grid_ragged_*): from `offsets` alone.  Host arithmetic only --
// standard headers, no HIP header and no handle -- so the plan is compiled with the host compiler and checked without a device
// (tools/grid_ragged_plan_dump.cpp, tests/test_grid_ragged_cpu.py).  logpdf_grid_ragged (blr_abi.hip) turns it into launches.
//   slot0   [B + 1]: regressor b owns the statistics slots slot0[b] .. slot0[b] + S_b - 1, S_b = grid_ragged_splits(N_b): the slots are
//           dense, column block 0 of a regressor comes first and holds the sums once the reduce kernel has run;
//   items   one per (regressor, column block): {reg, n0, n, slot} -- block `slot - slot0[reg]` covers the observations n0 .. n0 + n - 1
//           of the regressor's own slice.  Sorted by descending n, ties by (reg, block): the hardware dispatches workgroups in order,
//           so this is K14's longest-first rule on column blocks -- one regressor of 2^20 observations runs on eight workgroups at once.
// The blocks of a regressor follow from its own count and nothing else -- never from B or from the other regressors: they are the
// blocks blr_logpdf_grid_* cuts at N = N_b, and the bit promise of the entry point rests on that.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace blr {

// grid_splits (blr_grid.hpp) restated for the host compiler: blocks of about 1024 columns, at most 8, whole stages of 64
inline void grid_ragged_splits(int64_t N, int* S, int* chunk) {
  const int64_t s = std::max<int64_t>(1, std::min<int64_t>(8, N / 1024));
  int64_t c = (N + s - 1) / s;
  c = (c + 63) / 64 * 64;
  *S = (int)s;
  *chunk = (int)std::max<int64_t>(c, 64);
}

struct GridRaggedItem {
  int32_t reg, n0, n, slot;
};

struct GridRaggedPlan {
  std::vector<int32_t> slot0;  // [B + 1], the prefix sums of S_b
  std::vector<GridRaggedItem> items;
  int64_t slots = 0;           // sum of S_b
  bool reduce = false;         // some S_b > 1
};

// sum of S_b: the entry point bounds it before anything is allocated
inline int64_t grid_ragged_slots(const int64_t* offsets, int64_t B) {
  int64_t slots = 0;
  for (int64_t b = 0; b < B; ++b) {
    int S, chunk;
    grid_ragged_splits(offsets[b + 1] - offsets[b], &S, &chunk);
    slots += S;
  }
  return slots;
}

// offsets: B + 1 entries, non-decreasing, every count <= 2^30, B and the sum of S_b below 2^24 (the entry point has checked)
inline void plan_grid_ragged(const int64_t* offsets, int64_t B, GridRaggedPlan& p) {
  p.slot0.assign((size_t)B + 1, 0);
  p.items.clear();
  p.reduce = false;
  int64_t slot = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t N = offsets[b + 1] - offsets[b];
    int S, chunk;
    grid_ragged_splits(N, &S, &chunk);
    p.slot0[(size_t)b] = (int32_t)slot;
    for (int sp = 0; sp < S; ++sp) {
      const int64_t n0 = (int64_t)sp * chunk;
      const int64_t n = std::max<int64_t>(0, std::min<int64_t>(chunk, N - n0));
      p.items.push_back({(int32_t)b, (int32_t)n0, (int32_t)n, (int32_t)(slot + sp)});
    }
    slot += S;
    p.reduce = p.reduce || S > 1;
  }
  p.slot0[(size_t)B] = (int32_t)slot;
  p.slots = slot;
  // (built in (reg, block) order: a stable sort keeps it among equal n)
  std::stable_sort(p.items.begin(), p.items.end(), [](const GridRaggedItem& a, const GridRaggedItem& b) { return a.n > b.n; });
}

}  // namespace blr
