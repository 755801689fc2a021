// kfl_splits: the one function the large-fold K-fold kernels (blr_kfold_large.hpp, blr_kfold_large_ragged.hpp) and the host planner of
// the unequal-count form (blr_kfold_large_ragged_plan.hpp) share -- where a fold's statistics slots lie follows from it on both sides.
#pragma once
#include <hip/hip_runtime.h>

namespace blr {

// Column blocks of a fold's statistics pass, a function of its own row count alone (grid_splits of blr_grid.hpp on n_f): blocks of
// about 1024 rows, at most 8, whole stages of 64.  A shorter last fold has no more blocks than a full one.
__host__ __device__ inline void kfl_splits(int nf, int* S, int* chunk) {
  int s = nf / 1024;
  s = s < 1 ? 1 : (s > 8 ? 8 : s);
  int c = (nf + s - 1) / s;
  c = (c + 63) / 64 * 64;
  *S = s;
  *chunk = c < 64 ? 64 : c;
}

inline int kfl_blocks(int nf) {
  int s = 1, c = 64;
  kfl_splits(nf, &s, &c);
  return s;
}

}  // namespace blr
