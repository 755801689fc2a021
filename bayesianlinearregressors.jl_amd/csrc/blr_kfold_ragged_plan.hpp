// The host plan of the ragged leave-fold-out predictives (blr_kfold_ragged_*): from `offsets`, F, D, the CU count, the
// element size and the handle's options alone.  Host arithmetic only -- no HIP call and no handle -- so the plan can be checked
// without a device (tools/kfold_ragged_plan_dump.cpp, tests/test_kfold_ragged_cpu.py).  kfold_ragged (blr_abi.hip) turns it into
// launches.
//   fold_offsets[B + 1]  regressor b owns the folds [fold_offsets[b], fold_offsets[b + 1]) of kf_logpdf: nfolds_b = ceil(N_b / F);
//   pack_offsets[B + 1]  ... and the fold packs [pack_offsets[b], pack_offsets[b + 1]): a pack is floor(64 / F) consecutive folds of
//                        ONE regressor (kfold_kernel's unit, blr_kfold.hpp), so no pack straddles two regressors; kfold_ragged_kernel
//                        finds its regressor by a binary search in this table;
//   chunks               consecutive regressors whose rows of Z (blr_kfold_ragged.hpp: DP = 16 ceil(D / 16) elements per observation,
//                        packed as the observations are) stay within 256 MiB -- never fewer than one regressor -- on top of the
//                        bounds of blr_ragged_items.hpp (65535 regressors, 256 MiB of images, option MAX_CHUNK);
//   items                the whitening pass's work items of every chunk: plan_ragged's (the same W, the same cut).
// plan_kfold_ragged fills the two tables and leaves chunks and items to plan_ragged with the bound on a chunk's rows.
#pragma once

#include "blr_ragged_items.hpp"

namespace blr {

constexpr int kFoldRaggedMaxF = 64;                      // = kFoldMax (asserted in blr_kfold_ragged.hpp)
constexpr int64_t kFoldRaggedZBytes = (int64_t)256 << 20;  // rows of Z of a chunk

struct KfoldRaggedPlan : RaggedPlan {  // W, chunks, items: the whitening pass's
  std::vector<int64_t> pack_offsets, fold_offsets;  // [B + 1]
};

inline int64_t kfold_ragged_folds(int64_t n, int64_t F) { return (n + F - 1) / F; }
inline int64_t kfold_ragged_pack_rows(int64_t F) { return (kFoldRaggedMaxF / F) * F; }

// fold_offsets alone (blr_kfold_ragged_fold_offsets): out[0] = 0, out[b + 1] = out[b] + ceil(N_b / F)
inline void kfold_ragged_fold_offsets(const int64_t* offsets, int64_t B, int64_t F, int64_t* out) {
  out[0] = 0;
  for (int64_t b = 0; b < B; ++b) out[b + 1] = out[b] + kfold_ragged_folds(offsets[b + 1] - offsets[b], F);
}

// offsets: B + 1 entries, non-decreasing, every count <= 2^30; 1 <= F <= 64; 1 <= D <= 128 (the entry points have checked)
inline void plan_kfold_ragged(const int64_t* offsets, int64_t B, int64_t F, int D, int cus, int elem, const BlrOptions& opt, KfoldRaggedPlan& p) {
  p.pack_offsets.assign((size_t)B + 1, 0);
  p.fold_offsets.assign((size_t)B + 1, 0);
  const int64_t pr = kfold_ragged_pack_rows(F);
  kfold_ragged_fold_offsets(offsets, B, F, p.fold_offsets.data());
  for (int64_t b = 0; b < B; ++b) p.pack_offsets[(size_t)b + 1] = p.pack_offsets[(size_t)b] + (offsets[b + 1] - offsets[b] + pr - 1) / pr;
  const int64_t row_bytes = (int64_t)16 * ((D + 15) / 16) * elem;
  plan_ragged(offsets, B, cus, elem, opt, p, kFoldRaggedZBytes / row_bytes);
}

}  // namespace blr
