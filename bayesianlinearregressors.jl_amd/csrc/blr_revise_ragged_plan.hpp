// The host plan of the ragged condition / forget pair (blr_update_factor_ragged_*, blr_downdate_factor_ragged_*):
// from `offsets`, D and three of the handle's options alone.  Host arithmetic only -- standard headers, no HIP header and no handle
// -- so the plan is compiled with the host compiler and checked without a device (tools/revise_ragged_plan_dump.cpp,
// tests/test_revise_ragged_cpu.py).  revise_ragged (blr_abi.hip) turns it into launches.
//   idle    regressors with k_b = 0, ascending: they cost no workgroup (revise_ragged_idle_kernel fills their status);
//   sweep   regressors that take the per-observation body: the Givens sweep of an update, the LDS body of a downdate;
//   refit   regressors of an update whose state is re-factored in place (fused_ragged_kernel, their list as its `order`).
// The active lists are sorted by descending k_b, ties by index: K14's longest-first rule.  The route of a regressor follows from
// (D, k_b, options) and nothing else -- never from B or from the other regressors: every bit promise of the pair rests on that.
//   update    k_b = 1 -> sweep, k_b >= 2 -> refit; SWEEP=always: k_b <= kReviseSweepMaxK -> sweep; SWEEP=never: all refit;
//             D > kReviseMaxD: all refit (what blr_update_factor_* does there);
//   downdate  every active regressor -> sweep.
// `serial`: D > kReviseMaxD, or a downdate under NO_DOWNDATE_LDS -- correct, not fast: the active regressors go one after the
// other through the equal-count entry point.  MAX_CHUNK caps the regressors of a launch; last_chunks counts the launches of the
// two active lists (0 when every regressor is idle; the serial route: one per active regressor).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace blr {

constexpr int kReviseMaxD = 128;       // = kSweepMaxD = kDowndateLdsMaxD (asserted in blr_revise_ragged.hpp)
constexpr int kReviseSweepMaxK = 16;   // = kSweepMaxK

struct ReviseRaggedPlan {
  std::vector<int32_t> idle, sweep, refit;
  bool serial = false;
  int64_t chunk = 1;        // regressors per launch of an active list
  int64_t last_chunks = 0;
};

// where one regressor goes: 0 idle, 1 sweep, 2 refit
inline int revise_ragged_route(bool downdate, int64_t D, int64_t k, int sweep_mode) {
  if (k == 0) return 0;
  if (downdate) return 1;
  if (D > kReviseMaxD || sweep_mode == 2) return 2;
  if (sweep_mode == 1) return k <= kReviseSweepMaxK ? 1 : 2;
  return k == 1 ? 1 : 2;
}

// offsets: B + 1 entries, non-decreasing, every count <= 2^30 (the entry points have checked).  Opt: BlrOptions, or any record
// with its members sweep (0 router, 1 always, 2 never), max_chunk (0: none) and no_downdate_lds.
template <typename Opt>
inline void plan_revise_ragged(const int64_t* offsets, int64_t B, int64_t D, bool downdate, const Opt& opt, ReviseRaggedPlan& p) {
  p.idle.clear();
  p.sweep.clear();
  p.refit.clear();
  for (int64_t b = 0; b < B; ++b) {
    const int route = revise_ragged_route(downdate, D, offsets[b + 1] - offsets[b], opt.sweep);
    (route == 0 ? p.idle : route == 1 ? p.sweep : p.refit).push_back((int32_t)b);
  }
  const auto longest_first = [offsets](int32_t i, int32_t j) { return offsets[i + 1] - offsets[i] > offsets[j + 1] - offsets[j]; };
  std::stable_sort(p.sweep.begin(), p.sweep.end(), longest_first);
  std::stable_sort(p.refit.begin(), p.refit.end(), longest_first);
  p.serial = D > kReviseMaxD || (downdate && opt.no_downdate_lds);
  const int64_t ns = (int64_t)p.sweep.size(), nr = (int64_t)p.refit.size();
  p.chunk = std::max<int64_t>(1, std::max(ns, nr));
  if (opt.max_chunk > 0) p.chunk = std::min<int64_t>(p.chunk, opt.max_chunk);
  p.last_chunks = p.serial ? ns + nr : (ns + p.chunk - 1) / p.chunk + (nr + p.chunk - 1) / p.chunk;
}

}  // namespace blr
