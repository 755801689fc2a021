// The plan of one large-D update (D > 128): route, split-K factors, workspace layout and the group size that will run, from the
// shape of the call alone.  Host arithmetic only -- no HIP call and no handle -- so every decision here can be checked without a
// device (tools/large_plan_dump.cpp, tests/test_large_plan_cpu.py).  posterior_large_group (blr_abi.hip) turns a plan into launches.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <queue>
#include <vector>

#include "blr_planes.hpp"  // kPB, LargeCfg, PlanesCfg, kPlanesChunkKb: the kernels' own tile constants
#include "blr_host.hpp"    // BlrOptions

namespace blr {

// Byte offsets of a workspace's buffers, one after the other, each rounded up to 256 bytes; `off` is the end of the last one.
struct Carve {
  size_t off = 0;
  size_t operator()(size_t bytes) {
    const size_t o = off;
    off = (off + bytes + 255) & ~(size_t)255;
    return o;
  }
};

// "X goes through the LDS-DMA ring": ColVecs whose base and leading dimension are multiples of 16 bytes.  (Whether the ring loop
// is switched on, and whether a decision also needs whole row blocks, is the caller's business.)
inline bool x_ring(int layout, bool aligned) { return layout == LAYOUT_COLVECS && aligned; }
template <typename T>
inline bool x_ring(int layout, const T* X, int64_t ldx) {
  return x_ring(layout, ((uintptr_t)X % 16 == 0) && ((ldx * (int64_t)sizeof(T)) % 16 == 0));
}

// Dynamic LDS of planes_kernel: the chunk's r, sqrt(w) and mu (16 floats per k-block each), then for a basis its raw inputs --
// the whole chunk's, padded to 8 input dimensions (xs_chunk), or one k-block's [Din][16].
constexpr size_t planes_pass_lds(bool rff, bool xs_chunk, int din) {
  return (size_t)(3 * 16 * kPlanesChunkKb + (rff ? (xs_chunk ? 8 * 16 * kPlanesChunkKb : din * 16) : 0)) * sizeof(float);
}
// blr_posterior_rff_f32 evaluates the basis inside the planes pass up to this input dimension: the largest whose pass fits in
// 64 KiB of LDS.  A conservative choice, not the hardware's limit: a gfx950 workgroup may use up to 160 KiB (D_in 2368), and the
// pass was measured to launch beyond 64 KiB without a raised attribute; 64 KiB is what HIP grants by default.
// A larger D_in materialises the features (rff_features_kernel) and runs the planes Gram on them -- so do D_in 833 .. 2368,
// which used to run fused (D_in >= 2369 failed to launch).
constexpr int kRffFusedMaxDin = 832;
static_assert(planes_pass_lds(true, true, 8) <= 65536 && planes_pass_lds(true, false, kRffFusedMaxDin) <= 65536 &&
                  planes_pass_lds(true, false, kRffFusedMaxDin + 1) > 65536,
              "kRffFusedMaxDin: the largest D_in whose planes pass fits in 64 KiB of LDS (the chosen cap)");

// Regressors share the launches of an update as long as their workspaces fit this many bytes (per handle; option CHAIN_WS_MB lowers
// the bound, blr_release_workspace hands the memory back: the scratch buffers of a handle only ever grow otherwise)
constexpr size_t kChainWorkspace = (size_t)8 << 30;
inline size_t large_ws_cap(const BlrOptions& opt) {
  return opt.chain_ws_mb > 0 ? (size_t)opt.chain_ws_mb << 20 : kChainWorkspace;  // (tests: small groups)
}
constexpr int kLargeParts = 1024;  // workgroups of the column statistics = partial sums of q and of the noise's log-determinant

struct LargeShape {
  int elem;        // sizeof(T): 4 | 8
  int D, N, layout, noise_kind, prior_kind;
  bool x_aligned;  // X's base (of the group's first regressor) and ldx are multiples of 16 bytes
  bool rff;        // a basis evaluated inside the planes pass, of
  int Din;         // ... this many input dimensions
  int S;           // multi-output evidence: columns of Y that ride along as one more row block; 0: an ordinary update
  int G;           // regressors asked to share the launches
};

// One regressor's workspace: byte offsets of its buffers (multiples of 256), `per` = its size = the stride to the next regressor's.
struct LargeLayout {
  size_t abar;    // augmented matrix [A; b'] (lda x DP)
  size_t w;       // dense prior: its padded copy, factored in place
  size_t xp;      // planes path: the operand planes
  size_t gp;      // split-K partial tiles (+ the prior factor's pseudo split)
  size_t bp;      // b partials, then (planes path) the rows' largest entries and the planes pass's redo flag
  size_t mu, qs;  // multi-output: x_n'mw, partial sums of q_s per column chunk
  size_t r;       // residuals
  size_t wv;      // diagonal noise: 1 / s_n (planes path: its square root) for the Gram launch
  size_t q, l;    // kLargeParts partial sums each
  size_t m;       // transposed factor for the back substitution
  size_t sc;      // scratch words: LargeScratch
  size_t per;
};
// the 64 scratch bytes at LargeLayout::sc (prior_diag_kernel clears the first 16 words); byte offsets
struct LargeScratch {
  static constexpr size_t logdet = 0;         // double: log det of the prior's factor
  static constexpr size_t info_prior = 8;     // int32 status words
  static constexpr size_t info_chol = 12;
  static constexpr size_t info_noise = 16;
  static constexpr size_t spare_info = 32;    // dense prior: what prior_diag_kernel's own look at the diagonal gives (not the answer)
  static constexpr size_t spare_logdet = 40;
};

struct LargePlan {
  // route
  bool bf3, planes, planes4, rff, x_ring;
  int NP;             // planes per operand: two fp16 (three products) or three bf16 (six)
  const char* route;  // blr_last_route's label; NULL while plan_large has not got as far as choosing it
  // dimensions
  int DP, NC, NCA, DPA;
  int64_t lda;
  int ntiles, ntiles_g, NKB, nbchunks, bslots;
  // split plan: column ranges per off-diagonal tile, per diagonal tile (0: one factor), strictly lower tiles with one range less
  int nsplit, nsplit_diag, nlong;
  LargeLayout o;
  int G;  // the group that will run
};

// (row blocks, N, slots) -> (off-diagonal ranges, diagonal ranges, tiles with one range less): blr_handle::gram_plans
using GramPlanCache = std::map<std::array<int, 3>, std::array<int, 3>>;

// Multi-round Gram launch of ONE regressor (c5: 136 tiles on 512 slots): with one split factor the launch takes whole rounds of
// the off-diagonal workgroup length (952 workgroups = 2 rounds at 93 % fill).  Three kinds of work items, dispatched longest
// first -- diagonal tiles with `sd` column ranges, `nlong` strictly lower tiles with so - 1 ranges, the others with so -- let
// a second round of SHORTER workgroups follow a first round of longer ones (c5: 64 x 3205 + 448 x 2597, then 448 x 2304 column
// units instead of 2 x 2597 everywhere).  The plan is the makespan of list scheduling on `slots` slots over a small neighbourhood
// of the one-factor choice s0 (10 ms of host time, once per shape and handle); `unit` = cost of a diagonal column / off-diagonal.
struct GramPlan { int so, sd, nlong; double makespan; };
inline double gram_makespan(int n_off, int NC, int so, int sd, int nlong, int N, int nsc, int slots, double unit, bool interleaved) {
  auto cols = [&](int sp) { return (double)(((N + sp - 1) / sp + nsc - 1) / nsc * nsc); };
  std::priority_queue<double, std::vector<double>, std::greater<double>> free_at;
  for (int i = 0; i < slots; ++i) free_at.push(0.0);
  double end = 0.0;
  auto run = [&](double cost) { double t = free_at.top() + cost; free_at.pop(); free_at.push(t); end = std::max(end, t); };
  if (interleaved) {  // one factor: item w -> tile w % ntiles, diagonal tiles spread over the launch
    const int ntiles = n_off + NC;
    for (int w = 0; w < ntiles * so; ++w) {
      const int t = w % ntiles;
      int ii = 0;
      while ((ii + 1) * (ii + 2) / 2 <= t) ++ii;
      const bool diag = t - ii * (ii + 1) / 2 == ii;
      run((diag ? unit : 1.0) * cols(so) + 256.0);
    }
    return end;
  }
  for (int i = 0; i < NC * sd; ++i) run(unit * cols(sd) + 256.0);
  for (int i = 0; i < nlong * (so - 1); ++i) run(cols(so - 1) + 256.0);
  for (int i = 0; i < (n_off - nlong) * so; ++i) run(cols(so) + 256.0);
  return end;
}
inline GramPlan plan_gram_rounds(int n_off, int NC, int s0, int N, int nsc, int slots, int max_split, double unit) {
  const double base = gram_makespan(n_off, NC, s0, s0, 0, N, nsc, slots, unit, true);
  // Candidates are the family that measured well on c5 (tools/scan_splits.sh): one or two ranges more than the one-factor choice,
  // diagonal tiles with as many ranges as the short tiles or half as many, the long tiles in sixteenths of the triangle.
  // (Measured against the model at D = 2048, N = 16384, ms per update: 7 | 7 -> 1.045; 8 | 8, 64 long -> 0.999; 8 | 4, 64 ->
  // 0.997; 8 | 6, 56 -> 0.999; 8 | 8, 56 (1032 workgroups: a third round) -> 1.065; 8 | 7, 64 -> 1.076 against a modelled tie.)
  GramPlan best{s0, 0, 0, base};
  for (int so = std::max(2, s0); so <= std::min(max_split, s0 + 2); ++so)
    for (int sd : {so, so / 2}) {
      if (sd < 1) continue;
      // the run of nlong values that tie for the best makespan of this (so, sd): take its middle (both ends sit next to a cliff)
      double m_best = 1e300;
      int first = -1, last = -1;
      for (int f = 0; f <= 16; ++f) {
        const double m = gram_makespan(n_off, NC, so, sd, n_off * f / 16, N, nsc, slots, unit, false);
        if (m < m_best * 0.995) { m_best = m; first = last = f; }
        else if (m <= m_best * 1.005 && f == last + 1) last = f;
      }
      if (m_best < best.makespan * 0.995) best = GramPlan{so, sd, n_off * ((first + last) / 2) / 16, m_best};
    }
  if (best.sd == 0 || best.makespan > 0.96 * base) return GramPlan{s0, 0, 0, base};  // not worth leaving the one-factor launch
  return best;
}

// Split plan of the tile kernels (gram_tile_kernel) for a launch that G regressors share: p.nsplit, p.nsplit_diag, p.nlong.
inline void plan_splits(const LargeShape& s, const BlrOptions& opt, int cus, GramPlanCache& cache, LargePlan& p, int G) {
  const int D = s.D, N = s.N, NC = p.NC, ntiles = p.ntiles;
  const int nstage_cols = s.elem == 4 ? LargeCfg<float>::NSC : LargeCfg<double>::NSC;
  const int max_split_cols = std::max(1, (N + nstage_cols - 1) / nstage_cols);
  const int max_split = std::min(64, max_split_cols);
  int &nsplit = p.nsplit, &nsplit_diag = p.nsplit_diag, &nlong = p.nlong;
  // split-K factor: fill the 2 x 256 workgroup slots of the chip in whole rounds (576 workgroups on 512 slots
  // would take two rounds for 1.125 rounds of work)
  // model of the launch: rounds x (columns per workgroup + 256) -- the 256 stands for a workgroup's fixed costs (pipeline fill,
  // the 64 KB partial it writes and the reduction reads back), fitted on c5 (136 tiles: 15 splits 1.232 ms, 11: 1.204, 7: 1.210)
  nsplit = 1;
  double best = 1e300;
  const int slots = cus * (s.elem == 4 ? BLR_GRAM_WGS : 2);
  for (int sp = 1; sp <= max_split; ++sp) {
    const int wgs = ntiles * sp * G;  // (the whole group's tiles are one launch)
    const int rounds = (wgs + slots - 1) / slots;
    const int cols_sp = ((N + sp - 1) / sp + nstage_cols - 1) / nstage_cols * nstage_cols;
    const double cost = (double)rounds * (cols_sp + 256.0);
    if (cost < best) { best = cost; nsplit = sp; }
  }
  // Diagonal macro tiles cost less per column than off-diagonal ones in the ring loop (only the 36 tiles of 16 x 16 on or below
  // the diagonal are computed: 10 MFMAs per k-step on the critical waves instead of 16; measured ~11.5 with the b partials
  // riding along), so in a single-round launch they get their OWN split factor: fewer, longer column ranges, and the
  // workgroup slots that frees go to the off-diagonal tiles.  Chosen so that the longest workgroup is shortest
  // (c3: 36 x 14 -> 28 x 15 + 8 x 11, i.e. 16 N / 14 -> 16 N / 15 per workgroup on 508 of 512 slots: 0.963 -> 0.935 ms;
  // tools/scan_splits.sh).  Multi-round launches (c5: 136 tiles x 15) keep one factor: there the dispatcher balances.
  // (on the bf16 matrix cores -- gram_tile_kernel<float, true> -- a diagonal tile is 18 matrix instructions and up to four operand
  // builds per half against 24 and four: the builds dominate and the tiles cost nearly the same per column; tools/scan_splits.sh at
  // c3: 15 | 11 0.80 ms, 14 | 14 0.75, 14 | 12 and 13 | 13 0.765)
  const double kDiagCost = p.bf3 ? 15.5 : 11.5;
  nsplit_diag = 0;  // 0: one factor for all tiles
  nlong = 0;        // strictly lower tiles with one column range less (multi-round launches)
  // (only where the diagonal tiles will go through the ring loop: f32, LDS-DMA staging, whole row blocks)
  const bool ring_rows = s.elem == 4 && p.x_ring && !opt.no_gram_ring && !opt.no_diag_split && D % kPB == 0 && NC >= 2;
  const bool dealt = ring_rows && (ntiles * nsplit * G <= slots || opt.gs_fields >= 2);
  if (opt.gs_fields >= 2) {  // "off-diagonal,diagonal" (equal: one factor): measurements only
    const int so = opt.gs_so, sd = opt.gs_sd, nl = opt.gs_nl, nf = opt.gs_fields;
    if (nf >= 2 && so >= 1 && sd >= 1 && sd <= so && so <= max_split) {
      nsplit = so;
      nsplit_diag = ((sd < so || nf == 3) && dealt) ? sd : 0;
      if (nf == 3 && nsplit_diag > 0 && so >= 2) nlong = std::max(0, std::min(nl, ntiles - NC));
    }
  } else if (dealt) {
    auto cols = [&](int sp) { return (double)(((N + sp - 1) / sp + nstage_cols - 1) / nstage_cols * nstage_cols); };
    const int n_off = ntiles - NC;
    double best_t = 16.0 * cols(nsplit);  // today's longest workgroup (diagonal tiles shorter, off-diagonal ones set the time)
    int bo = 0, bd = 0;
    for (int so = 1; so <= max_split; ++so)
      for (int sd = 1; sd <= so; ++sd) {
        if ((n_off * so + NC * sd) * G > slots) break;
        const double t = std::max(16.0 * cols(so), kDiagCost * cols(sd)) * (1.0 + 0.002 * so);
        if (t < best_t * 0.995) { best_t = t; bo = so; bd = sd; }
      }
    if (bo > 0) { nsplit = bo; nsplit_diag = bd; }
  }
  // multi-round launch of one regressor: three kinds of work items (plan_gram_rounds)
  const bool ring_ok = ring_rows && opt.gs_fields < 2;
  if (ring_ok && G == 1 && nsplit_diag == 0 && ntiles * nsplit > slots && nsplit >= 2) {
    const std::array<int, 3> key{NC, N, slots};
    auto it = cache.find(key);
    if (it == cache.end()) {
      const GramPlan pl = plan_gram_rounds(ntiles - NC, NC, nsplit, N, nstage_cols, slots, max_split, kDiagCost / 16.0);
      it = cache.emplace(key, std::array<int, 3>{pl.so, pl.sd, pl.nlong}).first;
      if (opt.plan_debug)
        fprintf(stderr, "blr: Gram plan for %d row blocks, N = %d: one factor %d -> ranges %d (off-diagonal, %d tiles with %d) / %d (diagonal), "
                        "modelled makespan %.0f column units\n", NC, N, nsplit, pl.so, pl.nlong, pl.so - 1, pl.sd, pl.makespan);
    }
    if (it->second[1] > 0) { nsplit = it->second[0]; nsplit_diag = it->second[1]; nlong = it->second[2]; }
  }
}

// the planes path: one 512-thread workgroup per CU, k-blocks of 16 columns, diagonal macro tiles as long as the others
inline void plan_splits_planes(const BlrOptions& opt, int cus, LargePlan& p, int G) {
  p.nsplit_diag = 0; p.nlong = 0; p.nsplit = 1;
  double best = 1e300;
  const int slots = cus * (p.planes4 ? 2 : 1);
  for (int sp = 1; sp <= std::min(64, std::max(1, p.NKB)); ++sp) {
    const int rounds = (p.ntiles_g * sp * G + slots - 1) / slots;
    const double cost = (double)rounds * (16.0 * ((p.NKB + sp - 1) / sp) + 192.0);  // (192: a workgroup's pipeline fill and its 64 KB partial tile, in columns)
    if (cost < best) { best = cost; p.nsplit = sp; }
  }
  if (opt.gs_fields >= 2 && opt.gs_so >= 1 && opt.gs_so <= 64) p.nsplit = opt.gs_so;  // (GRAM_SPLITS: measurements only)
}

// THE workspace layout of one regressor under split factor `nsplit` (+ the prior factor's pseudo split): serves the clamp of the
// group (LargeLayout::per) and the offsets the launches use.  *bslots: slots of b partials.
inline LargeLayout large_layout(const LargeShape& s, const LargePlan& p, int nsplit, int* bslots = nullptr) {
  const size_t esz = (size_t)s.elem, n1 = (size_t)std::max(s.N, 1);
  const int nsplit_total = nsplit + (s.prior_kind == PRIOR_UPPER_FACTOR ? 1 : 0);  // (nsplit_diag <= nsplit: the partials are laid out for the larger factor)
  const int nb = std::max(nsplit_total, p.nbchunks);
  if (bslots) *bslots = nb;
  Carve carve;
  LargeLayout o{};
  o.abar = carve((size_t)p.lda * p.DP * esz);
  o.w = carve(s.prior_kind == PRIOR_DENSE ? (size_t)p.DP * p.DP * esz : 0);
  o.xp = carve(p.planes ? (size_t)p.NKB * p.NCA * 4 * p.NP * 1024 : 0);
  o.gp = carve((size_t)((int64_t)nsplit_total * p.ntiles_g) * kPB * kPB * esz);
  // b partials, then (planes path) the rows' largest entries: both zeroed by the prior launch's scratch initialisation
  o.bp = carve((size_t)nb * p.NCA * kPB * sizeof(double) + (size_t)p.DPA * sizeof(unsigned) + 8);  // (+ the planes pass's redo flag)
  o.mu = carve(s.S ? n1 * esz : 0);
  o.qs = carve(s.S ? (size_t)p.nbchunks * kPB * sizeof(double) : 0);
  o.r = carve(n1 * esz);
  o.wv = carve(s.noise_kind == NOISE_DIAGONAL ? n1 * esz : 0);
  o.q = carve((size_t)kLargeParts * sizeof(double));
  o.l = carve((size_t)kLargeParts * sizeof(double));
  o.m = carve((size_t)p.DP * p.DP * esz);
  o.sc = carve(64);
  o.per = carve.off;
  return o;
}

// Plans the update of `s.G` regressors.  Returns NULL, or the message of the call's error (hipErrorInvalidValue); p.route is set
// once the route is decided, which is before the multi-output check.
inline const char* plan_large(const LargeShape& s, const BlrOptions& opt, int cus, size_t ws_cap, GramPlanCache& cache, LargePlan& p) {
  p = LargePlan{};
  p.x_ring = x_ring(s.layout, s.x_aligned);
  // fp32 Gram on the bf16 matrix cores: only where the ring loop runs (aligned ColVecs -- use_dma == 1).  RowVecs / unaligned fp32 calls
  // take the plain-f32 instantiation, its split plan and its label (they used to launch the BF3K instantiation's f32 loops,
  // 15 % slower, with a plan costed for bf16 diagonal tiles and a route that named a kernel form that never ran).
  p.bf3 = s.elem == 4 && !opt.no_bf16x3 && !opt.no_gram_ring && p.x_ring;
  // fp32, ColVecs (any alignment): the operands of the Gram product are split into their three bf16 planes ONCE, in the fragment order
  // of the matrix instruction, and the Gram launch only moves and multiplies them (blr_planes.hpp)
  p.rff = s.rff;
  p.planes = s.elem == 4 && !opt.no_bf16x3 && !opt.no_planes && s.layout == LAYOUT_COLVECS && s.N > 0;
  if (p.rff && !p.planes) return "a basis that is not materialised needs the planes path";
  if (p.rff && s.Din > kRffFusedMaxDin) return "a basis of D_in > kRffFusedMaxDin must be materialised";
  p.NP = opt.no_fp16_planes ? 3 : 2;
  p.route = s.elem == 8 ? "gram_tile_kernel<double>"
                        : (p.planes ? (p.NP == 2 ? (opt.planes8 ? "gram_planes_kernel<2>" : "gram_planes4_kernel") : "gram_planes_kernel<3>")
                                    : (p.bf3 ? "gram_tile_kernel<float, true>" : "gram_tile_kernel<float>"));  // (large-D pipeline: the Gram launch dominates; <float, true>: full tiles on the bf16 matrix cores)
  if (p.rff)  // (the basis evaluated inside the planes pass: distinguishable from the same Gram kernel on materialised features)
    p.route = p.NP == 2 ? (opt.planes8 ? "gram_planes_kernel<2> (basis in planes pass)" : "gram_planes4_kernel (basis in planes pass)")
                        : "gram_planes_kernel<3> (basis in planes pass)";
  p.DP = (s.D + kPB - 1) / kPB * kPB; p.NC = p.DP / kPB;
  p.lda = p.DP + kPB;
  p.ntiles = p.NC * (p.NC + 1) / 2;
  // multi-output evidence: one more row block of operand planes (the residuals of Y's columns), its macro tiles in the Gram launch
  if (s.S && !(p.planes && !p.rff && !opt.no_fp16_planes && s.G == 1 && s.prior_kind != PRIOR_UPPER_FACTOR && s.S >= 1 && s.S <= kPB))
    return "multi-output rows need the fp16 planes path (internal)";
  p.NCA = p.NC + (s.S ? 1 : 0); p.DPA = p.NCA * kPB;
  p.ntiles_g = p.NCA * (p.NCA + 1) / 2;
  p.planes4 = p.NP == 2 && !opt.planes8;  // 64 x 64 per wave, two 256-thread workgroups per CU (gram_planes4_kernel)
  const int kbs = p.NP == 2 ? PlanesCfg<2>::KBS : PlanesCfg<3>::KBS;
  p.NKB = ((s.N + 15) / 16 + kbs - 1) / kbs * kbs;  // k-blocks of 16 columns, padded to whole stages of the Gram launch (zero columns)
  // column chunks of the planes pass (one b partial each): ~ 2 workgroups per CU, and no chunk beyond kPlanesChunkKb k-blocks (its
  // per-column scalars live in LDS)
  p.nbchunks = p.planes ? std::max(1, std::min(p.NKB, std::max((512 + p.NC - 1) / p.NC, (p.NKB + kPlanesChunkKb - 1) / kPlanesChunkKb))) : 0;
  // The split plan depends on how many regressors share the launch -- and the workspace one regressor needs depends on the
  // plan.  Plan for the requested group first, clamp the group to the workspace bound, then plan AGAIN for the group that will
  // really run (a clamped group used to run with the split of the larger one: under-split, fewer rounds than modelled).
  auto plan = [&](int G) { if (p.planes) plan_splits_planes(opt, cus, p, G); else plan_splits(s, opt, cus, cache, p, G); };
  auto clamp = [&](int G, size_t per) { return (int)std::max<size_t>(1, std::min<size_t>((size_t)G, ws_cap / per)); };
  p.G = s.G;
  plan(p.G);
  const int Gc = clamp(p.G, large_layout(s, p, p.nsplit).per);
  if (Gc != p.G) {
    p.G = Gc;
    plan(p.G);
  }
  p.o = large_layout(s, p, p.nsplit, &p.bslots);
  p.G = clamp(p.G, p.o.per);  // (the re-planned split may need a little more per regressor)
  return nullptr;
}

}  // namespace blr
