"""The evidence grid over data sets of unequal lengths, timed (GPU box): python tools/grid_ragged_bench.py [--out FILE]
Times blr_logpdf_grid_ragged_* (evidence of every setting, argmax, posterior at the winner) with HIP events -- 3 warm-up + 15 timed
calls, median -- against its yardsticks in the same process.  4096 regressors, G = 16, (D = 128, fp64) and (D = 64, fp32), isotropic
noise (one variance per regressor), diagonal prior, everything device resident:
  (a) equal counts of 4096 against blr_logpdf_grid_* on the same data (about parity is expected);
  (b) counts log-uniform in [64, 16384] against the loop of 4096 calls of blr_logpdf_grid_* with B = 1 and against G calls of
      blr_posterior_ragged_* on scaled operands (the evidence only: that route has no argmax and no refit; its evidence is
      compared to rounding, not bit for bit);
  (c) one regressor of 2^20 observations among 4095 of 256, against the same loop.
Every row's outputs are compared bit for bit with its blr_logpdf_grid_* yardstick.  Writes profiles/grid_ragged_bench.json by
default.  The numbers of DESIGN.md K30."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS = 3, 15
B, G = 4096, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grid_ragged_bench.json"))
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn):
        ts = []
        for _ in range(WARMUP + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts[WARMUP:]))

    def row(name, counts, D, dtype, equal):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        item = 8 if dtype == np.float64 else 4
        offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        total = int(offsets[-1])
        gen = torch.Generator(device=dev).manual_seed(1234)
        X = torch.randn((total, D), device=dev, dtype=tdt, generator=gen)  # ColVecs: D x total column-major, the slices side by side
        y = torch.randn((total,), device=dev, dtype=tdt, generator=gen)
        s = torch.full((B,), 0.1, device=dev, dtype=tdt)
        mw = torch.zeros((B, D), device=dev, dtype=tdt)
        Lw = torch.exp(0.3 * torch.randn((B, D), device=dev, dtype=tdt, generator=gen))
        sc = 10.0 ** np.linspace(-2, 2, 4)
        alpha = torch.tensor(np.repeat(sc, 4), device=dev, dtype=tdt)
        tau = torch.tensor(np.tile(sc, 4), device=dev, dtype=tdt)

        def outputs():
            return (torch.zeros((B, G), device=dev, dtype=torch.float64), torch.zeros((B, G), device=dev, dtype=torch.int32),
                    torch.zeros(B, device=dev, dtype=torch.int64), torch.zeros((B, D), device=dev, dtype=tdt),
                    torch.zeros((B, D, D), device=dev, dtype=tdt))

        p = lambda t: t.data_ptr()  # noqa: E731
        lp, info, best, mwb, Tb = outputs()
        lp1, info1, best1, mwb1, Tb1 = outputs()

        def ragged():
            h.logpdf_grid_ragged(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, offsets, p(X), D, p(y), a.NOISE_ISOTROPIC, p(s), 1,
                                 a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, G, p(alpha), 0, p(tau), 0, p(lp), G, p(best), p(mwb), D, p(Tb), D,
                                 D * D, p(info), G)

        def batched():  # equal counts only: the equal-count entry point on the same data
            N = int(counts[0])
            h.logpdf_grid(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, p(X), D, D * N, p(y), N, a.NOISE_ISOTROPIC, p(s), 1,
                          a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, G, p(alpha), 0, p(tau), 0, p(lp1), G, p(best1), p(mwb1), D, p(Tb1), D,
                          D * D, p(info1), G)

        def loop():  # B calls with B = 1, each on its slice
            for b in range(B):
                o, n = int(offsets[b]), int(counts[b])
                h.logpdf_grid(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, 1, D, n, p(X) + o * D * item, D, 0, p(y) + o * item, 0,
                              a.NOISE_ISOTROPIC, p(s) + b * item, 0, a.PRIOR_DIAGONAL, p(mw) + b * D * item, 0, p(Lw) + b * D * item, 1, 0,
                              G, p(alpha), 0, p(tau), 0, p(lp1) + b * G * 8, G, p(best1) + b * 8, p(mwb1) + b * D * item, D,
                              p(Tb1) + b * D * D * item, D, D * D, p(info1) + b * G * 4, G)

        # the operands of the scaled route, prepared outside the timed region: s_g = tau_g s, Lw_g = alpha_g Lw
        s_g = (tau[:, None] * s[None, :]).contiguous()        # [G, B]
        L_g = (alpha[:, None, None] * Lw[None]).contiguous()  # [G, B, D]
        lp_g = torch.zeros((G, B), device=dev, dtype=torch.float64)
        info_g = torch.zeros((G, B), device=dev, dtype=torch.int32)

        def scaled():  # G calls of blr_posterior_ragged_*, one per setting (evidence only)
            for g in range(G):
                h.posterior_ragged(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, offsets, p(X), D, p(y), a.NOISE_ISOTROPIC,
                                   p(s_g) + g * B * item, 1, a.PRIOR_DIAGONAL, p(mw), D, p(L_g) + g * B * D * item, 1, D, None, D, None, D,
                                   D * D, None, D, D * D, p(lp_g) + g * B * 8, p(info_g) + g * B * 4)

        r = dict(row=name, B=B, G=G, D=D, dtype=np.dtype(dtype).name, observations=total, longest=int(max(counts)), shortest=int(min(counts)))
        r["ragged_ms"] = round(timed(ragged), 4)
        r["route"] = h.last_route()
        if equal:
            r["grid_batched_ms"] = round(timed(batched), 4)
            r["ragged_over_batched"] = round(r["ragged_ms"] / r["grid_batched_ms"], 3)
        else:
            r["loop_of_single_calls_ms"] = round(timed(loop), 4)
            r["speedup_over_loop"] = round(r["loop_of_single_calls_ms"] / r["ragged_ms"], 3)
            if name == "b":
                r["scaled_posterior_ragged_ms"] = round(timed(scaled), 4)
                r["speedup_over_scaled"] = round(r["scaled_posterior_ragged_ms"] / r["ragged_ms"], 3)
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0 and int(info1.abs().sum()) == 0
        # against blr_logpdf_grid_* (batched in (a), the loop of single calls in (b) and (c)): evidence, argmax and refit, bit for bit
        r["same_bits_as_grid_yardstick"] = bool(torch.equal(lp, lp1) and torch.equal(best, best1) and torch.equal(mwb, mwb1) and torch.equal(Tb, Tb1))
        if "scaled_posterior_ragged_ms" in r:  # another algorithm (the Gram matrix of the scaled operands): the evidence to rounding
            assert int(info_g.abs().sum()) == 0
            r["max_rel_diff_evidence_vs_scaled"] = float(((lp - lp_g.T).abs() / lp_g.T.abs()).max())
        print(json.dumps(r), flush=True)
        del X
        torch.cuda.empty_cache()
        return r

    rng = np.random.Generator(np.random.PCG64(2024))
    shapes = {
        "a": (np.full(B, 4096, dtype=np.int64), True),
        "b": (np.floor(np.exp(rng.uniform(np.log(64.0), np.log(16384.0), size=B))).astype(np.int64), False),
        "c": (np.concatenate(([1 << 20], np.full(B - 1, 256))).astype(np.int64)[rng.permutation(B)], False),
    }
    rows = []
    for D, dtype in ((128, np.float64), (64, np.float32)):
        for name, (counts, equal) in shapes.items():
            rows.append(row(name, counts, D, dtype, equal))
    res = dict(tool="tools/grid_ragged_bench.py", warmup=WARMUP, reps=REPS, timer="HIP events, median", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
