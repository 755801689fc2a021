"""Exact leave-one-out of multi-output states, timed (GPU box): python tools/loo_multi_bench.py [--quick] [--out FILE]
Times blr_loo_multi_batched_* (S means and log densities and one variance per input, S totals per regressor) with HIP events
through blr_timer_* -- one untimed call, 2 warm-up + 9 timed calls, median -- in the same process on the same handle against
  baseline 1: the loop it replaces, S blr_loo_batched_* calls on the same state (mw pointer stepped by one column of M, y by one
              column of Y, every call with all four outputs);
  baseline 2: blr_marginals_multi_batched_* mean + var at the same S, the stream the new kernel extends (no Y, no epilogue).
Shapes: 64 x (128, 4096) and 2048 x (128, 4096); S = 2, 8, 64; fp64 and fp32; isotropic noise, aligned ColVecs.  The noise
variance is large enough that no leverage is degenerate (every input takes the full epilogue).
--quick: B = 8 and 64 instead of 64 and 2048 (a smoke run of every row).
Writes profiles/loo_multi_bench.json by default.  The numbers of DESIGN.md K20."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WARMUP, REPS = 2, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_multi_bench.json"))
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn):
        fn()  # untimed: workspace allocation, LDS limits
        torch.cuda.synchronize()
        ts = []
        for _ in range(WARMUP + REPS):
            h.timer_start()
            fn()
            ts.append(h.timer_stop())
        return float(np.median(ts[WARMUP:]))

    def row(B, D, N, S, dtype):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        item = 8 if dtype == np.float64 else 4
        gen = torch.Generator(device=dev).manual_seed(4321)
        X = torch.randn((B, N, D), device=dev, dtype=tdt, generator=gen)  # ColVecs: D x N column-major per regressor
        Y = torch.randn((B, S, N), device=dev, dtype=tdt, generator=gen)  # N x S column-major per regressor
        M = torch.randn((B, S, D), device=dev, dtype=tdt, generator=gen) / D ** 0.5  # D x S column-major per regressor
        # upper factors, column-major: [b][c][r] holds U[r, c], r <= c
        U = torch.tril(0.05 * torch.randn((B, D, D), device=dev, dtype=tdt, generator=gen), -1)
        U += torch.diag_embed(1.0 + torch.rand((B, D), device=dev, dtype=tdt, generator=gen))
        s = torch.full((B,), 1.0e3, device=dev, dtype=tdt)  # sigma2_n is about D / 2: 1 - h_n stays near 0.94
        lm = torch.zeros((B, S, N), device=dev, dtype=tdt)
        lv = torch.zeros((B, N), device=dev, dtype=tdt)
        ll = torch.zeros((B, S, N), device=dev, dtype=torch.float64)
        tot = torch.zeros((B, S), device=dev, dtype=torch.float64)
        lm_l = torch.zeros((B, S, N), device=dev, dtype=tdt)
        lv_l = torch.zeros((B, N), device=dev, dtype=tdt)
        ll_l = torch.zeros((B, S, N), device=dev, dtype=torch.float64)
        tot_l = torch.zeros((S, B), device=dev, dtype=torch.float64)
        info = torch.zeros(B, device=dev, dtype=torch.int32)
        info_l = torch.zeros((S, B), device=dev, dtype=torch.int32)
        p = lambda t: t.data_ptr()  # noqa: E731

        def multi():
            h.loo_multi_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, S, p(X), D, D * N, p(Y), N, N * S, a.NOISE_ISOTROPIC, p(s), 1,
                                p(M), D, D * S, p(U), D, D * D, p(lm), N, N * S, p(lv), N, p(ll), N, N * S, p(tot), S, p(info))

        def loop():  # one blr_loo_batched_* call per column, each over the B regressors
            for c in range(S):
                h.loo(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, p(X), D, D * N, p(Y) + c * N * item, N * S, a.NOISE_ISOTROPIC, p(s), 1,
                      p(M) + c * D * item, D * S, p(U), D, D * D, p(lm_l) + c * N * item, N * S, p(lv_l), N, p(ll_l) + c * N * 8, N * S,
                      p(tot_l) + c * B * 8, p(info_l) + c * B * 4)

        t_multi = timed(multi)
        t_loop = timed(loop)
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0 and int(info_l.abs().sum()) == 0
        assert bool(torch.isfinite(ll).all()) and bool(torch.isfinite(tot).all())
        diffs = dict(max_abs_diff_mean_over_scale=float((lm - lm_l).abs().max()) / float(lm_l.abs().max()),
                     max_rel_diff_var=float(((lv - lv_l).abs() / lv_l.abs()).max()),
                     max_abs_diff_logpdf=float((ll - ll_l).abs().max()),
                     max_rel_diff_total=float(((tot - tot_l.transpose(0, 1)).abs() / tot_l.transpose(0, 1).abs()).max()))

        def marg():  # (the means go into the loop's buffer: compared above already)
            h.marginals_multi_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, S, p(X), D, D * N, a.NOISE_ISOTROPIC, p(s), 1,
                                      a.PRIOR_UPPER_FACTOR, p(M), D, D * S, p(U), D, D * D, p(lm_l), N, N * S, p(lv_l), N, p(info))

        t_marg = timed(marg)
        torch.cuda.synchronize()
        x_bytes = B * D * N * item
        out_bytes = B * (N * S * (2 * item + 8) + N * item + S * 8)  # Y in, means and log densities out; var; totals
        other = B * (D * S + D * (D + 1) // 2) * item + out_bytes
        r = dict(B=B, D=D, N=N, S=S, dtype=np.dtype(dtype).name, multi_ms=round(t_multi, 4), loop_ms=round(t_loop, 4),
                 marginals_multi_ms=round(t_marg, 4), speedup_vs_loop=round(t_loop / t_multi, 3),
                 time_over_marginals_multi=round(t_multi / t_marg, 3), passes=-(-S // a.LOO_COLS_PER_PASS), x_bytes=x_bytes,
                 x_bytes_loop=S * x_bytes, other_bytes=other, multi_TBps_algorithmic=round((x_bytes + other) / t_multi / 1e9, 3), **diffs)
        print(json.dumps(r), flush=True)
        del X, Y, M, U, lm, ll, lm_l, ll_l
        torch.cuda.empty_cache()
        return r

    sizes = (8, 64) if args.quick else (64, 2048)
    rows = [row(B, 128, 4096, S, dt) for dt in (np.float64, np.float32) for B in sizes for S in (2, 8, 64)]
    res = dict(tool="tools/loo_multi_bench.py" + (" --quick" if args.quick else ""), warmup=WARMUP, reps=REPS,
               timer="HIP events (blr_timer_*), median, after one untimed call", cols_per_pass=a.LOO_COLS_PER_PASS, rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
