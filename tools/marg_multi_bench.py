"""Batched multi-output marginals, timed (GPU box): python tools/marg_multi_bench.py [--quick] [--out FILE]
Times blr_marginals_multi_batched_* (S mean columns and one variance per input and regressor) with HIP events through
blr_timer_* -- one untimed call, 2 warm-up + 9 timed calls, median -- against the loop it replaces, in the same process on the
same handle: one blr_marginals_batched_* call with mean + var for column 0, plus S - 1 mean-only calls with the mw pointer stepped
by one column.  Shapes: 64 x (128, 4096) and 4096 x (128, 4096); S = 2, 8, 64; fp64 and fp32; factor prior, isotropic noise,
aligned ColVecs.  Per row also the bytes of X the call has to read at least once (algorithmic) and reads by design (once per pass
of MARG_COLS_PER_PASS columns), and what the measured time makes of them.
--quick: B = 8 and 64 instead of 64 and 4096 (a smoke run of every row).
Writes profiles/marg_multi_bench.json by default.  The numbers of DESIGN.md K18."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marg_multi_bench.json"))
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
        M = torch.randn((B, S, D), device=dev, dtype=tdt, generator=gen)  # D x S column-major per regressor
        # upper factors, column-major: [b][c][r] holds U[r, c], r <= c
        U = torch.tril(0.05 * torch.randn((B, D, D), device=dev, dtype=tdt, generator=gen), -1)
        U += torch.diag_embed(1.0 + torch.rand((B, D), device=dev, dtype=tdt, generator=gen))
        s = torch.full((B,), 0.1, device=dev, dtype=tdt)
        mean = torch.zeros((B, S, N), device=dev, dtype=tdt)
        var = torch.zeros((B, N), device=dev, dtype=tdt)
        mean_l = torch.zeros((S, B, N), device=dev, dtype=tdt)
        var_l = torch.zeros((B, N), device=dev, dtype=tdt)
        info = torch.zeros(B, device=dev, dtype=torch.int32)
        info_l = torch.zeros((S, B), device=dev, dtype=torch.int32)
        p = lambda t: t.data_ptr()  # noqa: E731

        def multi():
            h.marginals_multi_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, S, p(X), D, D * N, a.NOISE_ISOTROPIC, p(s), 1,
                                      a.PRIOR_UPPER_FACTOR, p(M), D, D * S, p(U), D, D * D, p(mean), N, N * S, p(var), N, p(info))

        def loop():  # column 0 with the variance, then S - 1 mean-only calls, each over the B regressors
            for c in range(S):
                h.marginals_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, p(X), D, D * N, a.NOISE_ISOTROPIC, p(s), 1,
                                    a.PRIOR_UPPER_FACTOR, p(M) + c * D * item, D * S, p(U), D, D * D, p(mean_l) + c * B * N * item, N,
                                    p(var_l) if c == 0 else None, N, p(info_l) + c * B * 4)

        t_multi = timed(multi)
        t_loop = timed(loop)
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0 and int(info_l.abs().sum()) == 0
        passes = -(-S // a.MARG_COLS_PER_PASS)
        x_bytes = B * D * N * item
        other = B * (D * S + D * (D + 1) // 2 + N * S + N) * item
        scale = float(mean_l.abs().max())
        r = dict(B=B, D=D, N=N, S=S, dtype=np.dtype(dtype).name, multi_ms=round(t_multi, 4), loop_ms=round(t_loop, 4),
                 speedup_vs_loop=round(t_loop / t_multi, 3), passes=passes, x_bytes_algorithmic=x_bytes, x_bytes_by_design=passes * x_bytes,
                 x_bytes_loop=S * x_bytes, other_bytes=other,
                 multi_TBps_algorithmic=round((x_bytes + other) / t_multi / 1e9, 3), loop_TBps_of_its_traffic=round((S * x_bytes + other) / t_loop / 1e9, 3),
                 max_abs_diff_mean_over_scale=float((mean - mean_l.transpose(0, 1)).abs().max()) / scale,
                 max_rel_diff_var=float(((var - var_l).abs() / var_l.abs()).max()))
        print(json.dumps(r), flush=True)
        del X, M, U, mean, mean_l
        torch.cuda.empty_cache()
        return r

    sizes = (8, 64) if args.quick else (64, 4096)
    rows = [row(B, 128, 4096, S, dt) for dt in (np.float64, np.float32) for B in sizes for S in (2, 8, 64)]
    res = dict(tool="tools/marg_multi_bench.py" + (" --quick" if args.quick else ""), warmup=WARMUP, reps=REPS,
               timer="HIP events (blr_timer_*), median, after one untimed call", cols_per_pass=a.MARG_COLS_PER_PASS, rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
