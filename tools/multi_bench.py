"""Batched multi-output posterior, timed (GPU box): python tools/multi_bench.py [--quick] [--out FILE]
Times blr_posterior_multi_batched_* (means and evidences of S target columns per regressor, one factor per regressor) with HIP
events -- one untimed pre-heat call, 3 warm-up + 15 timed calls, median -- against the ways to the same numbers without it, in the
same process on the same (default) handle:
  (a) 4096 x (128, 4096) fp64, S = 8 and S = 2: a loop of S blr_posterior_batched_f64 calls, the y pointer stepped by one column;
  (b) 8192 x (64, 1024) fp64, S = 8: the same loop;
  (c) row (a) in fp32;
  (d) 1 x (128, 4096) fp64, S = 64: blr_posterior_batched_f64 with strideX = 0 over the S columns (what logpdf_columns does at
      D <= 128), and blr_logpdf_multi_f64.
--quick: B = 64 instead of 4096 / 8192 (a smoke run of every row).
Writes profiles/multi_bench.json by default.  The numbers of DESIGN.md K17."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WARMUP, REPS = 3, 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_bench.json"))
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn):
        fn()  # pre-heat: workspace allocation, LDS limits
        torch.cuda.synchronize()
        ts = []
        for _ in range(WARMUP + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts[WARMUP:]))

    def row(name, B, D, N, S, dtype):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        item = 8 if dtype == np.float64 else 4
        gen = torch.Generator(device=dev).manual_seed(1234)
        X = torch.randn((B, N, D), device=dev, dtype=tdt, generator=gen)  # ColVecs: D x N column-major per regressor
        W = torch.randn((B, D, S), device=dev, dtype=tdt, generator=gen)
        Y = ((X @ W) + (0.1 ** 0.5) * torch.randn((B, N, S), device=dev, dtype=tdt, generator=gen)).transpose(1, 2).contiguous()  # N x S column-major
        del W
        s = torch.full((B,), 0.1, device=dev, dtype=tdt)
        mw = torch.zeros((B, D), device=dev, dtype=tdt)
        Lw = torch.exp(0.3 * torch.randn((B, D), device=dev, dtype=tdt, generator=gen))
        M = torch.zeros((B, S, D), device=dev, dtype=tdt)
        Mb = torch.zeros((B, S, D), device=dev, dtype=tdt)
        lp = torch.zeros((B, S), device=dev, dtype=torch.float64)
        lp_b = torch.zeros((S, B), device=dev, dtype=torch.float64)
        info = torch.zeros(B, device=dev, dtype=torch.int32)
        info_b = torch.zeros((S, B), device=dev, dtype=torch.int32)
        p = lambda t: t.data_ptr()  # noqa: E731

        def multi():
            h.posterior_multi_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, S, p(X), D, D * N, p(Y), N, N * S, a.NOISE_ISOTROPIC,
                                      p(s), 1, a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, p(M), D, D * S, None, D, D * D, None, D, D * D,
                                      p(lp), S, p(info))

        def loop():  # S calls, one per column, each over the B regressors
            for c in range(S):
                h.posterior_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, p(X), D, D * N, p(Y) + c * N * item, N * S,
                                    a.NOISE_ISOTROPIC, p(s), 1, a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, p(Mb) + c * D * item, D * S, None, D,
                                    D * D, None, D, D * D, p(lp_b) + c * B * 8, p(info_b) + c * B * 4)

        t_multi = timed(multi)
        route = h.last_route()
        t_loop = timed(loop)
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0 and int(info_b.abs().sum()) == 0
        r = dict(row=name, B=B, D=D, N=N, S=S, dtype=np.dtype(dtype).name, column0_route=route, multi_ms=round(t_multi, 4),
                 loop_ms=round(t_loop, 4), speedup_vs_loop=round(t_loop / t_multi, 3),
                 max_rel_diff_evidence=float(((lp - lp_b.T).abs() / lp_b.T.abs()).max()),
                 max_abs_diff_mean=float((M - Mb).abs().max()))
        if B == 1:  # the two single-data-set routes
            lp_s = torch.zeros(S, device=dev, dtype=torch.float64)
            info_s = torch.zeros(S, device=dev, dtype=torch.int32)

            def shared_x():
                h.posterior_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, S, D, N, p(X), D, 0, p(Y), N, a.NOISE_ISOTROPIC, p(s), 0,
                                    a.PRIOR_DIAGONAL, p(mw), 0, p(Lw), 1, 0, None, D, None, D, D * D, None, D, D * D, p(lp_s), p(info_s))

            def logpdf_multi():
                h.logpdf_multi(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, D, N, S, p(X), D, p(Y), N, a.NOISE_ISOTROPIC, p(s), a.PRIOR_DIAGONAL,
                               p(mw), p(Lw), 1, p(lp_s), None, D, p(info_s))

            r["stride0_batched_ms"] = round(timed(shared_x), 4)
            r["logpdf_multi_ms"] = round(timed(logpdf_multi), 4)
            r["speedup_vs_stride0"] = round(r["stride0_batched_ms"] / t_multi, 3)
            r["speedup_vs_logpdf_multi"] = round(r["logpdf_multi_ms"] / t_multi, 3)
        print(json.dumps(r), flush=True)
        del X, Y
        torch.cuda.empty_cache()
        return r

    big, big_c = (64, 64) if args.quick else (4096, 8192)
    rows = [row("a", big, 128, 4096, 8, np.float64), row("a", big, 128, 4096, 2, np.float64), row("b", big_c, 64, 1024, 8, np.float64),
            row("c", big, 128, 4096, 8, np.float32), row("c", big, 128, 4096, 2, np.float32), row("d", 1, 128, 4096, 64, np.float64)]
    res = dict(tool="tools/multi_bench.py" + (" --quick" if args.quick else ""), warmup=WARMUP, reps=REPS,
               timer="HIP events, median, after one untimed call", rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
