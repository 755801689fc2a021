"""Batched predictive covariance, timed (GPU box): python tools/cov_batched_bench.py [--quick] [--out FILE]
Times blr_mean_and_cov_batched_* (mean and the full N x N covariance of B regressors in one call) with HIP events through
blr_timer_* -- one untimed call, 2 warm-up + 9 timed calls, median -- in the same process on the same handle against the loop it
replaces: B blr_mean_and_cov_* calls on the same data (device memspace; every one of them drains the stream and allocates and frees
its temporaries, which is part of what the loop costs; 1 warm-up + 3 timed rounds of the loop, median).
Shapes: B = 64 and 4096 regressors x (D = 128, N = 16, 64, 256); fp64 and fp32; one candidate set shared by all regressors
(strideX = 0) and one per regressor; factor priors, isotropic noise, ColVecs.
--quick: B = 8 and 64 instead of 64 and 4096 (a smoke run of every row).
Writes profiles/cov_batched_bench.json by default.  The numbers of DESIGN.md K21."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WARMUP, REPS = 2, 9
LOOP_WARMUP, LOOP_REPS = 1, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_batched_bench.json"))
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn, warmup, reps):
        fn()  # untimed: workspace allocation, LDS limits
        torch.cuda.synchronize()
        ts = []
        for _ in range(warmup + reps):
            h.timer_start()
            fn()
            ts.append(h.timer_stop())
        return float(np.median(ts[warmup:]))

    def row(B, D, N, dtype, shared):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        item = 8 if dtype == np.float64 else 4
        gen = torch.Generator(device=dev).manual_seed(4321)
        nx = 1 if shared else B
        X = torch.randn((nx, N, D), device=dev, dtype=tdt, generator=gen)  # ColVecs: D x N column-major per regressor
        mw = torch.randn((B, D), device=dev, dtype=tdt, generator=gen)
        # upper factors, column-major: [b][c][r] holds U[r, c], r <= c
        U = torch.tril(0.05 * torch.randn((B, D, D), device=dev, dtype=tdt, generator=gen), -1)
        U += torch.diag_embed(1.0 + torch.rand((B, D), device=dev, dtype=tdt, generator=gen))
        s = torch.full((B,), 0.5, device=dev, dtype=tdt)
        m = torch.zeros((B, N), device=dev, dtype=tdt)
        C = torch.zeros((B, N, N), device=dev, dtype=tdt)
        m_l = torch.zeros((B, N), device=dev, dtype=tdt)
        C_l = torch.zeros((B, N, N), device=dev, dtype=tdt)
        info = torch.zeros(B, device=dev, dtype=torch.int32)
        info_l = torch.zeros(B, device=dev, dtype=torch.int32)
        p = lambda t: t.data_ptr()  # noqa: E731
        strideX = 0 if shared else D * N

        def batched():
            h.mean_and_cov_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, p(X), D, strideX, a.NOISE_ISOTROPIC, p(s), N, 1,
                                   a.PRIOR_UPPER_FACTOR, p(mw), D, p(U), D, D * D, p(m), N, p(C), N, N * N, p(info))

        def loop():  # one blr_mean_and_cov_* call per regressor
            for b in range(B):
                h.mean_and_cov(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, D, N, p(X) + b * strideX * item, D, a.NOISE_ISOTROPIC, p(s) + b * item, N,
                               a.PRIOR_UPPER_FACTOR, p(mw) + b * D * item, p(U) + b * D * D * item, D, p(m_l) + b * N * item,
                               p(C_l) + b * N * N * item, N, p(info_l) + b * 4)

        t_batched = timed(batched, WARMUP, REPS)
        chunks = h.get_stat("last_chunks")
        t_loop = timed(loop, LOOP_WARMUP, LOOP_REPS)
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0 and int(info_l.abs().sum()) == 0
        assert bool(torch.equal(C, C.transpose(1, 2)))
        diffs = dict(max_rel_diff_cov=float((C - C_l).abs().max()) / float(C_l.abs().max()),
                     max_rel_diff_mean=float((m - m_l).abs().max()) / float(m_l.abs().max()))
        in_bytes = (nx * D * N + B * (D + D * (D + 1) // 2)) * item
        out_bytes = B * (N * N + N) * item
        r = dict(B=B, D=D, N=N, dtype=np.dtype(dtype).name, shared_x=bool(shared), batched_ms=round(t_batched, 4), loop_ms=round(t_loop, 4),
                 speedup_vs_loop=round(t_loop / t_batched, 3), chunks=chunks, in_bytes=in_bytes, out_bytes=out_bytes,
                 batched_TBps_algorithmic=round((in_bytes + out_bytes) / t_batched / 1e9, 3),
                 batched_TFLOPs=round(B * (D * D * N + N * N * D) / t_batched / 1e9, 3), **diffs)
        print(json.dumps(r), flush=True)
        del X, U, C, C_l
        torch.cuda.empty_cache()
        return r

    sizes = (8, 64) if args.quick else (64, 4096)
    rows = [row(B, 128, N, dt, shared) for dt in (np.float64, np.float32) for B in sizes for N in (16, 64, 256) for shared in (True, False)]
    res = dict(tool="tools/cov_batched_bench.py" + (" --quick" if args.quick else ""), warmup=WARMUP, reps=REPS, loop_warmup=LOOP_WARMUP,
               loop_reps=LOOP_REPS, timer="HIP events (blr_timer_*), median, after one untimed call", rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
