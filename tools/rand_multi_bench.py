"""Multi-output draws, timed (GPU box): python tools/rand_multi_bench.py [--quick] [--out FILE]
Times blr_rand_multi_batched_* (R draws from each of the S column posteriors of B regressors, one shared factor per regressor) with
HIP events through blr_timer_* -- one untimed call, 2 warm-up + 9 timed calls, median -- against the loop it replaces, in the same
process on the same handle and the same operands: S calls of blr_rand_batched_* with the mw pointer stepped by one column and Z1 / Z2
/ Y stepped by R columns.  Device memspace, factor prior, aligned ColVecs, weights not returned; fp64 and fp32.  Shapes:
  thompson  B = 4096, D = 128, ONE shared set of N = 16 candidates, R = 1, S = 2, 8, 64, noise-free function values;
  long-N    B = 256, D = 128, N = 4096 per regressor, S = 8, R = 2, isotropic noise.
Per row also the largest difference between the two results over the largest value (the routes differ in rounding only).
--quick: B = 64 and 8 instead of 4096 and 256 (a smoke run of every row).
Writes profiles/rand_multi_bench.json by default.  The numbers of DESIGN.md K22; a row where the loop wins is reported as a miss."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WARMUP, REPS = 2, 9
COLS_PER_PASS = 16  # csrc/blr_rand_multi.hpp kRandColsPerPass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rand_multi_bench.json"))
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

    def row(shape, B, D, N, S, R, dtype, shared_x, noisy):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        item = 8 if dtype == np.float64 else 4
        SR = S * R
        gen = torch.Generator(device=dev).manual_seed(4321)
        X = torch.randn((1 if shared_x else B, N, D), device=dev, dtype=tdt, generator=gen) / D ** 0.5  # ColVecs: D x N column-major
        M = torch.randn((B, S, D), device=dev, dtype=tdt, generator=gen)  # D x S column-major per regressor
        # upper factors, column-major: [b][c][r] holds U[r, c], r <= c
        U = torch.tril(0.05 * torch.randn((B, D, D), device=dev, dtype=tdt, generator=gen), -1)
        U += torch.diag_embed(1.0 + torch.rand((B, D), device=dev, dtype=tdt, generator=gen))
        s = torch.full((B,), 0.1, device=dev, dtype=tdt)
        Z1 = torch.randn((B, SR, D), device=dev, dtype=tdt, generator=gen)
        Z2 = torch.randn((B, SR, N), device=dev, dtype=tdt, generator=gen) if noisy else None
        Y = torch.zeros((B, SR, N), device=dev, dtype=tdt)
        Y_l = torch.zeros((B, SR, N), device=dev, dtype=tdt)
        info = torch.zeros(B, device=dev, dtype=torch.int32)
        info_l = torch.zeros((S, B), device=dev, dtype=torch.int32)
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        sX = 0 if shared_x else D * N

        def multi():
            h.rand_multi_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, S, R, p(X), D, sX, a.NOISE_ISOTROPIC, p(s) if noisy else None, 1,
                                 a.PRIOR_UPPER_FACTOR, p(M), D, D * S, p(U), D, D * D, p(Z1), D, D * SR, p(Z2), N, N * SR, None, D, D * SR,
                                 p(Y), N, N * SR, p(info))

        def loop():  # column c: R draws per regressor with mw = M[:, c]
            for c in range(S):
                h.rand_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, R, p(X), D, sX, a.NOISE_ISOTROPIC, p(s) if noisy else None, 1,
                               a.PRIOR_UPPER_FACTOR, p(M) + c * D * item, D * S, p(U), D, D * D, p(Z1) + c * R * D * item, D, D * SR,
                               p(Z2) + c * R * N * item if noisy else None, N, N * SR, None, D, D * SR, p(Y_l) + c * R * N * item, N, N * SR,
                               p(info_l) + c * B * 4)

        t_multi = timed(multi)
        chunks = h.get_stat("last_chunks")
        t_loop = timed(loop)
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0 and int(info_l.abs().sum()) == 0
        scale = float(Y_l.abs().max())
        assert scale > 0.0 and float(Y.abs().max()) > 0.0
        x_bytes = (1 if shared_x else B) * D * N * item
        r = dict(shape=shape, B=B, D=D, N=N, S=S, R=R, dtype=np.dtype(dtype).name, shared_x=shared_x, noisy=noisy, multi_ms=round(t_multi, 4),
                 loop_ms=round(t_loop, 4), speedup_vs_loop=round(t_loop / t_multi, 3), miss=bool(t_multi > t_loop), chunks=int(chunks),
                 passes=-(-SR // COLS_PER_PASS), x_bytes=x_bytes, factor_bytes=B * D * (D + 1) // 2 * item,
                 normals_and_outputs_bytes=B * SR * (D + N * (2 if noisy else 1)) * item,
                 max_abs_diff_over_scale=float((Y - Y_l).abs().max()) / scale)
        print(json.dumps(r), flush=True)
        del X, M, U, Z1, Z2, Y, Y_l
        torch.cuda.empty_cache()
        return r

    Bt, Bl = (64, 8) if args.quick else (4096, 256)
    rows = []
    for dt in (np.float64, np.float32):
        rows += [row("thompson", Bt, 128, 16, S, 1, dt, True, False) for S in (2, 8, 64)]
        rows.append(row("long-N", Bl, 128, 4096, 8, 2, dt, False, True))
    res = dict(tool="tools/rand_multi_bench.py" + (" --quick" if args.quick else ""), warmup=WARMUP, reps=REPS,
               timer="HIP events (blr_timer_*), median, after one untimed call", cols_per_pass=COLS_PER_PASS, rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
