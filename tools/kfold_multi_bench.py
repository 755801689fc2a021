"""K-fold predictives of multi-output states, timed (GPU box): python tools/kfold_multi_bench.py [--quick] [--out FILE]
Times blr_kfold_multi_batched_* with HIP events (median of the timed repeats after warm-up) against what it replaces, in the same
process and on the same resident data: a loop of S blr_kfold_batched_* calls, one per column (M[:, c], Y[:, c]), all four outputs in
both.  Resident states at B in {2048, 64} x (D, N) = (128, 4096), F in {8, 64}, S in {2, 8, 64}, fp64 and fp32.  The loop is timed
with fewer repeats than the call (it is up to S times as long).  Every row where the one call is slower than the loop is printed as
a MISS.  --quick: B = 64 only.  The numbers of DESIGN.md K25."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS, LOOP_WARMUP, LOOP_REPS = 3, 11, 1, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn, warmup=WARMUP, reps=REPS):
        ts = []
        for r in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    out, misses = [], []

    def shape(nb, D, N, S, ndt):
        dt = torch.float64 if ndt == np.float64 else torch.float32
        name = np.dtype(ndt).name
        g = torch.Generator(device=dev).manual_seed(1)
        X = torch.randn((nb, N, D), generator=g, dtype=dt, device=dev) * (1.0 / np.sqrt(D))  # ColVecs, ldx = D
        Y = torch.randn((nb, S, N), generator=g, dtype=dt, device=dev)                      # N x S column-major, ldY = N
        s = torch.full((1,), 0.5, dtype=dt, device=dev)
        Lw = torch.ones((nb, D), dtype=dt, device=dev)
        m0 = torch.zeros((nb, D), dtype=dt, device=dev)
        M, T = torch.empty((nb, S, D), dtype=dt, device=dev), torch.empty((nb, D, D), dtype=dt, device=dev)
        info = torch.zeros(nb, dtype=torch.int32, device=dev)
        es = X.element_size()
        h.posterior_multi_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, S, X.data_ptr(), D, N * D, Y.data_ptr(), N, N * S,
                                  a.NOISE_ISOTROPIC, s.data_ptr(), 0, a.PRIOR_DIAGONAL, m0.data_ptr(), D, Lw.data_ptr(), 1, D, M.data_ptr(), D,
                                  D * S, T.data_ptr(), D, D * D, None, D, D * D, None, S, info.data_ptr())
        torch.cuda.synchronize()
        assert not info.any().item()
        km, kv = torch.empty((nb, S, N), dtype=dt, device=dev), torch.empty((nb, N), dtype=dt, device=dev)
        km1, kv1 = torch.empty_like(km), torch.empty_like(kv)
        for F in (8, 64):
            nf = -(-N // F)
            kl, tot = torch.empty((nb, S, nf), dtype=torch.float64, device=dev), torch.empty((nb, S), dtype=torch.float64, device=dev)
            kl1, tot1 = torch.empty_like(kl), torch.empty((S, nb), dtype=torch.float64, device=dev)

            def multi():
                h.kfold_multi_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, S, F, X.data_ptr(), D, N * D, Y.data_ptr(), N, N * S,
                                      a.NOISE_ISOTROPIC, s.data_ptr(), 0, M.data_ptr(), D, D * S, T.data_ptr(), D, D * D, km.data_ptr(), N,
                                      N * S, kv.data_ptr(), N, kl.data_ptr(), nf, nf * S, tot.data_ptr(), S, info.data_ptr())

            def loop():  # existing code: one single-column call per column
                for c in range(S):
                    h.kfold(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, F, X.data_ptr(), D, N * D, Y.data_ptr() + c * N * es, N * S,
                            a.NOISE_ISOTROPIC, s.data_ptr(), 0, M.data_ptr() + c * D * es, D * S, T.data_ptr(), D, D * D,
                            km1.data_ptr() + c * N * es, N * S, kv1.data_ptr(), N, kl1.data_ptr() + c * nf * 8, nf * S,
                            tot1.data_ptr() + c * nb * 8, info.data_ptr())

            t_multi = timed(multi)
            chunks = h.get_stat("last_chunks")
            t_loop = timed(loop, LOOP_WARMUP, LOOP_REPS)
            torch.cuda.synchronize()
            scale = float(kl1.abs().max().item())
            row = dict(dtype=name, B=nb, D=D, N=N, F=F, S=S, folds=nf, kfold_multi_ms=round(t_multi, 4), loop_of_S_kfold_ms=round(t_loop, 4),
                       speedup_over_loop=round(t_loop / t_multi, 3), chunks=chunks, degenerate_folds=int(torch.isnan(kl[:, 0]).sum().item()),
                       max_logpdf_diff_rel=float((kl - kl1).abs().max().item()) / scale)
            print(json.dumps(row), flush=True)
            out.append(row)
            if t_multi > t_loop:
                line = (f"MISS: {name} B={nb} F={F} S={S}: the one call at {row['kfold_multi_ms']} ms is slower than the loop of {S} "
                        f"blr_kfold_batched_* calls at {row['loop_of_S_kfold_ms']} ms (x {round(t_multi / t_loop, 3)})")
                print(line, flush=True)
                misses.append(line)
            del kl, tot, kl1, tot1
        del X, Y, M, T, km, kv, km1, kv1
        torch.cuda.empty_cache()

    for ndt in (np.float64, np.float32):
        for nb in ((64,) if args.quick else (2048, 64)):
            for S in (2, 8, 64):
                shape(nb, 128, 4096, S, ndt)
    if not misses:
        print("no row is slower than the loop it replaces", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, loop_warmup=LOOP_WARMUP, loop_reps=LOOP_REPS,
                           timer="hip events, median", note="loop_of_S_kfold_ms: S calls of blr_kfold_batched_*, one per column",
                           rows=out, misses=misses), f, indent=1)


if __name__ == "__main__":
    main()
