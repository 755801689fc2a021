"""Leave-fold-out predictives for large folds, timed (GPU box): python tools/kfold_large_bench.py [--quick] [--out FILE]
Times blr_kfold_large_batched_* with HIP events (median of the timed repeats after warm-up), every comparison in the same process,
from resident states at B in {2048, 64} x (D, N) = (128, 4096), fp64 and fp32, F in {64, 128, 410 (10 folds), 820 (5 folds), 2048},
all four outputs:
  (a) K refits: per fold blr_posterior_batched_* on the OTHER folds' data (gathered into a buffer of its own before the clock starts)
      plus blr_marginals_batched_* at the fold's inputs -- MEASURED fold by fold where K <= 10, else timed on the first fold and
      EXTRAPOLATED to all K (labelled as such);
  (b) F = 64 against blr_kfold_batched_*, the observation-space route.
Every row slower than a yardstick is printed as a MISS.  --quick: B = 64 only.  The numbers of DESIGN.md K24."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS = 3, 11
FOLD_SIZES = (64, 128, 410, 820, 2048)


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

    def timed(fn, reps=REPS):
        ts = []
        for r in range(WARMUP + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    out, misses = [], []

    def emit(row):
        print(json.dumps(row), flush=True)
        out.append(row)

    def miss(row, what):
        line = f"MISS: {row['dtype']} B={row['B']} F={row['F']}: kfold_large {row['kfold_large_ms']} ms is slower than {what}"
        print(line, flush=True)
        misses.append(line)

    def shape(nb, D, N, ndt):
        dt = torch.float64 if ndt == np.float64 else torch.float32
        name = np.dtype(ndt).name
        g = torch.Generator(device=dev).manual_seed(1)
        X = torch.randn((nb, N, D), generator=g, dtype=dt, device=dev) * (1.0 / np.sqrt(D))
        y = torch.randn((nb, N), generator=g, dtype=dt, device=dev)
        s = torch.full((1,), 0.5, dtype=dt, device=dev)
        Lw = torch.ones((nb, D), dtype=dt, device=dev)
        m0 = torch.zeros((nb, D), dtype=dt, device=dev)
        mw, T = torch.empty((nb, D), dtype=dt, device=dev), torch.empty((nb, D, D), dtype=dt, device=dev)
        mw2, T2 = torch.empty_like(mw), torch.empty_like(T)
        info = torch.zeros(nb, dtype=torch.int32, device=dev)
        es = X.element_size()

        def post(Xs, ys, n, ld_n, mwo, To):
            h.posterior_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, n, Xs.data_ptr(), D, ld_n * D, ys.data_ptr(), ld_n,
                                a.NOISE_ISOTROPIC, s.data_ptr(), 0, a.PRIOR_DIAGONAL, m0.data_ptr(), D, Lw.data_ptr(), 1, D, mwo.data_ptr(), D,
                                To.data_ptr(), D, D * D, None, D, D * D, None, info.data_ptr())

        post(X, y, N, N, mw, T)
        torch.cuda.synchronize()
        assert not info.any().item()
        km, kv = torch.empty((nb, N), dtype=dt, device=dev), torch.empty((nb, N), dtype=dt, device=dev)
        kl = torch.empty((nb, N), dtype=torch.float64, device=dev)
        tot = torch.empty(nb, dtype=torch.float64, device=dev)
        for F in FOLD_SIZES:
            nf = -(-N // F)
            kf_args = (ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, F, X.data_ptr(), D, N * D, y.data_ptr(), N, a.NOISE_ISOTROPIC,
                       s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, km.data_ptr(), N, kv.data_ptr(), N, kl.data_ptr(), nf,
                       tot.data_ptr(), info.data_ptr())
            t_kf = timed(lambda: h.kfold_large(*kf_args))
            row = dict(dtype=name, B=nb, D=D, N=N, F=F, folds=nf, kfold_large_ms=round(t_kf, 4), chunks=h.get_stat("last_chunks"),
                       degenerate_folds=int(torch.isnan(kl[:, :nf]).sum().item()))
            measured = nf <= 10
            t_refit = 0.0
            for f in range(nf if measured else 1):
                lo, hi = f * F, min((f + 1) * F, N)
                Xr = torch.cat([X[:, :lo], X[:, hi:]], dim=1).contiguous()  # the other folds' data, gathered before the clock starts
                yr = torch.cat([y[:, :lo], y[:, hi:]], dim=1).contiguous()
                nr = N - (hi - lo)

                def refit():
                    post(Xr, yr, nr, nr, mw2, T2)
                    h.marginals_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, hi - lo, X.data_ptr() + lo * D * es, D, N * D,
                                        a.NOISE_ISOTROPIC, s.data_ptr(), 0, a.PRIOR_UPPER_FACTOR, mw2.data_ptr(), D, T2.data_ptr(), D, D * D,
                                        km.data_ptr(), N, kv.data_ptr(), N, info.data_ptr())

                t_refit += timed(refit, reps=5)
                del Xr, yr
            if not measured:
                t_refit *= nf
            row.update(refits_ms=round(t_refit, 2), refits_measured=measured, speedup_over_refits=round(t_refit / t_kf, 2))
            if F <= 64:
                t_small = timed(lambda: h.kfold(*kf_args))
                row.update(kfold_ms=round(t_small, 4), ratio_to_kfold=round(t_kf / t_small, 3))
            emit(row)
            if t_kf > t_refit:
                miss(row, f"{nf} refits ({'measured' if measured else 'extrapolated from one'}) at {row['refits_ms']} ms")
            if F <= 64 and t_kf > t_small:
                miss(row, f"blr_kfold_batched_* at {row['kfold_ms']} ms (x {row['ratio_to_kfold']})")
        del X, y, T, mw, T2, mw2, km, kv, kl
        torch.cuda.empty_cache()

    for ndt in (np.float64, np.float32):
        if not args.quick:
            shape(2048, 128, 4096, ndt)
        shape(64, 128, 4096, ndt)
    if not misses:
        print("no row is slower than its yardstick", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, timer="hip events, median",
                           note="refits_ms is MEASURED fold by fold where refits_measured is true, else EXTRAPOLATED from the first fold",
                           rows=out, misses=misses), f, indent=1)


if __name__ == "__main__":
    main()
