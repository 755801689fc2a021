"""Leave-fold-out (K-fold) predictives, timed (GPU box): python tools/kfold_bench.py [--quick] [--out FILE]
Times blr_kfold_batched_* with HIP events (median of the timed repeats after warm-up), every comparison in the same process, from
resident states at B in {2048, 64} x (D, N) = (128, 4096), fp64 and fp32, F in {1, 8, 64}, all four outputs:
  (a) F = 1 against blr_loo_batched_* (its fused route, and its composed route under option NO_MARG_GEMM: the K-fold call adds the
      round trip of the rows Z through workspace, so it is expected to cost about what the composed route costs);
  (b) the loop it replaces -- per fold blr_downdate_factor_* (k = F), blr_marginals_batched_* at the fold's inputs and
      blr_update_factor_* (k = F) -- timed on a SAMPLE of 8 folds and EXTRAPOLATED to all N / F of them (labelled as such);
  (c) K refits: blr_posterior_batched_* on N - F observations, timed once and multiplied by N / F (labelled as such).
Every row slower than its yardstick is printed as a MISS.  --quick: B = 64 only.  The numbers of DESIGN.md K23."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS, SAMPLE = 3, 11, 8


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

    def timed(fn, restore=lambda: None, reps=REPS):
        ts = []
        for r in range(WARMUP + reps):
            restore()
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
        line = f"MISS: {row['dtype']} B={row['B']} F={row['F']}: kfold {row['kfold_ms']} ms is slower than {what}"
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

        def post(n, mwo, To):
            h.posterior_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, n, X.data_ptr(), D, N * D, y.data_ptr(), N, a.NOISE_ISOTROPIC,
                                s.data_ptr(), 0, a.PRIOR_DIAGONAL, m0.data_ptr(), D, Lw.data_ptr(), 1, D, mwo.data_ptr(), D, To.data_ptr(), D,
                                D * D, None, D, D * D, None, info.data_ptr())

        post(N, mw, T)
        torch.cuda.synchronize()
        assert not info.any().item()
        km, kv = torch.empty((nb, N), dtype=dt, device=dev), torch.empty((nb, N), dtype=dt, device=dev)
        kl = torch.empty((nb, N), dtype=torch.float64, device=dev)
        tot = torch.empty(nb, dtype=torch.float64, device=dev)

        def loo():
            h.loo(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, X.data_ptr(), D, N * D, y.data_ptr(), N, a.NOISE_ISOTROPIC, s.data_ptr(), 0,
                  mw.data_ptr(), D, T.data_ptr(), D, D * D, km.data_ptr(), N, kv.data_ptr(), N, kl.data_ptr(), N, tot.data_ptr(), info.data_ptr())

        t_loo = timed(loo)
        h.set_option("NO_MARG_GEMM", "1")
        t_loo_c = timed(loo)
        h.set_option("NO_MARG_GEMM", None)
        T0, mw0 = T.clone(), mw.clone()
        lp1 = torch.empty(nb, dtype=torch.float64, device=dev)
        for F in (1, 8, 64):
            nf = -(-N // F)

            def kfold():
                h.kfold(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, F, X.data_ptr(), D, N * D, y.data_ptr(), N, a.NOISE_ISOTROPIC,
                        s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, km.data_ptr(), N, kv.data_ptr(), N, kl.data_ptr(), nf,
                        tot.data_ptr(), info.data_ptr())

            t_kf = timed(kfold)
            row = dict(dtype=name, B=nb, D=D, N=N, F=F, folds=nf, kfold_ms=round(t_kf, 4), chunks=h.get_stat("last_chunks"),
                       degenerate_folds=int(torch.isnan(kl[:, :nf]).sum().item()))
            if F == 1:
                row.update(loo_fused_ms=round(t_loo, 4), loo_composed_ms=round(t_loo_c, 4), ratio_to_loo_fused=round(t_kf / t_loo, 3),
                           ratio_to_loo_composed=round(t_kf / t_loo_c, 3))

            def restore():
                T.copy_(T0)
                mw.copy_(mw0)

            def loop():  # forget the fold, predict it, put it back: SAMPLE folds
                for f in range(SAMPLE):
                    xp, yp = X.data_ptr() + f * F * D * es, y.data_ptr() + f * F * es
                    h.downdate_factor(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, F, xp, D, N * D, yp, N, a.NOISE_ISOTROPIC, s.data_ptr(), 0,
                                      mw.data_ptr(), D, T.data_ptr(), D, D * D, lp1.data_ptr(), info.data_ptr())
                    h.marginals_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, F, xp, D, N * D, a.NOISE_ISOTROPIC, s.data_ptr(), 0,
                                        a.PRIOR_UPPER_FACTOR, mw.data_ptr(), D, T.data_ptr(), D, D * D, km.data_ptr(), N, kv.data_ptr(), N,
                                        info.data_ptr())
                    h.update_factor(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, F, xp, D, N * D, yp, N, a.NOISE_ISOTROPIC, s.data_ptr(), 0,
                                    mw.data_ptr(), D, T.data_ptr(), D, D * D, None, info.data_ptr())

            t_loop = timed(loop, restore, 5) / SAMPLE * nf
            restore()
            t_refit = timed(lambda: post(N - F, mw2, T2), reps=5) * nf
            row.update(loop_extrapolated_ms=round(t_loop, 2), loop_folds_timed=SAMPLE, speedup_over_loop=round(t_loop / t_kf, 1),
                       refits_extrapolated_ms=round(t_refit, 2), speedup_over_refits=round(t_refit / t_kf, 1))
            emit(row)
            if F == 1 and t_kf > t_loo:
                miss(row, f"blr_loo_batched_* (fused route) at {row['loo_fused_ms']} ms (x {row['ratio_to_loo_fused']})")
            if F == 1 and t_kf > t_loo_c:
                miss(row, f"blr_loo_batched_* (composed route) at {row['loo_composed_ms']} ms (x {row['ratio_to_loo_composed']})")
            if t_kf > t_loop:
                miss(row, f"the forget / predict / condition loop, extrapolated from {SAMPLE} folds, at {row['loop_extrapolated_ms']} ms")
            if t_kf > t_refit:
                miss(row, f"{nf} refits, extrapolated from one, at {row['refits_extrapolated_ms']} ms")
        del X, y, T, mw, T2, mw2, T0, mw0, km, kv, kl
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
                           note="loop_extrapolated_ms and refits_extrapolated_ms are EXTRAPOLATED from a sample (8 folds, one refit)",
                           rows=out, misses=misses), f, indent=1)


if __name__ == "__main__":
    main()
