"""Ragged K-fold predictives, timed (GPU box): python tools/kfold_ragged_bench.py [--quick] [--out FILE]
Times blr_kfold_ragged_* (mean, var, logpdf, total; device memspace) with HIP events -- the protocol of tools/marg_ragged_bench.py:
about two seconds of untimed calls first (clocks settle), then 3 warm-up + 15 timed calls, median -- at D = 128 fp64 and D = 64
fp32, F in {8, 64}.  The states (mw', T) come from blr_posterior_ragged_* on the same packed data, so they contain every fold.
  (a) 4096 regressors at equal counts of 4096, isotropic noise, against blr_kfold_batched_* of the same build;
  (b) 4096 regressors, N_b log-uniform in [64, 16384], diagonal noise, against a loop of B = 1 blr_kfold_batched_* calls (what
      kfold_map does for such a batch) over a sample of 64 regressors, EXTRAPOLATED to the batch (labelled as such).  Padding to the
      longest regressor is no route here: it changes the folds;
  (c) one regressor of 2^20 observations among 4095 of 256, against the same call on a handle with RAGGED_ITEM = 2^20 (the long
      regressor's whitening stays one work item): whether cutting it pays.
Every row in which the ragged call is the slower one is printed as a MISS.  --quick: 256 regressors, counts divided by 8 (a smoke run
of the tool).  The numbers of DESIGN.md K27."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS, PREHEAT_S = 3, 15, 2.0
FS = (8, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream

    def handle(**opts):
        hd = a.Handle(0)
        hd.set_stream(stream)
        hd.set_async(True)
        for k, v in opts.items():
            hd.set_option(k, v)
        return hd

    h = handle()
    h_whole = handle(RAGGED_ITEM=str(1 << 20))
    nb = 256 if args.quick else 4096
    shrink = 8 if args.quick else 1
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    CV = a.LAYOUT_COLVECS
    misses = []

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn, preheat=True):
        spent = once(fn)
        while preheat and spent < PREHEAT_S * 1e3:
            spent += once(fn)
        ts = [once(fn) for _ in range(WARMUP + REPS)]
        return float(np.median(ts[WARMUP:]))

    class Out:
        """outputs of one route: per-observation arrays of n elements, nf log densities, per-regressor arrays of nb"""

        def __init__(self, n, nf, tdt):
            self.km, self.kv = torch.zeros(n, device=dev, dtype=tdt), torch.zeros(n, device=dev, dtype=tdt)
            self.kl = torch.zeros(nf, device=dev, dtype=torch.float64)
            self.tot = torch.zeros(nb, device=dev, dtype=torch.float64)
            self.info = torch.zeros(nb, device=dev, dtype=torch.int32)

        def same(self, o):
            return bool(torch.equal(self.km, o.km) and torch.equal(self.kv, o.kv) and torch.equal(self.kl, o.kl) and torch.equal(self.tot, o.tot))

    def fit(dtype, D, off, X, y, nk, s, tdt, gen):
        """states of the packed data: diagonal prior, blr_posterior_ragged_*"""
        mw = 0.1 * torch.randn((nb, D), device=dev, dtype=tdt, generator=gen)
        Lw = torch.exp(0.3 * torch.randn((nb, D), device=dev, dtype=tdt, generator=gen))
        mwp, Tp = torch.zeros((nb, D), device=dev, dtype=tdt), torch.zeros((nb, D, D), device=dev, dtype=tdt)
        info = torch.zeros(nb, device=dev, dtype=torch.int32)
        h.posterior_ragged(dtype, a.MEM_DEVICE, CV, nb, D, off, p(X), D, p(y), nk, p(s), 0, a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D,
                           p(mwp), D, p(Tp), D, D * D, None, D, D * D, None, p(info))
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0
        return mwp, Tp

    def fold_offsets(counts, F):
        return np.concatenate(([0], np.cumsum(-(-counts // F)))).astype(np.int64)

    def ragged(hd, dtype, D, off, F, X, y, nk, s, mwp, Tp, o):
        return lambda: hd.kfold_ragged(dtype, a.MEM_DEVICE, CV, nb, D, off, F, p(X), D, p(y), nk, p(s), 0, p(mwp), D, p(Tp), D, D * D,
                                       p(o.km), p(o.kv), p(o.kl), p(o.tot), p(o.info))

    def batched(dtype, B, D, N, F, X, y, nk, s, mwp, Tp, o, first=0, at=0, fat=0):
        """blr_kfold_batched_* on B regressors of N observations from regressor `first`, observation `at`, fold `fat` of the arrays"""
        it = 8 if dtype == np.float64 else 4
        nf = -(-N // F)
        return lambda: h.kfold(dtype, a.MEM_DEVICE, CV, B, D, N, F, p(X) + at * D * it, D, D * N, p(y) + at * it, N, nk,
                               p(s) + (at * it if nk == a.NOISE_DIAGONAL else 0), N if nk == a.NOISE_DIAGONAL else 0,
                               p(mwp) + first * D * it, D, p(Tp) + first * D * D * it, D, D * D, p(o.km) + at * it, N, p(o.kv) + at * it, N,
                               p(o.kl) + fat * 8, nf, p(o.tot) + first * 8, p(o.info) + first * 4)

    def case(D, dtype):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        name = np.dtype(dtype).name
        gen = torch.Generator(device=dev).manual_seed(4321)
        rows = []

        def emit(slower, **kw):
            rows.append(dict(D=D, dtype=name, B=nb, **kw))
            print(json.dumps(rows[-1]), flush=True)
            if slower:
                misses.append(f"MISS: case {kw['case']} {name} D={D} F={kw['F']}: {slower}")
                print(misses[-1], flush=True)

        # ---- (a) equal counts against the equal-count entry point --------------------------------------------------------------------
        N = 4096 // shrink
        X = torch.randn((nb * N, D), device=dev, dtype=tdt, generator=gen) * (0.7 / math.sqrt(D))
        y = torch.randn(nb * N, device=dev, dtype=tdt, generator=gen)
        s = torch.full((1,), 0.5, device=dev, dtype=tdt)
        counts = np.full(nb, N, dtype=np.int64)
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        mwp, Tp = fit(dtype, D, off, X, y, a.NOISE_ISOTROPIC, s, tdt, gen)
        for F in FS:
            nf = int(fold_offsets(counts, F)[-1])
            o_r, o_b = Out(nb * N, nf, tdt), Out(nb * N, nf, tdt)
            t_r = timed(ragged(h, dtype, D, off, F, X, y, a.NOISE_ISOTROPIC, s, mwp, Tp, o_r))
            chunks = h.get_stat("last_chunks")
            t_b = timed(batched(dtype, nb, D, N, F, X, y, a.NOISE_ISOTROPIC, s, mwp, Tp, o_b))
            torch.cuda.synchronize()
            assert int(o_r.info.abs().sum()) == 0 and int(o_b.info.abs().sum()) == 0
            emit(f"ragged {t_r:.3f} ms against blr_kfold_batched_* at {t_b:.3f} ms" if t_r > t_b else None,
                 case="a", F=F, N=N, ragged_ms=round(t_r, 4), batched_ms=round(t_b, 4), ragged_over_batched=round(t_r / t_b, 4),
                 ragged_chunks=chunks, bit_identical=o_r.same(o_b), nan_folds=int(torch.isnan(o_r.kl).sum()))
            del o_r, o_b
        del X, y
        torch.cuda.empty_cache()

        # ---- (b) log-uniform counts: ragged against a loop of single calls -----------------------------------------------------------
        rng = np.random.Generator(np.random.PCG64(99))
        lo, hi = 64 // min(shrink, 4), 16384 // shrink
        counts = np.floor(np.exp(rng.uniform(math.log(lo), math.log(hi + 1), size=nb))).astype(np.int64).clip(lo, hi)
        nmax, total = int(counts.max()), int(counts.sum())
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        Xp = torch.randn((total, D), device=dev, dtype=tdt, generator=gen) * (0.7 / math.sqrt(D))
        yp = torch.randn(total, device=dev, dtype=tdt, generator=gen)
        sp = torch.exp(0.3 * torch.randn(total, device=dev, dtype=tdt, generator=gen))
        mwp, Tp = fit(dtype, D, off, Xp, yp, a.NOISE_DIAGONAL, sp, tdt, gen)
        sample = np.random.Generator(np.random.PCG64(7)).choice(nb, size=min(64, nb), replace=False)
        for F in FS:
            fo = fold_offsets(counts, F)
            o_r, o_l = Out(total, int(fo[-1]), tdt), Out(total, int(fo[-1]), tdt)
            t_r = timed(ragged(h, dtype, D, off, F, Xp, yp, a.NOISE_DIAGONAL, sp, mwp, Tp, o_r))
            chunks = h.get_stat("last_chunks")
            singles = [batched(dtype, 1, D, int(counts[b]), F, Xp, yp, a.NOISE_DIAGONAL, sp, mwp, Tp, o_l, first=int(b), at=int(off[b]),
                               fat=int(fo[b])) for b in sample]
            t_l = timed(lambda: [f() for f in singles], preheat=False) * nb / len(sample)
            torch.cuda.synchronize()
            assert int(o_r.info.abs().sum()) == 0
            same = all(torch.equal(o_r.km[off[b]:off[b + 1]], o_l.km[off[b]:off[b + 1]]) and torch.equal(o_r.kv[off[b]:off[b + 1]], o_l.kv[off[b]:off[b + 1]])
                       and torch.equal(o_r.kl[fo[b]:fo[b + 1]], o_l.kl[fo[b]:fo[b + 1]]) and torch.equal(o_r.tot[b], o_l.tot[b]) for b in sample)
            emit(f"ragged {t_r:.3f} ms against the loop, extrapolated, at {t_l:.1f} ms" if t_r > t_l else None,
                 case="b", F=F, counts=f"log-uniform in [{lo}, {hi}]", max_N=nmax, mean_N=round(total / nb, 1), ragged_ms=round(t_r, 4),
                 loop_ms_extrapolated=round(t_l, 2), loop_sample=len(sample), loop_over_ragged=round(t_l / t_r, 2), ragged_chunks=chunks,
                 bit_identical_on_sample=bool(same), nan_folds=int(torch.isnan(o_r.kl).sum()))
            del o_r, o_l
        del Xp, yp, sp
        torch.cuda.empty_cache()

        # ---- (c) one very long regressor: whitening cut into items against kept whole ------------------------------------------------
        counts = np.full(nb, 256 // min(shrink, 4), dtype=np.int64)
        counts[nb // 2] = (1 << 20) // shrink
        total = int(counts.sum())
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        Xp = torch.randn((total, D), device=dev, dtype=tdt, generator=gen) * (0.7 / math.sqrt(D))
        yp = torch.randn(total, device=dev, dtype=tdt, generator=gen)
        sp = torch.exp(0.3 * torch.randn(total, device=dev, dtype=tdt, generator=gen))
        mwp, Tp = fit(dtype, D, off, Xp, yp, a.NOISE_DIAGONAL, sp, tdt, gen)
        for F in FS:
            nf = int(fold_offsets(counts, F)[-1])
            o_r, o_w = Out(total, nf, tdt), Out(total, nf, tdt)
            t_r = timed(ragged(h, dtype, D, off, F, Xp, yp, a.NOISE_DIAGONAL, sp, mwp, Tp, o_r))
            t_w = timed(ragged(h_whole, dtype, D, off, F, Xp, yp, a.NOISE_DIAGONAL, sp, mwp, Tp, o_w))
            torch.cuda.synchronize()
            assert int(o_r.info.abs().sum()) == 0 and int(o_w.info.abs().sum()) == 0
            emit(f"cut into items {t_r:.3f} ms against kept whole at {t_w:.3f} ms" if t_r > t_w else None,
                 case="c", F=F, long_N=int(counts[nb // 2]), other_N=int(counts[0]), split_ms=round(t_r, 4), whole_ms=round(t_w, 4),
                 whole_over_split=round(t_w / t_r, 3), bit_identical=o_r.same(o_w), nan_folds=int(torch.isnan(o_r.kl).sum()))
            del o_r, o_w
        del Xp, yp, sp
        torch.cuda.empty_cache()
        return rows

    rows = case(128, np.float64) + case(64, np.float32)
    if not misses:
        print("no row has the ragged call as the slower one", flush=True)
    res = dict(tool="tools/kfold_ragged_bench.py", device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, preheat_s=PREHEAT_S,
               timer="HIP events, median", note="loop_ms_extrapolated is EXTRAPOLATED from a sample of regressors", rows=rows, misses=misses)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
