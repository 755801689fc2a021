"""Ragged large-fold K-fold predictives, timed (GPU box): python tools/kfold_large_ragged_bench.py [--quick] [--out FILE]
Times blr_kfold_large_ragged_* (mean, var, logpdf, total; device memspace) with HIP events -- the protocol of
tools/kfold_ragged_bench.py: about two seconds of untimed calls first (clocks settle), then 3 warm-up + 15 timed calls, median -- at
D = 128, fp64 and fp32.  The states (mw', T) come from blr_posterior_ragged_* on the same packed data, so they contain every fold;
the fold sizes from blr_kfold_large_ragged_fold_sizes (K folds per regressor).
  (a) 2048 regressors at equal counts of 4096, isotropic noise, K = 10 and K = 5, against blr_kfold_large_batched_* of the same
      build (expected: parity);
  (b) 2048 regressors, N_b log-uniform in [640, 16384], diagonal noise, K = 10, against a loop of B = 1
      blr_kfold_large_batched_* calls over a sample of 64 regressors, EXTRAPOLATED to the batch (labelled as such);
  (c) one regressor of 2^20 observations among 2047 of 1024, K = 10, against the same loop: the long regressor's call timed itself,
      the short ones EXTRAPOLATED from a sample of 64.
Every row in which the ragged call is the slower one is printed as a MISS.  --quick: 128 regressors, counts divided by 8 (a smoke run
of the tool).  The numbers of DESIGN.md K28; default output profiles/kfold_large_ragged_bench.json."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WARMUP, REPS, PREHEAT_S = 3, 15, 2.0
D = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfold_large_ragged_bench.json"))
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    h = a.Handle(0)
    h.set_stream(stream)
    h.set_async(True)
    lib = a.load_library()
    nb = 128 if args.quick else 2048
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
        def __init__(self, n, nf, tdt):
            self.km, self.kv = torch.zeros(n, device=dev, dtype=tdt), torch.zeros(n, device=dev, dtype=tdt)
            self.kl = torch.zeros(nf, device=dev, dtype=torch.float64)
            self.tot = torch.zeros(nb, device=dev, dtype=torch.float64)
            self.info = torch.zeros(nb, device=dev, dtype=torch.int32)

        def same(self, o):
            return bool(torch.equal(self.km, o.km) and torch.equal(self.kv, o.kv) and torch.equal(self.kl, o.kl) and torch.equal(self.tot, o.tot))

    def tables(off, K):
        fs, fo = np.zeros(nb, dtype=np.int64), np.zeros(nb + 1, dtype=np.int64)
        assert lib.blr_kfold_large_ragged_fold_sizes(nb, a._ptr(off), K, a._ptr(fs)) == 0
        assert lib.blr_kfold_large_ragged_fold_offsets(nb, a._ptr(off), a._ptr(fs), a._ptr(fo)) == 0
        return fs, fo

    def fit(dtype, off, X, y, nk, s, tdt, gen):
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

    def ragged(dtype, off, fs, X, y, nk, s, mwp, Tp, o):
        return lambda: h.kfold_large_ragged(dtype, a.MEM_DEVICE, CV, nb, D, off, fs, p(X), D, p(y), nk, p(s), 0, p(mwp), D, p(Tp), D, D * D,
                                            p(o.km), p(o.kv), p(o.kl), p(o.tot), p(o.info))

    def batched(dtype, B, N, F, X, y, nk, s, mwp, Tp, o, first=0, at=0, fat=0):
        """blr_kfold_large_batched_* on B regressors of N observations from regressor `first`, observation `at`, fold `fat` of the arrays"""
        it = 8 if dtype == np.float64 else 4
        nf = -(-N // F)
        return lambda: h.kfold_large(dtype, a.MEM_DEVICE, CV, B, D, N, F, p(X) + at * D * it, D, D * N, p(y) + at * it, N, nk,
                                     p(s) + (at * it if nk == a.NOISE_DIAGONAL else 0), N if nk == a.NOISE_DIAGONAL else 0,
                                     p(mwp) + first * D * it, D, p(Tp) + first * D * D * it, D, D * D, p(o.km) + at * it, N, p(o.kv) + at * it, N,
                                     p(o.kl) + fat * 8, nf, p(o.tot) + first * 8, p(o.info) + first * 4)

    def same_on(o_r, o_l, off, fo, regs):
        return all(torch.equal(o_r.km[off[b]:off[b + 1]], o_l.km[off[b]:off[b + 1]]) and torch.equal(o_r.kv[off[b]:off[b + 1]], o_l.kv[off[b]:off[b + 1]])
                   and torch.equal(o_r.kl[fo[b]:fo[b + 1]], o_l.kl[fo[b]:fo[b + 1]]) and torch.equal(o_r.tot[b], o_l.tot[b]) for b in regs)

    def case(dtype):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        name = np.dtype(dtype).name
        gen = torch.Generator(device=dev).manual_seed(4321)
        rows = []

        def emit(slower, **kw):
            rows.append(dict(D=D, dtype=name, B=nb, **kw))
            print(json.dumps(rows[-1]), flush=True)
            if slower:
                misses.append(f"MISS: case {kw['case']} {name} K={kw['K']}: {slower}")
                print(misses[-1], flush=True)

        def data(counts, diag):
            total = int(counts.sum())
            off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
            X = torch.randn((total, D), device=dev, dtype=tdt, generator=gen) * (0.7 / math.sqrt(D))
            y = torch.randn(total, device=dev, dtype=tdt, generator=gen)
            s = torch.exp(0.3 * torch.randn(total, device=dev, dtype=tdt, generator=gen)) if diag else torch.full((1,), 0.5, device=dev, dtype=tdt)
            nk = a.NOISE_DIAGONAL if diag else a.NOISE_ISOTROPIC
            mwp, Tp = fit(dtype, off, X, y, nk, s, tdt, gen)
            return total, off, X, y, s, nk, mwp, Tp

        # ---- (a) equal counts against the equal-count entry point --------------------------------------------------------------------
        N = 4096 // shrink
        counts = np.full(nb, N, dtype=np.int64)
        total, off, X, y, s, nk, mwp, Tp = data(counts, False)
        for K in (10, 5):
            fs, fo = tables(off, K)
            F = int(fs[0])
            o_r, o_b = Out(total, int(fo[-1]), tdt), Out(total, int(fo[-1]), tdt)
            t_r = timed(ragged(dtype, off, fs, X, y, nk, s, mwp, Tp, o_r))
            chunks = h.get_stat("last_chunks")
            t_b = timed(batched(dtype, nb, N, F, X, y, nk, s, mwp, Tp, o_b))
            chunks_b = h.get_stat("last_chunks")
            torch.cuda.synchronize()
            assert int(o_r.info.abs().sum()) == 0 and int(o_b.info.abs().sum()) == 0
            emit(f"ragged {t_r:.3f} ms against blr_kfold_large_batched_* at {t_b:.3f} ms" if t_r > t_b else None,
                 case="a", K=K, N=N, F=F, ragged_ms=round(t_r, 4), batched_ms=round(t_b, 4), ragged_over_batched=round(t_r / t_b, 4),
                 ragged_chunks=chunks, batched_chunks=chunks_b, bit_identical=o_r.same(o_b), nan_folds=int(torch.isnan(o_r.kl).sum()))
            del o_r, o_b
        del X, y
        torch.cuda.empty_cache()

        # ---- (b) log-uniform counts: ragged against a loop of single calls -----------------------------------------------------------
        K = 10
        rng = np.random.Generator(np.random.PCG64(99))
        lo, hi = 640 // shrink, 16384 // shrink
        counts = np.floor(np.exp(rng.uniform(math.log(lo), math.log(hi + 1), size=nb))).astype(np.int64).clip(lo, hi)
        total, off, X, y, s, nk, mwp, Tp = data(counts, True)
        fs, fo = tables(off, K)
        sample = np.random.Generator(np.random.PCG64(7)).choice(nb, size=min(64, nb), replace=False)
        o_r, o_l = Out(total, int(fo[-1]), tdt), Out(total, int(fo[-1]), tdt)
        t_r = timed(ragged(dtype, off, fs, X, y, nk, s, mwp, Tp, o_r))
        chunks = h.get_stat("last_chunks")
        singles = [batched(dtype, 1, int(counts[b]), int(fs[b]), X, y, nk, s, mwp, Tp, o_l, first=int(b), at=int(off[b]), fat=int(fo[b])) for b in sample]
        t_l = timed(lambda: [f() for f in singles], preheat=False) * nb / len(sample)
        torch.cuda.synchronize()
        assert int(o_r.info.abs().sum()) == 0
        emit(f"ragged {t_r:.3f} ms against the loop, extrapolated, at {t_l:.1f} ms" if t_r > t_l else None,
             case="b", K=K, counts=f"log-uniform in [{lo}, {hi}]", max_N=int(counts.max()), mean_N=round(total / nb, 1), ragged_ms=round(t_r, 4),
             loop_ms_extrapolated=round(t_l, 2), loop_sample=len(sample), loop_over_ragged=round(t_l / t_r, 2), ragged_chunks=chunks,
             bit_identical_on_sample=bool(same_on(o_r, o_l, off, fo, sample)), nan_folds=int(torch.isnan(o_r.kl).sum()))
        del o_r, o_l, X, y, s
        torch.cuda.empty_cache()

        # ---- (c) one very long regressor among short ones, against the same loop ------------------------------------------------------
        counts = np.full(nb, 1024 // min(shrink, 4), dtype=np.int64)
        big = nb // 2
        counts[big] = (1 << 20) // shrink
        total, off, X, y, s, nk, mwp, Tp = data(counts, True)
        fs, fo = tables(off, K)
        short = np.array([b for b in np.random.Generator(np.random.PCG64(7)).choice(nb, size=min(65, nb), replace=False) if b != big][:64])
        o_r, o_l = Out(total, int(fo[-1]), tdt), Out(total, int(fo[-1]), tdt)
        t_r = timed(ragged(dtype, off, fs, X, y, nk, s, mwp, Tp, o_r))
        chunks = h.get_stat("last_chunks")
        one = lambda b: batched(dtype, 1, int(counts[b]), int(fs[b]), X, y, nk, s, mwp, Tp, o_l, first=int(b), at=int(off[b]), fat=int(fo[b]))  # noqa: E731
        t_big = timed(one(big), preheat=False)
        singles = [one(b) for b in short]
        t_short = timed(lambda: [f() for f in singles], preheat=False) * (nb - 1) / len(short)
        t_l = t_big + t_short
        torch.cuda.synchronize()
        assert int(o_r.info.abs().sum()) == 0
        emit(f"ragged {t_r:.3f} ms against the loop, extrapolated, at {t_l:.1f} ms" if t_r > t_l else None,
             case="c", K=K, long_N=int(counts[big]), other_N=int(counts[0]), ragged_ms=round(t_r, 4), loop_long_ms=round(t_big, 4),
             loop_short_ms_extrapolated=round(t_short, 2), loop_ms_extrapolated=round(t_l, 2), loop_sample=len(short), loop_over_ragged=round(t_l / t_r, 2),
             ragged_chunks=chunks, bit_identical_on_sample=bool(same_on(o_r, o_l, off, fo, [big] + list(short))), nan_folds=int(torch.isnan(o_r.kl).sum()))
        del o_r, o_l, X, y, s
        torch.cuda.empty_cache()
        return rows

    rows = case(np.float64) + case(np.float32)
    if not misses:
        print("no row has the ragged call as the slower one", flush=True)
    res = dict(tool="tools/kfold_large_ragged_bench.py", device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, preheat_s=PREHEAT_S,
               timer="HIP events, median", quick=bool(args.quick),
               note="loop_ms_extrapolated / loop_short_ms_extrapolated are EXTRAPOLATED from loop_sample regressors", rows=rows, misses=misses)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
