"""Ragged marginals and leave-one-out, timed (GPU box): python tools/marg_ragged_bench.py [--quick] [--out FILE]
Times blr_marginals_ragged_* (mean + var) and blr_loo_ragged_* (mean, var, logpdf, total; device memspace) with HIP events -- the
protocol of tools/ragged_bench.py: about two seconds of untimed calls first (clocks settle), then 3 warm-up + 15 timed calls,
median -- at D = 128 fp64 and D = 64 fp32.  The states (mw', T) come from blr_posterior_ragged_* on the same packed data, so the
leave-one-out sees states that contain their observations.
  (a) 4096 regressors at equal counts of 4096, isotropic noise, against blr_marginals_batched_* / blr_loo_batched_* of the same
      build;
  (b) 4096 regressors, N_b log-uniform in [64, 16384], diagonal noise, three routes to the same numbers: the ragged call; the
      equal-count call on every regressor padded to max N_b with x = 0, y = 0, s = 1 columns; a loop of B = 1 equal-count calls
      over a sample of 64 regressors, scaled to the batch.  The padding ratio of the drawn counts is recorded;
  (c) one regressor of 2^20 observations among 4095 of 256, against the same call on a handle with RAGGED_ITEM = 2^20 (the long
      regressor stays one work item): whether cutting it pays.
--quick: 256 regressors, counts divided by 8 (a smoke run of the tool).
The numbers of DESIGN.md K26."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS, PREHEAT_S = 3, 15, 2.0


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
        """outputs of one route: per-observation arrays of n elements, per-regressor ones of nb"""

        def __init__(self, n, tdt):
            self.mean, self.var = torch.zeros(n, device=dev, dtype=tdt), torch.zeros(n, device=dev, dtype=tdt)
            self.lm, self.lv = torch.zeros(n, device=dev, dtype=tdt), torch.zeros(n, device=dev, dtype=tdt)
            self.ll = torch.zeros(n, device=dev, dtype=torch.float64)
            self.tot = torch.zeros(nb, device=dev, dtype=torch.float64)
            self.info = torch.zeros(nb, device=dev, dtype=torch.int32)

    def fit(dtype, D, off, X, y, nk, s, strides, tdt, gen):
        """states of the packed data: diagonal prior, blr_posterior_ragged_*"""
        mw = 0.1 * torch.randn((nb, D), device=dev, dtype=tdt, generator=gen)
        Lw = torch.exp(0.3 * torch.randn((nb, D), device=dev, dtype=tdt, generator=gen))
        mwp, Tp = torch.zeros((nb, D), device=dev, dtype=tdt), torch.zeros((nb, D, D), device=dev, dtype=tdt)
        info = torch.zeros(nb, device=dev, dtype=torch.int32)
        h.posterior_ragged(dtype, a.MEM_DEVICE, CV, nb, D, off, p(X), D, p(y), nk, p(s), strides, a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D,
                           p(mwp), D, p(Tp), D, D * D, None, D, D * D, None, p(info))
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0
        return mwp, Tp

    def marg_ragged(hd, dtype, D, off, X, nk, s, strides, mwp, Tp, o):
        return lambda: hd.marginals_ragged(dtype, a.MEM_DEVICE, CV, nb, D, off, p(X), D, nk, p(s), strides, a.PRIOR_UPPER_FACTOR, p(mwp), D,
                                           p(Tp), D, D * D, p(o.mean), p(o.var), p(o.info))

    def loo_ragged(hd, dtype, D, off, X, y, nk, s, strides, mwp, Tp, o):
        return lambda: hd.loo_ragged(dtype, a.MEM_DEVICE, CV, nb, D, off, p(X), D, p(y), nk, p(s), strides, p(mwp), D, p(Tp), D, D * D,
                                     p(o.lm), p(o.lv), p(o.ll), p(o.tot), p(o.info))

    def marg_batched(dtype, B, D, N, X, nk, s, strides, mwp, Tp, o, first=0, at=0):
        it = 8 if dtype == np.float64 else 4
        return lambda: h.marginals_batched(dtype, a.MEM_DEVICE, CV, B, D, N, p(X), D, D * N, nk, p(s), strides, a.PRIOR_UPPER_FACTOR,
                                           p(mwp) + first * D * it, D, p(Tp) + first * D * D * it, D, D * D, p(o.mean) + at * it, N,
                                           p(o.var) + at * it, N, p(o.info) + first * 4)

    def loo_batched(dtype, B, D, N, X, y, nk, s, strides, mwp, Tp, o, first=0, at=0):
        it = 8 if dtype == np.float64 else 4
        return lambda: h.loo(dtype, a.MEM_DEVICE, CV, B, D, N, p(X), D, D * N, p(y), N, nk, p(s), strides, p(mwp) + first * D * it, D,
                             p(Tp) + first * D * D * it, D, D * D, p(o.lm) + at * it, N, p(o.lv) + at * it, N, p(o.ll) + at * 8, N,
                             p(o.tot) + first * 8, p(o.info) + first * 4)

    def rel(x, y_):
        return float(((x - y_).abs() / (y_.abs() + 1e-30)).max())

    def case(D, dtype):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        name = np.dtype(dtype).name
        gen = torch.Generator(device=dev).manual_seed(4321)
        rows = []

        def emit(**kw):
            rows.append(dict(D=D, dtype=name, B=nb, **kw))
            print(json.dumps(rows[-1]), flush=True)

        # ---- (a) equal counts against the equal-count entry points ----------------------------------------------------------------
        N = 4096 // shrink
        X = torch.randn((nb * N, D), device=dev, dtype=tdt, generator=gen) * (0.7 / math.sqrt(D))
        y = torch.randn(nb * N, device=dev, dtype=tdt, generator=gen)
        s = torch.full((1,), 0.5, device=dev, dtype=tdt)
        off = np.arange(nb + 1, dtype=np.int64) * N
        mwp, Tp = fit(dtype, D, off, X, y, a.NOISE_ISOTROPIC, s, 0, tdt, gen)
        o_r, o_b = Out(nb * N, tdt), Out(nb * N, tdt)
        t_mr = timed(marg_ragged(h, dtype, D, off, X, a.NOISE_ISOTROPIC, s, 0, mwp, Tp, o_r))
        route = h.last_route()
        t_mb = timed(marg_batched(dtype, nb, D, N, X, a.NOISE_ISOTROPIC, s, 0, mwp, Tp, o_b))
        t_lr = timed(loo_ragged(h, dtype, D, off, X, y, a.NOISE_ISOTROPIC, s, 0, mwp, Tp, o_r))
        t_lb = timed(loo_batched(dtype, nb, D, N, X, y, a.NOISE_ISOTROPIC, s, 0, mwp, Tp, o_b))
        torch.cuda.synchronize()
        assert int(o_r.info.abs().sum()) == 0 and int(o_b.info.abs().sum()) == 0
        emit(case="a", what="marginals", N=N, ragged_ms=round(t_mr, 4), batched_ms=round(t_mb, 4), ragged_over_batched=round(t_mr / t_mb, 4),
             ragged_route=route, max_rel_diff_var=rel(o_r.var, o_b.var))
        emit(case="a", what="loo", N=N, ragged_ms=round(t_lr, 4), batched_ms=round(t_lb, 4), ragged_over_batched=round(t_lr / t_lb, 4),
             max_rel_diff_total=rel(o_r.tot, o_b.tot))
        del X, y, o_r, o_b
        torch.cuda.empty_cache()

        # ---- (b) log-uniform counts: ragged, padded to the longest, a loop of single calls ----------------------------------------
        rng = np.random.Generator(np.random.PCG64(99))
        lo, hi = 64 // min(shrink, 4), 16384 // shrink
        counts = np.floor(np.exp(rng.uniform(math.log(lo), math.log(hi + 1), size=nb))).astype(np.int64).clip(lo, hi)
        nmax, total = int(counts.max()), int(counts.sum())
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        Xp = torch.randn((total, D), device=dev, dtype=tdt, generator=gen) * (0.7 / math.sqrt(D))
        yp = torch.randn(total, device=dev, dtype=tdt, generator=gen)
        sp = torch.exp(0.3 * torch.randn(total, device=dev, dtype=tdt, generator=gen))
        mwp, Tp = fit(dtype, D, off, Xp, yp, a.NOISE_DIAGONAL, sp, 0, tdt, gen)
        mask = torch.arange(nmax, device=dev)[None, :] < torch.tensor(counts, device=dev)[:, None]  # [B, nmax]
        Xpad = torch.zeros((nb, nmax, D), device=dev, dtype=tdt)
        Xpad[mask] = Xp
        ypad = torch.zeros((nb, nmax), device=dev, dtype=tdt)
        ypad[mask] = yp
        spad = torch.ones((nb, nmax), device=dev, dtype=tdt)
        spad[mask] = sp
        o_r, o_p, o_l = Out(total, tdt), Out(nb * nmax, tdt), Out(total, tdt)
        res = {}
        for what, rag, pad, single in (
                ("marginals", marg_ragged(h, dtype, D, off, Xp, a.NOISE_DIAGONAL, sp, 0, mwp, Tp, o_r),
                 marg_batched(dtype, nb, D, nmax, Xpad, a.NOISE_DIAGONAL, spad, nmax, mwp, Tp, o_p),
                 lambda b: marg_batched(dtype, 1, D, int(counts[b]), Xp[off[b]:], a.NOISE_DIAGONAL, sp[off[b]:], 0, mwp, Tp, o_l, first=int(b), at=int(off[b]))),
                ("loo", loo_ragged(h, dtype, D, off, Xp, yp, a.NOISE_DIAGONAL, sp, 0, mwp, Tp, o_r),
                 loo_batched(dtype, nb, D, nmax, Xpad, ypad, a.NOISE_DIAGONAL, spad, nmax, mwp, Tp, o_p),
                 lambda b: loo_batched(dtype, 1, D, int(counts[b]), Xp[off[b]:], yp[off[b]:], a.NOISE_DIAGONAL, sp[off[b]:], 0, mwp, Tp, o_l, first=int(b), at=int(off[b])))):
            t_r, t_p = timed(rag), timed(pad)
            sample = np.random.Generator(np.random.PCG64(7)).choice(nb, size=min(64, nb), replace=False)
            singles = [single(b) for b in sample]
            t_l = timed(lambda: [f() for f in singles], preheat=False) * nb / len(sample)
            torch.cuda.synchronize()
            assert int(o_r.info.abs().sum()) == 0 and int(o_p.info.abs().sum()) == 0
            if what == "marginals":
                diff = rel(o_r.var, o_p.var.view(nb, nmax)[mask])
            else:
                diff = rel(o_r.ll, o_p.ll.view(nb, nmax)[mask])
            res[what] = dict(ragged_ms=round(t_r, 4), padded_ms=round(t_p, 4), loop_ms_scaled=round(t_l, 2), loop_sample=len(sample),
                             padded_over_ragged=round(t_p / t_r, 3), loop_over_ragged=round(t_l / t_r, 2), max_rel_diff_vs_padded=diff)
        for what, r in res.items():
            emit(case="b", what=what, counts=f"log-uniform in [{lo}, {hi}]", max_N=nmax, mean_N=round(total / nb, 1),
                 padding_ratio=round(nmax * nb / total, 3), **r)
        del Xpad, ypad, spad, Xp, yp, sp, o_r, o_p, o_l, mask
        torch.cuda.empty_cache()

        # ---- (c) one very long regressor: cut into items against kept whole --------------------------------------------------------
        counts = np.full(nb, 256 // min(shrink, 4), dtype=np.int64)
        counts[nb // 2] = (1 << 20) // shrink
        total = int(counts.sum())
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        Xp = torch.randn((total, D), device=dev, dtype=tdt, generator=gen) * (0.7 / math.sqrt(D))
        yp = torch.randn(total, device=dev, dtype=tdt, generator=gen)
        sp = torch.exp(0.3 * torch.randn(total, device=dev, dtype=tdt, generator=gen))
        mwp, Tp = fit(dtype, D, off, Xp, yp, a.NOISE_DIAGONAL, sp, 0, tdt, gen)
        o_r, o_w = Out(total, tdt), Out(total, tdt)
        t_mr = timed(marg_ragged(h, dtype, D, off, Xp, a.NOISE_DIAGONAL, sp, 0, mwp, Tp, o_r))
        t_mw = timed(marg_ragged(h_whole, dtype, D, off, Xp, a.NOISE_DIAGONAL, sp, 0, mwp, Tp, o_w))
        t_lr = timed(loo_ragged(h, dtype, D, off, Xp, yp, a.NOISE_DIAGONAL, sp, 0, mwp, Tp, o_r))
        t_lw = timed(loo_ragged(h_whole, dtype, D, off, Xp, yp, a.NOISE_DIAGONAL, sp, 0, mwp, Tp, o_w))
        torch.cuda.synchronize()
        same = bool(torch.equal(o_r.var, o_w.var) and torch.equal(o_r.mean, o_w.mean) and torch.equal(o_r.ll, o_w.ll) and torch.equal(o_r.tot, o_w.tot))
        emit(case="c", what="marginals", long_N=int(counts[nb // 2]), other_N=int(counts[0]), split_ms=round(t_mr, 4), whole_ms=round(t_mw, 4),
             whole_over_split=round(t_mw / t_mr, 3), bit_identical=same)
        emit(case="c", what="loo", long_N=int(counts[nb // 2]), other_N=int(counts[0]), split_ms=round(t_lr, 4), whole_ms=round(t_lw, 4),
             whole_over_split=round(t_lw / t_lr, 3), bit_identical=same)
        del Xp, yp, sp, o_r, o_w
        torch.cuda.empty_cache()
        return rows

    rows = case(128, np.float64) + case(64, np.float32)
    res = dict(tool="tools/marg_ragged_bench.py", device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, preheat_s=PREHEAT_S,
               timer="HIP events, median", rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
