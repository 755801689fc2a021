"""Regressors with unequal observation counts, timed (GPU box): python tools/ragged_bench.py [--quick] [--out FILE]
Times blr_posterior_ragged_* (mw', T, evidence; device memspace) with HIP events -- about two seconds of untimed calls first
(clocks settle), then 3 warm-up + 15 timed calls, median -- at D = 128 fp64 and D = 64 fp32 with 4096 regressors:
  (a) every N_b = 1024 through the ragged call against blr_posterior_batched_* on a handle with NO_I8_GRAM = 1,
      NO_WAVE_KERNEL = 1: the same kernel body, isotropic noise;
  (b) N_b log-uniform in [16, 4096], diagonal noise, three routes to the same numbers: the ragged call; the equal-count call
      on every regressor padded to max N_b with x = 0, y = 0, s = 1 columns (evidence corrected by 1/2 log 2 pi per padded
      column); a loop of B = 1 calls over a sample of 64 regressors, scaled to the batch.  Also the ragged call's fraction of
      8 TB/s by its algorithmic bytes (X, y, s once; mw, Lw in; mw', T out);
  (c) the counts of (b) in ascending and in descending order: the host orders the regressors itself, the times must agree.
--quick: 256 regressors (a smoke run of the tool).
The numbers of DESIGN.md K14."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS, PREHEAT_S = 3, 15, 2.0
HBM_BYTES_PER_S = 8e12


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
    h_eq = handle(NO_I8_GRAM="1", NO_WAVE_KERNEL="1")  # the equal-count entry point on the phases the ragged kernel runs
    nb = 256 if args.quick else 4096
    p = lambda t: t.data_ptr()  # noqa: E731

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn, preheat=True):
        t, spent = once(fn), 0.0
        while preheat and spent < PREHEAT_S * 1e3:
            spent += once(fn)
        ts = [once(fn) for _ in range(WARMUP + REPS)]
        return float(np.median(ts[WARMUP:])), t

    def outputs(D, tdt):
        return (torch.zeros((nb, D), device=dev, dtype=tdt), torch.zeros((nb, D, D), device=dev, dtype=tdt),
                torch.zeros(nb, device=dev, dtype=torch.float64), torch.zeros(nb, device=dev, dtype=torch.int32))

    def ragged_call(dtype, D, offsets, X, y, nk, s, strides, mw, Lw, out):
        mwp, Tp, lp, info = out
        return lambda: h.posterior_ragged(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, offsets, p(X), D, p(y), nk, p(s), strides,
                                          a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, p(mwp), D, p(Tp), D, D * D, None, D, D * D, p(lp), p(info))

    def batched_call(hd, dtype, B, D, N, X, y, nk, s, strides, mw, Lw, out, first=0):
        mwp, Tp, lp, info = out
        it = 8 if dtype == np.float64 else 4
        return lambda: hd.posterior_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, p(X), D, D * N, p(y), N, nk, p(s), strides,
                                            a.PRIOR_DIAGONAL, p(mw) + first * D * it, D, p(Lw) + first * D * it, 1, D, p(mwp) + first * D * it, D,
                                            p(Tp) + first * D * D * it, D, D * D, None, D, D * D, p(lp) + first * 8, p(info) + first * 4)

    def case(D, dtype):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        it = 8 if dtype == np.float64 else 4
        gen = torch.Generator(device=dev).manual_seed(4321)
        mw = 0.1 * torch.randn((nb, D), device=dev, dtype=tdt, generator=gen)
        Lw = torch.exp(0.3 * torch.randn((nb, D), device=dev, dtype=tdt, generator=gen))
        rows = []

        # ---- (a) equal counts: the ragged call against the equal-count call, the same kernel body ----------------------------
        N = 1024
        X = torch.randn((nb, N, D), device=dev, dtype=tdt, generator=gen)
        y = torch.randn((nb, N), device=dev, dtype=tdt, generator=gen)
        s = torch.full((1,), 0.1, device=dev, dtype=tdt)
        o_r, o_b = outputs(D, tdt), outputs(D, tdt)
        off = np.arange(nb + 1, dtype=np.int64) * N
        t_r, _ = timed(ragged_call(dtype, D, off, X, y, a.NOISE_ISOTROPIC, s, 0, mw, Lw, o_r))
        route_r = h.last_route()
        t_b, _ = timed(batched_call(h_eq, dtype, nb, D, N, X, y, a.NOISE_ISOTROPIC, s, 0, mw, Lw, o_b))
        route_b = h_eq.last_route()
        torch.cuda.synchronize()
        assert int(o_r[3].abs().sum()) == 0 and int(o_b[3].abs().sum()) == 0
        same = bool(torch.equal(o_r[0], o_b[0]) and torch.equal(o_r[1], o_b[1]) and torch.equal(o_r[2], o_b[2]))
        rows.append(dict(case="a", D=D, dtype=np.dtype(dtype).name, B=nb, N=N, ragged_ms=round(t_r, 4), batched_ms=round(t_b, 4),
                         ragged_over_batched=round(t_r / t_b, 4), bit_identical=same, ragged_route=route_r, batched_route=route_b))
        print(json.dumps(rows[-1]), flush=True)
        del X, y

        # ---- (b) log-uniform counts: ragged, padded to the longest, a loop of single calls ---------------------------------------
        rng = np.random.Generator(np.random.PCG64(99))
        counts = np.floor(np.exp(rng.uniform(math.log(16), math.log(4096 + 1), size=nb))).astype(np.int64).clip(16, 4096)
        nmax, total = int(counts.max()), int(counts.sum())
        cnt_d = torch.tensor(counts, device=dev)
        mask = torch.arange(nmax, device=dev)[None, :] < cnt_d[:, None]          # [B, nmax]
        Xpad = torch.randn((nb, nmax, D), device=dev, dtype=tdt, generator=gen)
        Xpad *= mask[:, :, None]
        ypad = torch.randn((nb, nmax), device=dev, dtype=tdt, generator=gen) * mask
        spad = torch.where(mask, torch.exp(0.3 * torch.randn((nb, nmax), device=dev, dtype=tdt, generator=gen)), torch.ones((), device=dev, dtype=tdt))
        Xp, yp, sp = Xpad[mask].contiguous(), ypad[mask].contiguous(), spad[mask].contiguous()  # regressor after regressor: [total, D]
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        o_r, o_p, o_l = outputs(D, tdt), outputs(D, tdt), outputs(D, tdt)
        t_r, _ = timed(ragged_call(dtype, D, off, Xp, yp, a.NOISE_DIAGONAL, sp, 0, mw, Lw, o_r))
        t_p, _ = timed(batched_call(h, dtype, nb, D, nmax, Xpad, ypad, a.NOISE_DIAGONAL, spad, nmax, mw, Lw, o_p))
        route_p = h.last_route()
        sample = rng.choice(nb, size=min(64, nb), replace=False)
        singles = [batched_call(h, dtype, 1, D, int(counts[b]), Xp[off[b]:], yp[off[b]:], a.NOISE_DIAGONAL, sp[off[b]:], 0, mw, Lw, o_l, first=int(b))
                   for b in sample]
        t_l, _ = timed(lambda: [f() for f in singles], preheat=False)
        t_l *= nb / len(sample)
        torch.cuda.synchronize()
        assert int(o_r[3].abs().sum()) == 0 and int(o_p[3].abs().sum()) == 0
        lp_pad = o_p[2] + 0.5 * math.log(2 * math.pi) * (nmax - cnt_d).to(torch.float64)
        rel = float(((o_r[2] - lp_pad).abs() / o_r[2].abs()).max())
        byts = total * (D + 2) * it + nb * (D * D + 3 * D) * it
        rows.append(dict(case="b", D=D, dtype=np.dtype(dtype).name, B=nb, counts="log-uniform in [16, 4096]", max_N=nmax, mean_N=round(total / nb, 1),
                         padding_ratio=round(nmax * nb / total, 3), ragged_ms=round(t_r, 4), padded_ms=round(t_p, 4), loop_ms_scaled=round(t_l, 2),
                         loop_sample=len(sample), padded_over_ragged=round(t_p / t_r, 3), loop_over_ragged=round(t_l / t_r, 1),
                         ragged_bytes=byts, ragged_fraction_of_8TBs=round(byts / (t_r * 1e-3) / HBM_BYTES_PER_S, 4),
                         max_rel_diff_evidence_vs_padded=rel, padded_route=route_p))
        print(json.dumps(rows[-1]), flush=True)
        del Xpad, ypad, spad

        # ---- (c) the same counts sorted: the host orders the regressors itself ---------------------------------------------------
        # (the columns are i.i.d.: another order of the counts is another set of offsets into the same packed arrays)
        res = {}
        for name, c in (("ascending", np.sort(counts)), ("descending", np.sort(counts)[::-1])):
            off_c = np.concatenate(([0], np.cumsum(c))).astype(np.int64)
            res[name], _ = timed(ragged_call(dtype, D, off_c, Xp, yp, a.NOISE_DIAGONAL, sp, 0, mw, Lw, o_r))
        torch.cuda.synchronize()
        assert int(o_r[3].abs().sum()) == 0
        rows.append(dict(case="c", D=D, dtype=np.dtype(dtype).name, B=nb, ascending_ms=round(res["ascending"], 4),
                         descending_ms=round(res["descending"], 4), as_drawn_ms=round(t_r, 4),
                         ascending_over_descending=round(res["ascending"] / res["descending"], 4)))
        print(json.dumps(rows[-1]), flush=True)
        del Xp, yp, sp
        torch.cuda.empty_cache()
        return rows

    rows = case(128, np.float64) + case(64, np.float32)
    res = dict(tool="tools/ragged_bench.py", device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, preheat_s=PREHEAT_S,
               timer="HIP events, median", rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
