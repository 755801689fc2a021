"""Downdate of a resident state, timed (GPU box): python tools/downdate_bench.py [--quick] [--out FILE]
Times blr_downdate_factor_* per call with HIP events (median of the timed repeats after warm-up; the state is restored from a
copy between repeats, outside the timed region, so every call removes observations the state really holds):
  - B in {1, 256, 2048, 4096} x D in {64, 128} x k in {1, 4, 16}, fp64 and fp32, on the LDS kernel and the global-memory
    kernel (option NO_DOWNDATE_LDS);
  - D in {256, 1024} at B = 1 (global-memory kernel);
  - a sliding-window step at 2048 x D = 128 (update k = 1, then downdate k = 1) against refitting a 4096-observation window
    with blr_posterior_batched_f64.
--quick: only the D = 128, B = 2048, k = 1 fp64 rows (the rocprofv3 --kernel-trace --stats case).  The numbers of DESIGN.md K11."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import blr_amd  # noqa: F401
from blr_amd import _abi as a

dev = torch.device("cuda:0")
h = a.Handle(0)
h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
h.set_async(True)
WARMUP, REPS = 3, 15


def timed(fn, restore, reps=REPS):
    """median ms of fn() over `reps` runs, each after restore() (not timed)"""
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


def state(nb, D, k, dt, seed=1):
    """posterior states that hold the k observations: T'T = U'U + X X' / s, plus the observations"""
    g = torch.Generator(device=dev).manual_seed(seed)
    U = torch.triu(torch.randn((nb, D, D), generator=g, dtype=torch.float64, device=dev)) * (0.3 / np.sqrt(D))
    U = U + torch.diag_embed(1.0 + U.diagonal(dim1=1, dim2=2).abs())
    X = torch.randn((nb, k, D), generator=g, dtype=torch.float64, device=dev) * (0.7 / np.sqrt(k))
    s = 0.5
    A = U.transpose(1, 2) @ U + X.transpose(1, 2) @ X / s
    Tp = torch.linalg.cholesky(A).transpose(1, 2)  # upper
    T0 = Tp.transpose(1, 2).contiguous().to(dt)    # column-major upper factor
    mw0 = torch.randn((nb, D), generator=g, dtype=torch.float64, device=dev).to(dt)
    y = torch.randn((nb, k), generator=g, dtype=torch.float64, device=dev).to(dt)
    return T0, mw0, X.to(dt).contiguous(), y, torch.full((1,), s, dtype=dt, device=dev)


def downdate_row(nb, D, k, ndt, kernel, out):
    dt = torch.float64 if ndt == np.float64 else torch.float32
    h.set_option("NO_DOWNDATE_LDS", "1" if kernel == "global" else None)
    T0, mw0, X, y, s = state(nb, D, k, dt)
    T, mw = T0.clone(), mw0.clone()
    lp = torch.zeros(nb, dtype=torch.float64, device=dev)
    info = torch.zeros(nb, dtype=torch.int32, device=dev)

    def restore():
        T.copy_(T0)
        mw.copy_(mw0)

    def dd():
        h.downdate_factor(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, k, X.data_ptr(), D, k * D, y.data_ptr(), k, a.NOISE_ISOTROPIC,
                          s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())

    ms = timed(dd, restore, REPS if nb > 1 else 30)
    bad = int((info != 0).sum().item())
    row = dict(what="downdate", dtype=np.dtype(ndt).name, kernel=kernel, B=nb, D=D, k=k, ms=round(ms, 5),
               per_s=round(nb / (ms * 1e-3)), failed=bad)
    print(json.dumps(row), flush=True)
    out.append(row)
    h.set_option("NO_DOWNDATE_LDS", None)
    del T0, mw0, X, T, mw
    torch.cuda.empty_cache()


def window_rows(out):
    nb, D, N = 2048, 128, 4096
    ndt, dt = np.float64, torch.float64
    T0, mw0, X, y, s = state(nb, D, 1, dt, seed=2)
    T, mw = T0.clone(), mw0.clone()
    lp = torch.zeros(nb, dtype=torch.float64, device=dev)
    info = torch.zeros(nb, dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(3)
    xn = torch.randn((nb, 1, D), generator=g, dtype=dt, device=dev) * 0.7
    yn = torch.randn((nb, 1), generator=g, dtype=dt, device=dev)

    def restore():
        T.copy_(T0)
        mw.copy_(mw0)

    def step():  # the newest observation in, the oldest out
        h.update_factor(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, 1, xn.data_ptr(), D, D, yn.data_ptr(), 1, a.NOISE_ISOTROPIC,
                        s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())
        h.downdate_factor(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, 1, X.data_ptr(), D, D, y.data_ptr(), 1, a.NOISE_ISOTROPIC,
                          s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())

    def upd():
        h.update_factor(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, 1, xn.data_ptr(), D, D, yn.data_ptr(), 1, a.NOISE_ISOTROPIC,
                        s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())

    t_upd = timed(upd, restore)
    t_step = timed(step, restore)
    bad = int((info != 0).sum().item())
    del T0, mw0, X, T, mw
    torch.cuda.empty_cache()
    # the alternative: refit every window from the prior (N = 4096 observations per regressor)
    Xw = torch.randn((nb, N, D), generator=g, dtype=dt, device=dev)
    yw = torch.randn((nb, N), generator=g, dtype=dt, device=dev)
    U = torch.eye(D, dtype=dt, device=dev).expand(nb, D, D).contiguous()
    m0 = torch.zeros((nb, D), dtype=dt, device=dev)
    mo, To = torch.empty_like(m0), torch.empty_like(U)

    def refit():
        h.posterior_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, Xw.data_ptr(), D, N * D, yw.data_ptr(), N, a.NOISE_ISOTROPIC,
                            s.data_ptr(), 0, a.PRIOR_UPPER_FACTOR, m0.data_ptr(), D, U.data_ptr(), D, D * D, mo.data_ptr(), D,
                            To.data_ptr(), D, D * D, None, D, D * D, lp.data_ptr(), info.data_ptr())

    t_refit = timed(refit, lambda: None, 10)
    row = dict(what="sliding_window", dtype="float64", B=nb, D=D, window=N, update_k1_ms=round(t_upd, 5), step_ms=round(t_step, 5),
               downdate_share_ms=round(t_step - t_upd, 5), refit_ms=round(t_refit, 5), refit_over_step=round(t_refit / t_step, 2),
               failed=bad)
    print(json.dumps(row), flush=True)
    out.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    if args.quick:
        for kernel in ("lds", "global"):
            downdate_row(2048, 128, 1, np.float64, kernel, out)
    else:
        for ndt in (np.float64, np.float32):
            for D in (64, 128):
                for nb in (1, 256, 2048, 4096):
                    for k in (1, 4, 16):
                        for kernel in ("lds", "global"):
                            downdate_row(nb, D, k, ndt, kernel, out)
        for D in (256, 1024):
            for k in (1, 4, 16):
                downdate_row(1, D, k, np.float64, "global", out)
        window_rows(out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, timer="hip events, median", rows=out), f,
                      indent=1)


if __name__ == "__main__":
    main()
