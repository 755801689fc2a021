"""Update / downdate of a resident multi-output state, timed (GPU box): python tools/state_cols_bench.py [--quick] [--out FILE]
Times blr_update_multi_factor_* / blr_downdate_multi_factor_* per call with HIP events (median of 15 calls after 3 warm-up calls; the
state is restored from a copy between repeats, outside the timed region -- the method of tools/downdate_bench.py) against the loop the
call replaces: S calls of the single-column entry point on S private copies of the state (the same library, the same handle):
  - 2048 x D = 128, fp64 and fp32, S in {2, 8, 64}, k in {1, 16, 256}: update, downdate, and at k = 1 the sliding-window pair
    (update k = 1, then downdate k = 1);
  - the pair (fp64) against refitting a 4096-observation window with blr_posterior_multi_batched_f64;
  - one D = 64 row and one B = 64 row (fp64, S = 8, k = 1).
--quick: the fp64 S = 8, k = 1 rows only.  The numbers of DESIGN.md K19."""
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


def state(nb, D, k, S, dt, seed=1):
    """states that hold the k observations (T'T = U'U + X X' / s), S mean columns, the observations, and k fresh ones"""
    g = torch.Generator(device=dev).manual_seed(seed)
    U = torch.triu(torch.randn((nb, D, D), generator=g, dtype=torch.float64, device=dev)) * (0.3 / np.sqrt(D))
    U = U + torch.diag_embed(1.0 + U.diagonal(dim1=1, dim2=2).abs())
    X = torch.randn((nb, k, D), generator=g, dtype=torch.float64, device=dev) * (0.7 / np.sqrt(k))
    s = 0.5
    A = U.transpose(1, 2) @ U + X.transpose(1, 2) @ X / s
    T0 = torch.linalg.cholesky(A).contiguous().to(dt)  # lower, row-major == the upper factor, column-major
    M0 = torch.randn((nb, S, D), generator=g, dtype=torch.float64, device=dev).to(dt)
    Y = torch.randn((nb, S, k), generator=g, dtype=torch.float64, device=dev).to(dt)
    Xn = (torch.randn((nb, k, D), generator=g, dtype=torch.float64, device=dev) * (0.7 / np.sqrt(k))).to(dt)
    Yn = torch.randn((nb, S, k), generator=g, dtype=torch.float64, device=dev).to(dt)
    return T0, M0, X.to(dt).contiguous(), Y, Xn, Yn, torch.full((1,), s, dtype=dt, device=dev)


def rows_for(nb, D, k, S, ndt, out, pair):
    dt = torch.float64 if ndt == np.float64 else torch.float32
    T0, M0, X, Y, Xn, Yn, s = state(nb, D, k, S, dt)
    T, M = T0.clone(), M0.clone()
    lp = torch.zeros((nb, S), dtype=torch.float64, device=dev)
    info = torch.zeros(nb, dtype=torch.int32, device=dev)
    # the loop's private states: S copies of the factor, the means column by column
    Tc0 = T0.unsqueeze(0).expand(S, nb, D, D).contiguous()
    Mc0 = M0.transpose(0, 1).contiguous()   # [S, nb, D]
    Yc, Ync = Y.transpose(0, 1).contiguous(), Yn.transpose(0, 1).contiguous()  # [S, nb, k]
    Tc, Mc = Tc0.clone(), Mc0.clone()
    lpc = torch.zeros((S, nb), dtype=torch.float64, device=dev)

    def restore():
        T.copy_(T0)
        M.copy_(M0)

    def restore_loop():
        Tc.copy_(Tc0)
        Mc.copy_(Mc0)

    def multi(fn, Xa, Ya):
        fn(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, k, S, Xa.data_ptr(), D, k * D, Ya.data_ptr(), k, k * S, a.NOISE_ISOTROPIC, s.data_ptr(), 0,
           M.data_ptr(), D, D * S, T.data_ptr(), D, D * D, lp.data_ptr(), S, info.data_ptr())

    def loop(fn, Xa, Yca):
        for c in range(S):
            fn(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, k, Xa.data_ptr(), D, k * D, Yca[c].data_ptr(), k, a.NOISE_ISOTROPIC, s.data_ptr(), 0,
               Mc[c].data_ptr(), D, Tc[c].data_ptr(), D, D * D, lpc[c].data_ptr(), info.data_ptr())

    cases = [("update", lambda: multi(h.update_multi_factor, Xn, Yn), lambda: loop(h.update_factor, Xn, Ync)),
             ("downdate", lambda: multi(h.downdate_multi_factor, X, Y), lambda: loop(h.downdate_factor, X, Yc))]
    if pair:
        cases.append(("window_pair", lambda: (multi(h.update_multi_factor, Xn, Yn), multi(h.downdate_multi_factor, X, Y)),
                      lambda: (loop(h.update_factor, Xn, Ync), loop(h.downdate_factor, X, Yc))))
    res = {}
    for what, new, old in cases:
        t_new = timed(new, restore)
        bad = int((info != 0).sum().item())
        t_old = timed(old, restore_loop)
        bad += int((info != 0).sum().item())
        row = dict(what=what, dtype=np.dtype(ndt).name, B=nb, D=D, k=k, S=S, multi_ms=round(t_new, 5), loop_ms=round(t_old, 5),
                   loop_over_multi=round(t_old / t_new, 3), failed=bad)
        print(json.dumps(row), flush=True)
        out.append(row)
        res[what] = t_new
    del Tc0, Tc, Mc0, Mc, T0, T, X, Xn
    torch.cuda.empty_cache()
    return res


def refit_row(S, t_pair, out):
    nb, D, N = 2048, 128, 4096
    dt = torch.float64
    g = torch.Generator(device=dev).manual_seed(3)
    Xw = torch.randn((nb, N, D), generator=g, dtype=dt, device=dev)
    Yw = torch.randn((nb, S, N), generator=g, dtype=dt, device=dev)
    U = torch.eye(D, dtype=dt, device=dev).expand(nb, D, D).contiguous()
    m0 = torch.zeros((nb, D), dtype=dt, device=dev)
    s = torch.full((1,), 0.5, dtype=dt, device=dev)
    Mo = torch.empty((nb, S, D), dtype=dt, device=dev)
    To = torch.empty_like(U)
    lp = torch.zeros((nb, S), dtype=torch.float64, device=dev)
    info = torch.zeros(nb, dtype=torch.int32, device=dev)

    def refit():
        h.posterior_multi_batched(np.float64, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, S, Xw.data_ptr(), D, N * D, Yw.data_ptr(), N, N * S,
                                  a.NOISE_ISOTROPIC, s.data_ptr(), 0, a.PRIOR_UPPER_FACTOR, m0.data_ptr(), D, U.data_ptr(), D, D * D,
                                  Mo.data_ptr(), D, D * S, To.data_ptr(), D, D * D, None, D, D * D, lp.data_ptr(), S, info.data_ptr())

    t_refit = timed(refit, lambda: None, 10)
    row = dict(what="refit_window", dtype="float64", B=nb, D=D, S=S, window=N, refit_ms=round(t_refit, 5), pair_ms=round(t_pair, 5),
               refit_over_pair=round(t_refit / t_pair, 2), failed=int((info != 0).sum().item()))
    print(json.dumps(row), flush=True)
    out.append(row)
    del Xw, Yw
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    if args.quick:
        rows_for(2048, 128, 1, 8, np.float64, out, True)
    else:
        for ndt in (np.float64, np.float32):
            for S in (2, 8, 64):
                for k in (1, 16, 256):
                    res = rows_for(2048, 128, k, S, ndt, out, k == 1)
                    if ndt == np.float64 and k == 1:
                        refit_row(S, res["window_pair"], out)
        rows_for(2048, 64, 1, 8, np.float64, out, True)
        rows_for(64, 128, 1, 8, np.float64, out, True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, timer="hip events, median",
                           cols_per_pass=a.STATE_COLS_PER_PASS, rows=out), f, indent=1)


if __name__ == "__main__":
    main()
