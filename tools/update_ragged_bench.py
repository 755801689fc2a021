"""Ragged condition / forget on resident states, timed (GPU box): python tools/update_ragged_bench.py [--out FILE]
Times blr_update_factor_ragged_* / blr_downdate_factor_ragged_* per call with HIP events (median of the timed repeats after warm-up;
the states are restored from a copy between repeats, outside the timed region, so every downdate removes observations the state
really holds) against what a caller has without them, for both directions, fp64 and fp32, D = 128:
  (a) k_b = 1 for all of 2048 regressors         against ONE blr_update_factor_* / blr_downdate_factor_* call at k = 1;
  (b) a bandit round: 4096 resident, 256 of them with k_b = 1
                                                  against the loop of 256 calls with B = 1 on the active states;
  (c) k_b geometric with mean 2 over 4096        against gather (states and slices of every distinct k into contiguous
                                                  copies), one equal-count call per distinct k, scatter back.
ratio = baseline / ragged: above 1 the ragged call wins.  The numbers of DESIGN.md K29 (profiles/update_ragged_bench.json)."""
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
WARMUP, REPS = 2, 9
D = 128
S = 0.5


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


def problem(counts, dt, seed):
    """nb resident states that hold their own slice of the packed observations: T'T = U'U + X_b X_b' / s"""
    nb, total = len(counts), int(np.sum(counts))
    g = torch.Generator(device=dev).manual_seed(seed)
    U = torch.triu(torch.randn((nb, D, D), generator=g, dtype=torch.float64, device=dev)) * (0.3 / np.sqrt(D))
    U = U + torch.diag_embed(1.0 + U.diagonal(dim1=1, dim2=2).abs())
    X = torch.randn((total, D), generator=g, dtype=torch.float64, device=dev) * 0.7  # [total, D] row-major == D x total ColVecs
    owner = torch.tensor(np.repeat(np.arange(nb), counts), device=dev)
    A = U.transpose(1, 2) @ U
    for lo in range(0, total, 1024):  # (outer products in slabs)
        x = X[lo:lo + 1024]
        A.index_add_(0, owner[lo:lo + 1024], x[:, :, None] * x[:, None, :] / S)
    T0 = torch.linalg.cholesky(A).contiguous().to(dt)  # lower factor row-major == column-major upper factor
    mw0 = torch.randn((nb, D), generator=g, dtype=torch.float64, device=dev).to(dt)
    y = torch.randn(total, generator=g, dtype=torch.float64, device=dev).to(dt)
    return T0, mw0, X.to(dt).contiguous(), y, torch.full((1,), S, dtype=dt, device=dev)


def bench_case(case, direction, ndt, out):
    dt = torch.float64 if ndt == np.float64 else torch.float32
    rng = np.random.Generator(np.random.PCG64(7))
    if case == "a_all_k1":
        counts = np.ones(2048, dtype=np.int64)
    elif case == "b_bandit_256_of_4096":
        counts = np.zeros(4096, dtype=np.int64)
        counts[rng.choice(4096, size=256, replace=False)] = 1
    else:
        counts = rng.geometric(0.5, size=4096).astype(np.int64)
    nb = len(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    T0, mw0, X, y, s = problem(counts, dt, 11)
    T, mw = T0.clone(), mw0.clone()
    lp = torch.zeros(nb, dtype=torch.float64, device=dev)
    info = torch.zeros(nb, dtype=torch.int32, device=dev)
    item = X.element_size()
    ragged_fn = h.update_factor_ragged if direction == "update" else h.downdate_factor_ragged
    equal_fn = h.update_factor if direction == "update" else h.downdate_factor

    def restore():
        T.copy_(T0)
        mw.copy_(mw0)

    def ragged():
        ragged_fn(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, offsets, X.data_ptr(), D, y.data_ptr(), a.NOISE_ISOTROPIC, s.data_ptr(), 0,
                  mw.data_ptr(), D, T.data_ptr(), D, D * D, lp.data_ptr(), info.data_ptr())

    def equal(n, k, Xp, yp, mwp, Tp, lpp, infop):
        equal_fn(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, n, D, k, Xp, D, k * D, yp, k, a.NOISE_ISOTROPIC, s.data_ptr(), 0, mwp, D, Tp, D, D * D,
                 lpp, infop)

    if case == "a_all_k1":
        def baseline():
            equal(nb, 1, X.data_ptr(), y.data_ptr(), mw.data_ptr(), T.data_ptr(), lp.data_ptr(), info.data_ptr())
        what = "one equal-count call, k = 1"
    elif case == "b_bandit_256_of_4096":
        active = np.flatnonzero(counts)

        def baseline():
            for b in active:
                o = int(offsets[b])
                equal(1, 1, X.data_ptr() + o * D * item, y.data_ptr() + o * item, mw.data_ptr() + int(b) * D * item,
                      T.data_ptr() + int(b) * D * D * item, lp.data_ptr() + int(b) * 8, info.data_ptr() + int(b) * 4)
        what = "loop of 256 calls with B = 1"
    else:
        groups = []
        for k in np.unique(counts):
            regs = np.flatnonzero(counts == k)
            cols = (offsets[regs][:, None] + np.arange(k)[None, :]).reshape(-1)
            groups.append((int(k), torch.tensor(regs, device=dev), torch.tensor(cols, device=dev)))

        def baseline():
            for k, regs, cols in groups:  # gather, one call per distinct k, scatter
                n = regs.numel()
                Tg, mg, Xg, yg = T.index_select(0, regs), mw.index_select(0, regs), X.index_select(0, cols), y.index_select(0, cols)
                lg, ig = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
                equal(n, k, Xg.data_ptr(), yg.data_ptr(), mg.data_ptr(), Tg.data_ptr(), lg.data_ptr(), ig.data_ptr())
                T.index_copy_(0, regs, Tg)
                mw.index_copy_(0, regs, mg)
                lp.index_copy_(0, regs, lg)
                info.index_copy_(0, regs, ig)
        what = f"gather, {len(groups)} equal-count calls (one per distinct k), scatter"

    t_ragged = timed(ragged, restore)
    bad_r = int((info != 0).sum().item())
    lists = [h.get_stat(k) for k in ("ragged_sweep", "ragged_refit", "ragged_idle")]
    t_base = timed(baseline, restore, REPS if case != "b_bandit_256_of_4096" else 5)
    bad_b = int((info != 0).sum().item())
    ratio = t_base / t_ragged
    row = dict(case=case, direction=direction, dtype=np.dtype(ndt).name, B=nb, D=D, observations=int(offsets[-1]), max_k=int(counts.max()),
               lists_sweep_refit_idle=lists, ragged_ms=round(t_ragged, 5), baseline=what, baseline_ms=round(t_base, 5), ratio=round(ratio, 3),
               verdict="win" if ratio > 1.03 else ("miss" if ratio < 0.97 else "equal within 3 %"), failed_ragged=bad_r, failed_baseline=bad_b)
    print(json.dumps(row), flush=True)
    out.append(row)
    del T0, mw0, X, T, mw
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    for ndt in (np.float64, np.float32):
        for direction in ("update", "downdate"):
            for case in ("a_all_k1", "b_bandit_256_of_4096", "c_geometric_mean_2"):
                bench_case(case, direction, ndt, out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, timer="hip events, median", rows=out), f, indent=1)


if __name__ == "__main__":
    main()
