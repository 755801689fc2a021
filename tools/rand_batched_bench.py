"""Timing of blr_rand_batched_* (draws from B regressors in one call) against the same work as a loop of single-regressor calls.

Both forms run on device pointers with the handle in async mode and are timed with the handle's device events (blr_timer_*) after
warm-up, alternating in the same process; the loop ends with one synchronise.  Bytes and flops come from the formulas below:
  bytes = w B (D(D+1)/2 + D + DS + [ND unless X is shared] + NS (1 + [Z2]) + [DS if W is returned]) + 4 B
  flops = B (D^2 S + 2 D N S)
Shares are of 8 TB/s (HBM, spec) and of the dense matrix peak (spec: 78.6 TFLOP/s fp64, 157.3 TFLOP/s fp32).

    python tools/rand_batched_bench.py [--reps R] [--shape thompson64|thompson32|c2|dense]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blr_amd  # noqa: E402,F401
from blr_amd import _abi  # noqa: E402

HBM = 8.0e12
PEAK = {np.float64: 78.6e12, np.float32: 157.3e12}

SHAPES = {
    # B, D, N, S, dtype, prior, shared X, noisy (Z2 given), W returned
    "thompson64": (4096, 128, 16, 1, np.float64, _abi.PRIOR_UPPER_FACTOR, True, False, False),
    "thompson32": (4096, 128, 16, 1, np.float32, _abi.PRIOR_UPPER_FACTOR, True, False, False),
    "c2": (256, 128, 4096, 16, np.float64, _abi.PRIOR_UPPER_FACTOR, False, True, False),
    "dense": (1024, 64, 256, 8, np.float32, _abi.PRIOR_DENSE, False, True, False),
}


def traffic(B, D, N, S, w, shared, noisy, want_w):
    return w * B * (D * (D + 1) // 2 + D + D * S + (0 if shared else N * D) + N * S * (1 + int(noisy)) + (D * S if want_w else 0)) + 4 * B


def flops(B, D, N, S):
    return B * (D * D * S + 2 * D * N * S)


def run(name, reps):
    B, D, N, S, dt, prior, shared, noisy, want_w = SHAPES[name]
    tdt = torch.float64 if dt == np.float64 else torch.float32
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(17)
    X = torch.randn((1 if shared else B, N, D), generator=g, dtype=tdt, device=dev) / D ** 0.5  # ColVecs: D x N column-major
    A = torch.randn((B, D, D), generator=g, dtype=torch.float64, device=dev) / D ** 0.5
    P = A @ A.transpose(1, 2) + torch.eye(D, dtype=torch.float64, device=dev)
    if prior == _abi.PRIOR_UPPER_FACTOR:
        L = torch.linalg.cholesky(P, upper=True).transpose(1, 2).to(tdt).contiguous()  # column-major upper factor
    else:
        L = P.to(tdt).contiguous()
    mw = torch.randn((B, D), generator=g, dtype=tdt, device=dev)
    s = torch.full((B, 1), 0.1, dtype=tdt, device=dev)
    Z1 = torch.randn((B, S, D), generator=g, dtype=tdt, device=dev)
    Z2 = torch.randn((B, S, N), generator=g, dtype=tdt, device=dev) if noisy else None
    Y = torch.empty((B, S, N), dtype=tdt, device=dev)
    Yl = torch.empty((B, S, N), dtype=tdt, device=dev)
    Wl = torch.empty((B, S, D), dtype=tdt, device=dev)  # the loop's weights (Thompson: sample, then apply)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    h = _abi.default_handle()
    torch.cuda.synchronize()  # the operands were written on torch's stream; the library runs on its handle's own stream
    sX = 0 if shared else N * D
    z2p = Z2.data_ptr() if noisy else None
    w = np.dtype(dt).itemsize

    def batched():
        h.rand_batched(dt, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, B, D, N, S, X.data_ptr(), D, sX, _abi.NOISE_ISOTROPIC, s.data_ptr(), 1,
                       prior, mw.data_ptr(), D, L.data_ptr(), D, D * D, Z1.data_ptr(), D, D * S, z2p, N, N * S, None, D, D * S,
                       Y.data_ptr(), N, N * S, info.data_ptr())

    def loop():
        for b in range(B):
            xb = X.data_ptr() + (0 if shared else b * N * D * w)
            Lb, mb, z1 = L.data_ptr() + b * D * D * w, mw.data_ptr() + b * D * w, Z1.data_ptr() + b * D * S * w
            yb = Yl.data_ptr() + b * N * S * w
            if noisy:
                h.rand(dt, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, D, N, S, xb, D, _abi.NOISE_ISOTROPIC, s.data_ptr() + b * w, prior, mb, Lb, D,
                       z1, D, Z2.data_ptr() + b * N * S * w, N, yb, N)
            else:
                wb = Wl.data_ptr() + b * D * S * w
                h.sample_weights(dt, _abi.MEM_DEVICE, D, S, prior, mb, Lb, D, z1, D, wb, D)
                h.apply_weights(dt, _abi.MEM_DEVICE, _abi.LAYOUT_COLVECS, D, N, S, xb, D, wb, D, yb, N)

    h.set_async(1)
    try:
        for _ in range(3):
            batched()
        loop()
        h.synchronize()
        tb, tl = [], []
        for _ in range(reps):
            h.timer_start()
            batched()
            tb.append(h.timer_stop())
            h.timer_start()
            loop()
            tl.append(h.timer_stop())  # (the stop event is recorded behind the loop's last launch; timer_stop synchronises on it)
        h.synchronize()
    finally:
        h.set_async(0)
    assert int(info.abs().sum()) == 0
    # the two forms compute the same draws (different kernels: compared to the tolerance of the element type)
    ref = Yl.double()
    err = float((Y.double() - ref).abs().max() / ref.abs().max().clamp(min=1.0))
    ms_b, ms_l = float(np.median(tb)), float(np.median(tl))
    nbytes, nflops = traffic(B, D, N, S, w, shared, noisy, want_w), flops(B, D, N, S)
    t = ms_b * 1e-3
    rec = dict(shape=name, B=B, D=D, N=N, S=S, dtype=np.dtype(dt).name, ms=round(ms_b, 4), ms_min=round(min(tb), 4),
               ms_loop=round(ms_l, 3), speedup=round(ms_l / ms_b, 1), bytes=nbytes, flops=nflops,
               hbm_share=round(nbytes / t / HBM, 3), matrix_share=round(nflops / t / PEAK[dt], 4), max_rel_diff_vs_loop=err)
    print(f"{name:11s} B={B} D={D} N={N} S={S} {np.dtype(dt).name}: batched {ms_b:.4f} ms (min {min(tb):.4f}), loop {ms_l:.2f} ms, "
          f"x{ms_l / ms_b:.1f}; {nbytes / 1e9:.3f} GB -> {nbytes / t / 1e12:.2f} TB/s = {nbytes / t / HBM:.3f} of 8 TB/s; "
          f"{nflops / t / 1e12:.2f} TFLOP/s = {nflops / t / PEAK[dt]:.4f} of the matrix peak; max rel diff vs loop {err:.1e}")
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", action="append", choices=sorted(SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: this tool measures on the device only")
    for name in args.shape or list(SHAPES):
        run(name, args.reps)


if __name__ == "__main__":
    main()
