"""blr_posterior_batched_x16 against its yardstick, timed (GPU box): python tools/x16_bench.py [--out FILE]
Rows: 4096 x (D = 128, N = 4096) and 8192 x (D = 64, N = 1024), isotropic noise, diagonal prior, posterior mean + factor + evidence,
everything device resident, aligned ColVecs and RowVecs, bf16 and fp16.  Per row, back to back in one process: the 16-bit call,
blr_posterior_batched_f32 on the widened features, and the widening pass itself (a device-side cast that writes the fp32 copy).
Pre-heated (3 calls), then 10 calls timed with blr_timer_*, median.  The algorithmic bytes are the 16-bit X, y and the outputs.
Writes profiles/x16_bench.json by default.  The numbers of DESIGN.md K31."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS = 3, 10
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "x16_bench.json"))
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn):
        ts = []
        for i in range(WARMUP + REPS):
            h.timer_start()
            fn()
            ts.append(h.timer_stop())
        return float(np.median(ts[WARMUP:]))

    rows = []
    for B, D, N in ((4096, 128, 4096), (8192, 64, 1024)):
        gen = torch.Generator(device=dev).manual_seed(1234)
        y = torch.randn((B, N), device=dev, dtype=torch.float32, generator=gen)
        s = torch.full((1,), 0.1, device=dev, dtype=torch.float32)
        mw = torch.zeros((B, D), device=dev, dtype=torch.float32)
        Lw = torch.exp(0.3 * torch.randn((B, D), device=dev, dtype=torch.float32, generator=gen))
        mw_post = torch.empty((B, D), device=dev, dtype=torch.float32)
        T = torch.empty((B, D * D), device=dev, dtype=torch.float32)
        lp = torch.empty((B,), device=dev, dtype=torch.float64)
        info = torch.empty((B,), device=dev, dtype=torch.int32)
        for fmt, tdt, xfmt in (("bf16", torch.bfloat16, a.X_BF16), ("f16", torch.float16, a.X_F16)):
            for lname, layout in (("ColVecs", a.LAYOUT_COLVECS), ("RowVecs", a.LAYOUT_ROWVECS)):
                # ColVecs: [B][N][D] row-major = D x N column-major per regressor; RowVecs: [B][D][N] = N x D column-major
                shape = (B, N, D) if layout == a.LAYOUT_COLVECS else (B, D, N)
                ldx = D if layout == a.LAYOUT_COLVECS else N
                X16 = torch.randn(shape, device=dev, dtype=torch.float32, generator=gen).to(tdt)
                X32 = X16.to(torch.float32)

                def call16():
                    h.posterior_batched_x16(xfmt, a.MEM_DEVICE, layout, B, D, N, X16.data_ptr(), ldx, D * N, y.data_ptr(), N, a.NOISE_ISOTROPIC,
                                            s.data_ptr(), 0, a.PRIOR_DIAGONAL, mw.data_ptr(), D, Lw.data_ptr(), 1, D, mw_post.data_ptr(), D,
                                            T.data_ptr(), D, D * D, None, D, D * D, lp.data_ptr(), info.data_ptr())

                def call32():
                    h.posterior_batched(np.float32, a.MEM_DEVICE, layout, B, D, N, X32.data_ptr(), ldx, D * N, y.data_ptr(), N, a.NOISE_ISOTROPIC,
                                        s.data_ptr(), 0, a.PRIOR_DIAGONAL, mw.data_ptr(), D, Lw.data_ptr(), 1, D, mw_post.data_ptr(), D,
                                        T.data_ptr(), D, D * D, None, D, D * D, lp.data_ptr(), info.data_ptr())

                def widen():
                    X32.copy_(X16)

                t16 = timed(call16)
                route16 = h.last_route()
                lp16 = lp.clone()
                assert int(info.abs().max()) == 0
                t32 = timed(call32)
                route32 = h.last_route()
                tw = timed(widen)
                rel = float(((lp16 - lp).abs() / lp.abs()).max())
                bytes16 = B * (2 * D * N + 4 * N + 4 * D + 4 * D * D + 4 * D + 12)
                rows.append(dict(B=B, D=D, N=N, fmt=fmt, layout=lname, route_x16=route16, route_f32=route32, ms_x16=t16, ms_f32=t32,
                                 ms_widen=tw, updates_per_s_x16=B / (t16 * 1e-3), updates_per_s_f32=B / (t32 * 1e-3),
                                 updates_per_s_f32_with_widen=B / ((t32 + tw) * 1e-3), algorithmic_bytes_x16=bytes16,
                                 tb_per_s_x16=bytes16 / (t16 * 1e-3) / 1e12, fraction_of_8tbs=bytes16 / (t16 * 1e-3) / HBM_PEAK,
                                 max_rel_evidence_difference=rel))
                print(json.dumps(rows[-1]), flush=True)
                del X16, X32
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/x16_bench.py", warmup=WARMUP, reps=REPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
