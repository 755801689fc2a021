"""blr_loo_batched_x16 against its yardsticks, timed (GPU box): python tools/x16_loo_bench.py [--out FILE]
Rows: 64 x (D = 128, N = 4096) and 4096 x (128, 4096), a state (mw, T), isotropic noise, all four outputs, everything device resident,
aligned ColVecs and RowVecs, bf16 and fp16.  Per row, back to back in one process: the 16-bit call, (a) blr_loo_batched_f32 on the
widened inputs and the widening pass itself (a device-side cast that writes the fp32 copy), (b) blr_marginals_batched_x16 mean + var
with T as an upper-factor prior at the same shape.  Pre-heated (3 calls), then 10 calls timed with blr_timer_*, median.  Writes
profiles/x16_loo_bench.json by default.  The numbers of DESIGN.md K35."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS = 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "x16_loo_bench.json"))
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
    D, N = 128, 4096
    for B in (64, 4096):
        gen = torch.Generator(device=dev).manual_seed(1234)
        s = torch.full((1,), 1024.0, device=dev, dtype=torch.float32)  # above every sigma2_n: no degenerate observation
        mw = torch.randn((B, D), device=dev, dtype=torch.float32, generator=gen)
        y = torch.randn((B, N), device=dev, dtype=torch.float32, generator=gen)
        # [B][i][j] row-major lower = column-major UPPER factor per regressor
        T = torch.tril(0.05 * torch.randn((B, D, D), device=dev, dtype=torch.float32, generator=gen), -1) + torch.eye(D, device=dev)
        lm, lv = (torch.empty((B, N), device=dev, dtype=torch.float32) for _ in range(2))
        ll, tot = torch.empty((B, N), device=dev, dtype=torch.float64), torch.empty((B,), device=dev, dtype=torch.float64)
        info = torch.empty((B,), device=dev, dtype=torch.int32)
        for fmt, tdt, xfmt in (("bf16", torch.bfloat16, a.X_BF16), ("f16", torch.float16, a.X_F16)):
            for lname, layout in (("ColVecs", a.LAYOUT_COLVECS), ("RowVecs", a.LAYOUT_ROWVECS)):
                shape = (B, N, D) if layout == a.LAYOUT_COLVECS else (B, D, N)
                ldx = D if layout == a.LAYOUT_COLVECS else N
                X16 = torch.randn(shape, device=dev, dtype=torch.float32, generator=gen).to(tdt)
                X32 = X16.to(torch.float32)
                tail = (y.data_ptr(), N, a.NOISE_ISOTROPIC, s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, lm.data_ptr(), N, lv.data_ptr(), N,
                        ll.data_ptr(), N, tot.data_ptr(), info.data_ptr())

                def loo16():
                    h.loo_batched_x16(xfmt, a.MEM_DEVICE, layout, B, D, N, X16.data_ptr(), ldx, D * N, *tail)

                def loo32():
                    h.loo(np.float32, a.MEM_DEVICE, layout, B, D, N, X32.data_ptr(), ldx, D * N, *tail)

                def marg16():
                    h.marginals_batched_x16(xfmt, a.MEM_DEVICE, layout, B, D, N, X16.data_ptr(), ldx, D * N, a.NOISE_ISOTROPIC, s.data_ptr(), 0,
                                            a.PRIOR_UPPER_FACTOR, mw.data_ptr(), D, T.data_ptr(), D, D * D, lm.data_ptr(), N, lv.data_ptr(), N,
                                            info.data_ptr())

                def widen():
                    X32.copy_(X16)

                t16 = timed(loo16)
                route16 = h.last_route()
                got = [x.clone() for x in (lm, lv, ll, tot)]
                t32 = timed(loo32)
                torch.cuda.synchronize()
                rel = [float((g - x).abs().max() / x.abs().max()) for g, x in zip(got, (lm, lv, ll, tot))]
                tm, tw = timed(marg16), timed(widen)
                torch.cuda.synchronize()
                rows.append(dict(B=B, D=D, N=N, fmt=fmt, layout=lname, route_x16=route16, ms_loo_x16=t16, ms_loo_f32=t32, ms_widen=tw, ms_marginals_x16=tm,
                                 ginputs_per_s_loo_x16=B * N / (t16 * 1e-3) / 1e9, ginputs_per_s_loo_f32=B * N / (t32 * 1e-3) / 1e9,
                                 ginputs_per_s_marginals_x16=B * N / (tm * 1e-3) / 1e9, ratio_to_f32=t32 / t16, ratio_to_f32_with_widen=(t32 + tw) / t16,
                                 ratio_to_marginals_x16=t16 / tm, max_rel_difference_to_f32=dict(zip(("mean", "var", "logpdf", "total"), rel))))
                print(json.dumps(rows[-1]), flush=True)
                del X16, X32
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/x16_loo_bench.py", warmup=WARMUP, reps=REPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
