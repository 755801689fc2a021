"""blr_posterior_multi_batched_x16 against its alternatives, timed (GPU box): python tools/x16_multi_bench.py [--out FILE]
Rows: 4096 x (D = 128, N = 4096) with S in {2, 8, 64} and 8192 x (D = 64, N = 1024) with S = 8, isotropic noise, diagonal prior, means +
factor + evidences, everything device resident, aligned ColVecs and RowVecs, bf16 and fp16.  Per row, back to back in one process: the
multi-output 16-bit call, a loop of S blr_posterior_batched_x16 calls, blr_posterior_multi_batched_f32 on the widened features, and the
widening pass itself (a device-side cast that writes the fp32 copy).  Pre-heated (3 calls), then 10 calls timed with blr_timer_*,
median.  Writes profiles/x16_multi_bench.json by default.  The numbers of DESIGN.md K33."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS = 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "x16_multi_bench.json"))
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
    for B, D, N, Ss in ((4096, 128, 4096, (2, 8, 64)), (8192, 64, 1024, (8,))):
        gen = torch.Generator(device=dev).manual_seed(1234)
        s = torch.full((1,), 0.1, device=dev, dtype=torch.float32)
        mw = torch.zeros((B, D), device=dev, dtype=torch.float32)
        Lw = torch.exp(0.3 * torch.randn((B, D), device=dev, dtype=torch.float32, generator=gen))
        T = torch.empty((B, D * D), device=dev, dtype=torch.float32)
        info = torch.empty((B,), device=dev, dtype=torch.int32)
        for fmt, tdt, xfmt in (("bf16", torch.bfloat16, a.X_BF16), ("f16", torch.float16, a.X_F16)):
            for lname, layout in (("ColVecs", a.LAYOUT_COLVECS), ("RowVecs", a.LAYOUT_ROWVECS)):
                shape = (B, N, D) if layout == a.LAYOUT_COLVECS else (B, D, N)
                ldx = D if layout == a.LAYOUT_COLVECS else N
                X16 = torch.randn(shape, device=dev, dtype=torch.float32, generator=gen).to(tdt)
                X32 = X16.to(torch.float32)
                for S in Ss:
                    Y = torch.randn((B, S, N), device=dev, dtype=torch.float32, generator=gen)  # N x S column-major per regressor
                    M = torch.empty((B, S * D), device=dev, dtype=torch.float32)
                    lp = torch.empty((B, S), device=dev, dtype=torch.float64)
                    m1 = torch.empty((B, D), device=dev, dtype=torch.float32)
                    lp1 = torch.empty((B,), device=dev, dtype=torch.float64)
                    p = lambda t: t.data_ptr()  # noqa: E731

                    def multi16():
                        h.posterior_multi_batched_x16(xfmt, a.MEM_DEVICE, layout, B, D, N, S, p(X16), ldx, D * N, p(Y), N, S * N, a.NOISE_ISOTROPIC,
                                                      p(s), 0, a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, p(M), D, S * D, p(T), D, D * D, None, D,
                                                      D * D, p(lp), S, p(info))

                    def loop16():
                        for c in range(S):
                            h.posterior_batched_x16(xfmt, a.MEM_DEVICE, layout, B, D, N, p(X16), ldx, D * N, p(Y) + 4 * c * N, S * N,
                                                    a.NOISE_ISOTROPIC, p(s), 0, a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, p(m1), D, p(T), D, D * D,
                                                    None, D, D * D, p(lp1), p(info))

                    def multi32():
                        h.posterior_multi_batched(np.float32, a.MEM_DEVICE, layout, B, D, N, S, p(X32), ldx, D * N, p(Y), N, S * N,
                                                  a.NOISE_ISOTROPIC, p(s), 0, a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, p(M), D, S * D, p(T), D,
                                                  D * D, None, D, D * D, p(lp), S, p(info))

                    def widen():
                        X32.copy_(X16)

                    t16 = timed(multi16)
                    route = h.last_route()
                    row = dict(B=B, D=D, N=N, S=S, fmt=fmt, layout=lname, route=route, multi_x16_ms=t16, loop_x16_ms=timed(loop16),
                               multi_f32_ms=timed(multi32), widen_ms=timed(widen))
                    row["x16_bytes_per_s"] = (2.0 * B * D * N * (1 + -(-(S - 1) // 63)) + 4.0 * B * S * N) / (t16 * 1e-3)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del Y, M, lp
                del X16, X32
    with open(args.out, "w") as f:
        json.dump(dict(warmup=WARMUP, reps=REPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
