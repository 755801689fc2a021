"""Evidence over a hyperparameter grid, timed (GPU box): python tools/grid_bench.py [--quick] [--out FILE]
Times blr_logpdf_grid_* (evidence of every setting, argmax, posterior at the winner) with HIP events -- 3 warm-up + 15 timed
calls, median -- against the way to the same numbers without it, in the same process:
  (a) one data set (128, 4096) fp64, isotropic noise, diagonal prior, G in {64, 1024}: blr_posterior_batched_f64 with
      strideX = 0, stridey = 0 and the G scaled (s, Lw) pairs;
  (b) 4096 resident data sets of that shape, G = 16: G calls of blr_posterior_batched_f64, one per setting, each over the B
      data sets at their strides;
  (c) 8192 x (64, 1024), G = 16, likewise;
  (d) (a) and (b) in fp32.
--quick: (a) at G = 64 and a B = 8, G = 16 call only (the rocprofv3 --kernel-trace --stats case: the launches of two (B, G)).
--stats-from DIR [--out FILE]: no timing; the per-call launch list from the kernel_trace.csv rocprofv3 wrote under DIR.
The numbers of DESIGN.md K13."""
import argparse
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS = 3, 15


def stats_from(d, out):
    import csv

    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    rows = []
    for fn in files:
        with open(fn) as f:
            for r in csv.DictReader(f):
                if "blr::grid_" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"].split("(")[0], int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]),
                                 int(r["Grid_Size_Y"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3,
                                 int(r["VGPR_Count"]), int(r["Scratch_Size"])))
    rows.sort()
    calls, cur = [], []
    for r in rows:  # a call starts with its prior kernel
        if "grid_prior_kernel" in r[1] and cur:
            calls.append(cur)
            cur = []
        cur.append(dict(kernel=r[1], workgroups_x=r[2], grid_y=r[3], us=round(r[4], 2), vgpr=r[5], scratch=r[6]))
    if cur:
        calls.append(cur)
    shapes = {}
    for c in calls:  # one representative (the last) call per launch geometry, and how many calls had it
        key = tuple((k["kernel"], k["workgroups_x"], k["grid_y"]) for k in c)
        shapes[key] = dict(calls=shapes.get(key, dict(calls=0))["calls"] + 1, launches=c)
    res = dict(source="rocprofv3 --kernel-trace --stats -- python tools/grid_bench.py --quick", per_call=list(shapes.values()))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-from", default=None)
    args = ap.parse_args()
    if args.stats_from:
        stats_from(args.stats_from, args.out)
        return

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn):
        ts = []
        for _ in range(WARMUP + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts[WARMUP:]))

    def row(name, B, D, N, G, dtype):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        gen = torch.Generator(device=dev).manual_seed(1234)
        X = torch.randn((B, N, D), device=dev, dtype=tdt, generator=gen)  # ColVecs: D x N column-major per data set
        w = torch.randn((B, D, 1), device=dev, dtype=tdt, generator=gen)
        y = (X @ w).squeeze(-1) + (0.1 ** 0.5) * torch.randn((B, N), device=dev, dtype=tdt, generator=gen)
        s = torch.full((B,), 0.1, device=dev, dtype=tdt)
        mw = torch.zeros((B, D), device=dev, dtype=tdt)
        Lw = torch.exp(0.3 * torch.randn((B, D), device=dev, dtype=tdt, generator=gen))
        side = int(round(G ** 0.5))
        sc = 10.0 ** np.linspace(-2, 2, side) if side * side == G else 10.0 ** np.linspace(-2, 2, G)
        al = np.repeat(sc, side) if side * side == G else sc
        ta = np.tile(sc, side) if side * side == G else sc[::-1].copy()
        alpha, tau = torch.tensor(al, device=dev, dtype=tdt), torch.tensor(ta, device=dev, dtype=tdt)
        lp = torch.zeros((B, G), device=dev, dtype=torch.float64)
        info = torch.zeros((B, G), device=dev, dtype=torch.int32)
        best = torch.zeros(B, device=dev, dtype=torch.int64)
        mwb = torch.zeros((B, D), device=dev, dtype=tdt)
        Tb = torch.zeros((B, D, D), device=dev, dtype=tdt)
        p = lambda t: t.data_ptr()  # noqa: E731

        def grid():
            h.logpdf_grid(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, p(X), D, D * N, p(y), N, a.NOISE_ISOTROPIC, p(s), 1,
                          a.PRIOR_DIAGONAL, p(mw), D, p(Lw), 1, D, G, p(alpha), 0, p(tau), 0, p(lp), G, p(best), p(mwb), D, p(Tb), D,
                          D * D, p(info), G)

        # the baseline's operands, prepared outside the timed region: s_g = tau_g s, Lw_g = alpha_g Lw
        s_g = (tau[:, None] * s[None, :]).contiguous()             # [G, B]
        L_g = (alpha[:, None, None] * Lw[None]).contiguous()       # [G, B, D]
        lp_b = torch.zeros((G, B), device=dev, dtype=torch.float64)
        info_b = torch.zeros((G, B), device=dev, dtype=torch.int32)

        if B == 1:
            def base():  # one call: the G settings as a batch over the one data set
                h.posterior_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, G, D, N, p(X), D, 0, p(y), 0, a.NOISE_ISOTROPIC, p(s_g), 1,
                                    a.PRIOR_DIAGONAL, p(mw), 0, p(L_g), 1, D, None, D, None, D, D * D, None, D, D * D, p(lp_b), p(info_b))
        else:
            def base():  # G calls, one per setting, each over the B data sets
                item = 8 if dtype == np.float64 else 4
                for g in range(G):
                    h.posterior_batched(dtype, a.MEM_DEVICE, a.LAYOUT_COLVECS, B, D, N, p(X), D, D * N, p(y), N, a.NOISE_ISOTROPIC,
                                        p(s_g) + g * B * item, 1, a.PRIOR_DIAGONAL, p(mw), D, p(L_g) + g * B * D * item, 1, D, None, D,
                                        None, D, D * D, None, D, D * D, p(lp_b) + g * B * 8, p(info_b) + g * B * 4)

        t_grid, t_base = timed(grid), timed(base)
        torch.cuda.synchronize()
        rel = float(((lp - lp_b.T).abs() / lp_b.T.abs()).max())
        assert int(info.abs().sum()) == 0 and int(info_b.abs().sum()) == 0
        r = dict(row=name, B=B, D=D, N=N, G=G, dtype=np.dtype(dtype).name, grid_ms=round(t_grid, 4), baseline_ms=round(t_base, 4),
                 speedup=round(t_base / t_grid, 3), max_rel_diff_evidence=rel)
        print(json.dumps(r), flush=True)
        del X
        torch.cuda.empty_cache()
        return r

    rows = []
    if args.quick:
        rows.append(row("a", 1, 128, 4096, 64, np.float64))
        rows.append(row("quick-b", 8, 128, 4096, 16, np.float64))
    else:
        rows.append(row("a", 1, 128, 4096, 64, np.float64))
        rows.append(row("a", 1, 128, 4096, 1024, np.float64))
        rows.append(row("b", 4096, 128, 4096, 16, np.float64))
        rows.append(row("c", 8192, 64, 1024, 16, np.float64))
        rows.append(row("d-a", 1, 128, 4096, 64, np.float32))
        rows.append(row("d-a", 1, 128, 4096, 1024, np.float32))
        rows.append(row("d-b", 4096, 128, 4096, 16, np.float32))
    res = dict(tool="tools/grid_bench.py", warmup=WARMUP, reps=REPS, timer="HIP events, median", rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
