"""Leave-one-out predictives, timed (GPU box): python tools/loo_bench.py [--quick] [--out FILE]
Times blr_loo_batched_* with HIP events (median of the timed repeats after warm-up), every comparison in the same process:
  (a) from a resident state, B in {64, 2048} x (D, N) = (128, 4096), fp64: LOO (all outputs and the total) against
      blr_marginals_batched_f64 mean + var on the same factor;
  (b) the pipeline of loo_map from the prior at 2048 x (128, 4096): blr_posterior_batched into device buffers, then the LOO
      call, against blr_posterior_batched alone;
  (c) the per-observation alternative at the same batch: forget (downdate k = 1) then condition (update k = 1) of one
      observation in every regressor, 32 observations in a row, reported per observation, with the speed-up of (a) over N of them;
  (d) (a) and (b) in fp32, and (1024, 65536) fp32 at B = 1 against the marginals' mean + var at that shape.
--quick: only (a) in fp64 (the rocprofv3 --kernel-trace --stats case).
--stats-from DIR [--out FILE]: no timing; turns the kernel_trace.csv that rocprofv3 wrote under DIR into the per-kernel JSON
summary of profiles/loo_kernel_stats.json.  The numbers of DESIGN.md K12."""
import argparse
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS = 3, 15


def stats_from(d, out, source):
    import csv

    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    per, regs = {}, {}
    for fn in files:
        with open(fn) as f:
            for r in csv.DictReader(f):
                if "blr::" not in r["Kernel_Name"]:  # (the timing script's own torch kernels)
                    continue
                key = (r["Kernel_Name"], int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"]))  # grid.y = regressors of the launch
                per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                regs[key] = dict(vgpr=int(r["VGPR_Count"]), agpr=int(r["Accum_VGPR_Count"]), scratch=int(r["Scratch_Size"]))
    rows = [dict(kernel=k, grid_yz=g, calls=len(v), total_us=round(sum(v), 2), avg_us=round(sum(v) / len(v), 2),
                 median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2), **regs[(k, g)])
            for (k, g), v in per.items()]
    rows.sort(key=lambda r: -r["total_us"])
    res = dict(source=source, kernels=rows)
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
        stats_from(args.stats_from, args.out, "rocprofv3 --kernel-trace --stats -- python tools/loo_bench.py --quick "
                                              "(64 and 2048 x (128, 4096) fp64: LOO from a resident state, marginals mean + var)")
        return

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn, restore=lambda: None, reps=REPS):
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

    def problem(nb, D, N, ndt, seed=1):
        """inputs (ColVecs, regressor b at b N D), observations, isotropic noise and the posterior (mw', T) given all of them"""
        dt = torch.float64 if ndt == np.float64 else torch.float32
        g = torch.Generator(device=dev).manual_seed(seed)
        X = torch.randn((nb, N, D), generator=g, dtype=dt, device=dev) * (1.0 / np.sqrt(D))
        y = torch.randn((nb, N), generator=g, dtype=dt, device=dev)
        s = torch.full((1,), 0.5, dtype=dt, device=dev)
        Lw = torch.ones((nb, D), dtype=dt, device=dev)
        m0 = torch.zeros((nb, D), dtype=dt, device=dev)
        mw, T = torch.empty((nb, D), dtype=dt, device=dev), torch.empty((nb, D, D), dtype=dt, device=dev)
        info = torch.zeros(nb, dtype=torch.int32, device=dev)

        def post():
            h.posterior_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, X.data_ptr(), D, N * D, y.data_ptr(), N,
                                a.NOISE_ISOTROPIC, s.data_ptr(), 0, a.PRIOR_DIAGONAL, m0.data_ptr(), D, Lw.data_ptr(), 1, D,
                                mw.data_ptr(), D, T.data_ptr(), D, D * D, None, D, D * D, None, info.data_ptr())

        post()
        torch.cuda.synchronize()
        assert not info.any().item()
        return dt, X, y, s, mw, T, post

    out = []

    def emit(row):
        print(json.dumps(row), flush=True)
        out.append(row)

    def rows_a_b(nb, D, N, ndt, with_b=True, with_c=False):
        dt, X, y, s, mw, T, post = problem(nb, D, N, ndt)
        lm, lv = torch.empty((nb, N), dtype=dt, device=dev), torch.empty((nb, N), dtype=dt, device=dev)
        ll = torch.empty((nb, N), dtype=torch.float64, device=dev)
        tot = torch.empty(nb, dtype=torch.float64, device=dev)
        info = torch.zeros(nb, dtype=torch.int32, device=dev)
        mm, mv = torch.empty((nb, N), dtype=dt, device=dev), torch.empty((nb, N), dtype=dt, device=dev)

        def loo():
            h.loo(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, X.data_ptr(), D, N * D, y.data_ptr(), N, a.NOISE_ISOTROPIC,
                  s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, lm.data_ptr(), N, lv.data_ptr(), N, ll.data_ptr(), N,
                  tot.data_ptr(), info.data_ptr())

        def marg():
            h.marginals_batched(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, N, X.data_ptr(), D, N * D, a.NOISE_ISOTROPIC, s.data_ptr(),
                                0, a.PRIOR_UPPER_FACTOR, mw.data_ptr(), D, T.data_ptr(), D, D * D, mm.data_ptr(), N, mv.data_ptr(), N,
                                info.data_ptr())

        t_loo, t_marg = timed(loo), timed(marg)
        name = np.dtype(ndt).name
        emit(dict(what="a_resident", dtype=name, B=nb, D=D, N=N, loo_ms=round(t_loo, 4), marginals_mean_var_ms=round(t_marg, 4),
                  ratio=round(t_loo / t_marg, 3), target_ratio=1.10, degenerate=int(torch.isnan(ll).sum().item())))
        if with_b:
            t_post = timed(post)
            t_pipe = timed(lambda: (post(), loo()))
            emit(dict(what="b_loo_map_from_prior", dtype=name, B=nb, D=D, N=N, posterior_plus_loo_ms=round(t_pipe, 4),
                      posterior_ms=round(t_post, 4), marginals_mean_var_ms=round(t_marg, 4),
                      target_ms=round(t_post + 1.15 * t_marg, 4), excess_over_posterior_in_marginals=round((t_pipe - t_post) / t_marg, 3)))
        if with_c:
            K = 32
            T0, m0 = T.clone(), mw.clone()
            lp1 = torch.empty(nb, dtype=torch.float64, device=dev)
            inf1 = torch.zeros(nb, dtype=torch.int32, device=dev)

            def restore():
                T.copy_(T0)
                mw.copy_(m0)

            def pairs():
                for n in range(K):  # observation n of every regressor out, then back in
                    xp, yp = X.data_ptr() + n * D * X.element_size(), y.data_ptr() + n * y.element_size()
                    h.downdate_factor(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, 1, xp, D, N * D, yp, N, a.NOISE_ISOTROPIC,
                                      s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, lp1.data_ptr(), inf1.data_ptr())
                    h.update_factor(ndt, a.MEM_DEVICE, a.LAYOUT_COLVECS, nb, D, 1, xp, D, N * D, yp, N, a.NOISE_ISOTROPIC,
                                    s.data_ptr(), 0, mw.data_ptr(), D, T.data_ptr(), D, D * D, None, inf1.data_ptr())

            t_pairs = timed(pairs, restore, 5) / K
            emit(dict(what="c_forget_condition_per_observation", dtype=name, B=nb, D=D, observations_timed=K,
                      per_observation_ms=round(t_pairs, 4), all_N_estimate_ms=round(t_pairs * N, 1),
                      loo_ms=round(t_loo, 4), speedup_of_loo=round(t_pairs * N / t_loo, 1), failed=int(inf1.ne(0).sum().item())))
            del T0, m0
        del X, y, T, mw, lm, lv, ll, mm, mv
        torch.cuda.empty_cache()

    if args.quick:
        for nb in (64, 2048):
            rows_a_b(nb, 128, 4096, np.float64, with_b=False)
    else:
        rows_a_b(64, 128, 4096, np.float64, with_b=False)
        rows_a_b(2048, 128, 4096, np.float64, with_b=True, with_c=True)
        rows_a_b(64, 128, 4096, np.float32, with_b=False)
        rows_a_b(2048, 128, 4096, np.float32, with_b=True)
        rows_a_b(1, 1024, 65536, np.float32, with_b=False)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, timer="hip events, median", rows=out), f,
                      indent=1)


if __name__ == "__main__":
    main()
