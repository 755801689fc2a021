"""blr_posterior_ragged_x16 against the ways round it, timed (GPU box): python tools/x16_ragged_bench.py [--out FILE]
D = 128, B = 4096, bf16, aligned ColVecs and RowVecs, isotropic noise, diagonal prior, posterior mean + factor + evidence, everything
device resident.  Per layout, back to back in one process:
  (a) equal counts of 4096 against blr_posterior_batched_x16 (parity expected; a slower ragged call is reported as a miss);
  (b) counts log-uniform in [64, 16384] against padding to the longest (blr_posterior_batched_x16 on zero-padded copies), a loop of
      B = 1 calls (a sample of 64 regressors, EXTRAPOLATED to B), and blr_posterior_ragged_f32 on the widened copy with and without
      the widening pass;
  (c) one regressor of 2^20 observations among 4095 of 256, cut, against the same call kept whole (RAGGED_ITEM = 2^20).
Pre-heated (3 calls), then 10 calls timed with blr_timer_*, median.  Writes profiles/x16_ragged_bench.json by default.  The numbers of
DESIGN.md K34."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARMUP, REPS = 3, 10
B, D, LOOP_SAMPLE = 4096, 128, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "x16_ragged_bench.json"))
    args = ap.parse_args()

    import torch

    import blr_amd  # noqa: F401
    from blr_amd import _abi as a

    dev = torch.device("cuda:0")
    h = a.Handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.set_async(True)

    def timed(fn, reps=REPS):
        ts = []
        for i in range(WARMUP + reps):
            h.timer_start()
            fn()
            ts.append(h.timer_stop())
        return float(np.median(ts[WARMUP:]))

    gen = torch.Generator(device=dev).manual_seed(1234)
    s = torch.full((1,), 0.1, device=dev, dtype=torch.float32)
    mw = torch.zeros((B, D), device=dev, dtype=torch.float32)
    Lw = torch.exp(0.3 * torch.randn((B, D), device=dev, dtype=torch.float32, generator=gen))
    mw_post = torch.empty((B, D), device=dev, dtype=torch.float32)
    T = torch.empty((B, D * D), device=dev, dtype=torch.float32)
    lp = torch.empty((B,), device=dev, dtype=torch.float64)
    info = torch.empty((B,), device=dev, dtype=torch.int32)
    prior = (a.PRIOR_DIAGONAL, mw.data_ptr(), D, Lw.data_ptr(), 1, D)
    outs = (mw_post.data_ptr(), D, T.data_ptr(), D, D * D, None, D, D * D, lp.data_ptr(), info.data_ptr())
    rng = np.random.default_rng(4321)
    cases = (("equal", np.full(B, 4096)), ("loguniform", np.exp(rng.uniform(np.log(64), np.log(16384), B)).astype(np.int64)),
             ("one_long", np.concatenate([[1 << 20], np.full(B - 1, 256)])))
    rows = []
    for lname, layout in (("ColVecs", a.LAYOUT_COLVECS), ("RowVecs", a.LAYOUT_ROWVECS)):
        col = layout == a.LAYOUT_COLVECS
        for case, counts in cases:
            offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            total, longest = int(offsets[-1]), int(counts.max())
            # ColVecs: [total][D] row-major = D x total column-major; RowVecs: [D][total] = total x D column-major
            X16 = torch.randn((total, D) if col else (D, total), device=dev, dtype=torch.float32, generator=gen).to(torch.bfloat16)
            y = torch.randn((total,), device=dev, dtype=torch.float32, generator=gen)
            ldx = D if col else total

            def ragged16():
                h.posterior_ragged_x16(a.X_BF16, a.MEM_DEVICE, layout, B, D, offsets, X16.data_ptr(), ldx, y.data_ptr(), a.NOISE_ISOTROPIC,
                                       s.data_ptr(), 0, *prior, *outs)

            row = dict(case=case, layout=lname, B=B, D=D, fmt="bf16", observations=total, longest=longest, ms_ragged_x16=timed(ragged16),
                       route=h.last_route(), chunks=h.get_stat("last_chunks"))
            assert int(info.abs().max()) == 0
            lp16 = lp.clone()
            if case == "equal":
                N = 4096
                row["ms_batched_x16"] = timed(lambda: h.posterior_batched_x16(
                    a.X_BF16, a.MEM_DEVICE, layout, B, D, N, X16.data_ptr(), ldx if col else total, N * D if col else N, y.data_ptr(), N,
                    a.NOISE_ISOTROPIC, s.data_ptr(), 0, *prior, *outs))
                row["same_bits_as_batched"] = bool(torch.equal(lp16, lp))
                row["miss"] = row["ms_ragged_x16"] > 1.02 * row["ms_batched_x16"]
            elif case == "loguniform":
                # padding to the longest: zero features and zero targets behind every regressor's own observations
                Xp = torch.zeros((B, longest, D) if col else (B, D, longest), device=dev, dtype=torch.bfloat16)
                yp = torch.zeros((B, longest), device=dev, dtype=torch.float32)
                row["ms_padded_batched_x16"] = timed(lambda: h.posterior_batched_x16(
                    a.X_BF16, a.MEM_DEVICE, layout, B, D, longest, Xp.data_ptr(), D if col else longest, D * longest, yp.data_ptr(), longest,
                    a.NOISE_ISOTROPIC, s.data_ptr(), 0, *prior, *outs))
                del Xp, yp
                sample = rng.choice(B, LOOP_SAMPLE, replace=False)

                def loop():
                    for b in sample:
                        o, n = int(offsets[b]), int(counts[b])
                        h.posterior_batched_x16(a.X_BF16, a.MEM_DEVICE, layout, 1, D, n, X16.data_ptr() + 2 * (o * D if col else o), ldx, 0,
                                                y.data_ptr() + 4 * o, 0, a.NOISE_ISOTROPIC, s.data_ptr(), 0, *prior, *outs)

                row["ms_loop_of_single_calls_extrapolated"] = timed(loop, reps=3) * B / LOOP_SAMPLE
                row["loop_sample"] = LOOP_SAMPLE
                X32 = X16.to(torch.float32)
                row["ms_ragged_f32_on_widened"] = timed(lambda: h.posterior_ragged(
                    np.float32, a.MEM_DEVICE, layout, B, D, offsets, X32.data_ptr(), ldx, y.data_ptr(), a.NOISE_ISOTROPIC, s.data_ptr(), 0,
                    *prior, *outs))
                row["route_f32"] = h.last_route()
                row["max_rel_evidence_difference_to_f32"] = float(((lp16 - lp).abs() / lp.abs()).max())
                row["ms_widen"] = timed(lambda: X32.copy_(X16))
                del X32
            else:
                h.set_option("RAGGED_ITEM", 1 << 20)
                row["ms_kept_whole"] = timed(ragged16, reps=3)
                row["route_kept_whole"] = h.last_route()
                h.set_option("RAGGED_ITEM", None)
                row["max_rel_evidence_difference_to_whole"] = float(((lp16 - lp).abs() / lp.abs()).max())
                row["speedup_cut_over_whole"] = row["ms_kept_whole"] / row["ms_ragged_x16"]
            row["updates_per_s_ragged_x16"] = B / (row["ms_ragged_x16"] * 1e-3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del X16, y
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/x16_ragged_bench.py", warmup=WARMUP, reps=REPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
