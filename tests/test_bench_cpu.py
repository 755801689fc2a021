"""bench.py without a GPU: what a plain run leaves to --full, and the files of --dump-outputs."""
import os

import numpy as np


def test_bench_extra_measurements_need_full(repo_root):
    # a plain run measures the headline only: the CPU leg and the secondary entries are asked for with --full, and asking for them
    # without it is an error before anything touches the GPU
    import subprocess
    import sys

    bench = os.path.join(repo_root, "bench.py")
    for extra in (["--secondary-only", "c3_f32"], ["--secondary", "1"], ["--cpu-seconds", "5"]):
        r = subprocess.run([sys.executable, bench, "--gpus", "1"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--full" in r.stderr, (extra, r.stderr[-500:])


def test_bench_dump_outputs_fit_and_repeat(repo_root, tmp_path):
    # --dump-outputs at the headline shape (4096 regressors, D = 128, fp64): T alone is 512 MB, so it goes out as a seeded sample of
    # its rows with their indices; all files within 64 MB, float32 / float64 only, and the same files from the same outputs
    import importlib.util
    import types

    import torch

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(repo_root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    B, D = 4096, 128
    wl = types.SimpleNamespace(torch=torch, lp=-torch.arange(B, dtype=torch.float64), info=torch.zeros(B, dtype=torch.int32),
                               mw_post=torch.arange(B * D, dtype=torch.float64).reshape(B, D),
                               T_post=torch.arange(B * D * D, dtype=torch.float64).reshape(B, D, D))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), wl, -123.5)
    bench.dump_outputs(str(b), wl, -123.5)
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    assert names == ["T_post.npy", "T_post_rows.npy", "info.npy", "logpdf.npy", "mw_post.npy", "total_log_evidence.npy"]
    assert sum(p.stat().st_size for p in a.iterdir()) <= 64 << 20
    for n in names:
        x = np.load(a / n)
        assert x.dtype in (np.float32, np.float64), n
        np.testing.assert_array_equal(x, np.load(b / n))
    assert np.load(a / "total_log_evidence.npy").tolist() == [-123.5]
    np.testing.assert_array_equal(np.load(a / "mw_post.npy"), wl.mw_post.numpy())
    rows = np.load(a / "T_post_rows.npy")
    assert 1000 < rows.size < B * D and np.all(np.diff(rows) > 0) and np.all(rows == np.round(rows))
    np.testing.assert_array_equal(np.load(a / "T_post.npy"), wl.T_post.reshape(-1, D).numpy()[rows.astype(np.int64)])
