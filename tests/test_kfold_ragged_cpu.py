"""CPU-side checks of the ragged leave-fold-out predictives (blr_kfold_ragged_*, blr_kfold_ragged_fold_offsets, kfold_ragged;
DESIGN.md K27): the symbols are declared, exported and bound with one arity; the fold table against NumPy; the argument checks that
need no device, one per documented position; the host-only planner (tools/kfold_ragged_plan_dump.cpp, also built and run with the
host sanitizers as a stand-alone program); the new kernels' resources from the compiled code object; and that no fold of the inputs
the GPU tests use is near-degenerate."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

import _kfold_ragged_data as K

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARITY = {"blr_kfold_ragged_f64": 23, "blr_kfold_ragged_f32": 23, "blr_kfold_ragged_fold_offsets": 4}
I64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731


def _arity(text, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return len([p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()])


def test_symbols_declared_exported_bound_and_one_arity(repo_root):
    header = open(os.path.join(repo_root, "include", "blr_mi355x.h")).read()
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    lib = _abi.load_library()
    for name, n in ARITY.items():
        assert hasattr(lib, name) and name in _abi.EXPORTED_SYMBOLS
        assert _arity(header, name) == len(_abi._SIGS[name][0]) == n
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m and len([t for t in m.group(1).split(",") if t.strip()]) == n, name
    assert "function kfold_ragged!(" in jl and hasattr(_abi.Handle, "kfold_ragged")
    assert blr_amd.kfold_ragged is R.kfold_ragged and "kfold_ragged" in blr_amd.__all__ and "kfold_ragged" in R.__all__
    block = header[header.rindex("/* ----", 0, header.index("int blr_kfold_ragged_f64")):header.index("int blr_kfold_ragged_f64")]
    block = re.sub(r"\s*\n \* ", " ", block)  # (the comment's line breaks)
    assert "map over fxs of different lengths" in block and "Bit promises" in block and "bit for bit what blr_kfold_batched_* with B = 1" in block


# ---- the fold table ------------------------------------------------------------------------------------------------------------------
def _fold_offsets(B, offsets, F, out="alloc"):
    fo = np.full(B + 1, -7, dtype=np.int64) if isinstance(out, str) else out
    rc = _abi.load_library().blr_kfold_ragged_fold_offsets(B, _abi._ptr(offsets), F, _abi._ptr(fo))
    return rc, fo


@pytest.mark.parametrize("F", K.FS)
def test_fold_offsets_against_numpy(F):
    off = np.concatenate([[K.LEAD], K.LEAD + np.cumsum(K.COUNTS)]).astype(np.int64)
    rc, fo = _fold_offsets(len(K.COUNTS), off, F)
    assert rc == 0
    want = np.concatenate([[0], np.cumsum(-(-np.array(K.COUNTS) // F))])
    assert fo.tolist() == want.tolist() and fo.tolist() == K.batch(5).fold_offsets(F).tolist()
    assert all(fo[b + 1] - fo[b] == (1 if 0 < n <= F else -(-n // F)) for b, n in enumerate(K.COUNTS))  # F > N_b: one fold


def test_fold_offsets_argument_errors():
    assert _fold_offsets(2, I64(0, 3, 2), 8)[0] == -6      # decreasing
    assert _fold_offsets(2, I64(-1, 3, 5), 8)[0] == -6     # negative
    assert _fold_offsets(2, None, 8)[0] == -6              # NULL with B > 0
    assert _fold_offsets(2, I64(0, 3, 5), 0)[0] == -7
    assert _fold_offsets(2, I64(0, 3, 5), 65)[0] == -7
    assert _fold_offsets(-1, I64(0), 8)[0] == -4
    assert _fold_offsets(2, I64(0, 3, 5), 8, out=None)[0] == -21
    rc, fo = _fold_offsets(0, None, 8)
    assert rc == 0 and fo.tolist() == [0]


# ---- argument errors of the entry points through a NULL handle ----------------------------------------------------------------------
def _kf(name, **kw):
    D = 4
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=2, D=D, offsets=I64(0, 3, 5), F=2, X=np.zeros((D, 5)), ldx=D, y=np.zeros(5),
             noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(2), strides=1, mw=np.zeros((2, D)), stridemw=D, T=np.zeros((2, D, D)), ldt=D,
             strideT=D * D, km=np.zeros(5), kv=np.zeros(5), kl=np.zeros(4), tot=np.zeros(2), info=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(_abi.load_library(), name)(None, a["memspace"], a["layout"], a["B"], a["D"], p(a["offsets"]), a["F"], p(a["X"]), a["ldx"],
                                              p(a["y"]), a["noise_kind"], p(a["s"]), a["strides"], p(a["mw"]), a["stridemw"], p(a["T"]), a["ldt"],
                                              a["strideT"], p(a["km"]), p(a["kv"]), p(a["kl"]), p(a["tot"]), p(a["info"]))


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_argument_errors_without_a_device(suf):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    name = f"blr_kfold_ragged_{suf}"
    assert _kf(name, memspace=7) == -2
    assert _kf(name, layout=2) == -3
    assert _kf(name, B=-1) == -4
    assert _kf(name, D=0) == -5 and _kf(name, D=8193, ldx=8193, ldt=8193) == -5
    assert _kf(name, offsets=I64(0, 3, 2)) == -6               # a decreasing entry
    assert _kf(name, offsets=I64(-1, 3, 5)) == -6              # a negative entry
    assert _kf(name, offsets=None) == -6                       # NULL with B > 0
    assert _kf(name, offsets=I64(0, 3, 3 + 2**30 + 1)) == -6   # a regressor beyond 2^30
    assert _kf(name, D=129, ldx=129, ldt=129, offsets=I64(0, 3, 3 + 16385)) == -6  # D > 128: N_b > 16384
    assert _kf(name, D=129, ldx=129, ldt=129, offsets=I64(0, 3, 3 + 16384)) == -1
    assert _kf(name, D=128, ldx=128, ldt=128, offsets=I64(0, 3, 3 + 16385)) == -1
    assert _kf(name, F=0) == -7 and _kf(name, F=65) == -7
    assert _kf(name, X=None) == -8
    assert _kf(name, ldx=3) == -9                              # ColVecs: ldx < D
    assert _kf(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -9  # RowVecs: ldx < offsets[B]
    assert _kf(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1
    assert _kf(name, y=None) == -10
    assert _kf(name, noise_kind=_abi.NOISE_DENSE) == -11       # dense noise couples the folds
    assert _kf(name, s=None) == -12
    assert _kf(name, strides=-1) == -13
    assert _kf(name, mw=None) == -14
    assert _kf(name, stridemw=-1) == -15
    assert _kf(name, T=None) == -16
    assert _kf(name, ldt=3) == -17
    assert _kf(name, strideT=-1) == -18
    assert _kf(name, info=None) == -23
    assert _kf(name, memspace=7, layout=2, F=0) == -2          # the ranges come first, in the order of the arguments
    assert _kf(name, B=0) == 0
    assert _kf(name) == -1                                     # valid arguments and a NULL handle
    assert _kf(name, km=None, kv=None, kl=None, tot=None) == -1  # every output may be NULL
    assert _kf(name, offsets=I64(2, 2, 5)) == -1               # an empty regressor and offsets[0] > 0 are valid
    assert _kf(name, F=64) == -1                               # F > N_b: one fold


# ---- the planner -------------------------------------------------------------------------------------------------------------------
OFFSETS = np.concatenate([[K.LEAD], K.LEAD + np.cumsum(K.COUNTS)]).tolist()


@pytest.fixture(scope="module")
def dump(tmp_path_factory, repo_root):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc in this image")
    d = tmp_path_factory.mktemp("kfold_ragged_plan")
    src = os.path.join(repo_root, "tools", "kfold_ragged_plan_dump.cpp")
    exes = {}
    for tag, extra in (("plain", []), ("san", ["-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"])):
        exe = str(d / f"kfold_ragged_plan_dump_{tag}")
        r = subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", *extra, "-o", exe, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        exes[tag] = exe
    return exes


def _plan(exe, offsets, D, F, options=(), cus=256, elem=8):
    r = subprocess.run([exe, str(cus), str(elem), str(D), str(F), *options, "--", *map(str, offsets)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout)


def _check_plan(p, offsets, F, max_chunk=None):
    counts = np.diff(offsets)
    W, pr = p["W"], (64 // F) * F
    assert W % 64 == 0 and W >= 64
    po, fo = p["pack_offsets"], p["fold_offsets"]
    assert len(po) == len(fo) == len(counts) + 1 and po[0] == fo[0] == 0
    assert all(b >= a for a, b in zip(po, po[1:]))                                # monotone
    for b, n in enumerate(counts):
        npk = po[b + 1] - po[b]
        assert npk == -(-int(n) // pr) and fo[b + 1] - fo[b] == -(-int(n) // F)
        # pack k of regressor b covers [k pr, min((k + 1) pr, N_b)) of ITS slice: whole folds, none of a neighbour's rows
        rows = [(k * pr, min((k + 1) * pr, int(n))) for k in range(npk)]
        assert all(lo < hi <= n and lo % F == 0 for lo, hi in rows)
        assert (rows[-1][1] if rows else 0) == n                                   # the last pack ends at N_b
    covered = [np.zeros(n, dtype=int) for n in counts]
    for reg, t0, nt in p["items"]:
        assert nt >= 1 and 16 * t0 < counts[reg] and (16 * t0) % W == 0 and (16 * t0) % 64 == 0
        lo, hi = 16 * t0, min(16 * (t0 + nt), counts[reg])
        assert 16 * (t0 + nt) < counts[reg] + 16 and hi - lo <= W
        covered[reg][lo:hi] += 1
    assert all(np.all(c == 1) for c in covered)                                   # every observation whitened exactly once
    pos = b = 0
    for c in p["chunks"]:
        assert c["b0"] == b and c["nb"] >= 1 and c["item0"] == pos and c["nb"] <= 65535 and c["nb"] * p["image_bytes"] <= 256 << 20
        rows = int(offsets[c["b0"] + c["nb"]] - offsets[c["b0"]])
        assert rows * p["row_bytes"] <= 256 << 20 or c["nb"] == 1                 # the rows of Z; never fewer than one regressor
        assert rows <= p["max_rows"] and c["nb"] <= p["max_nb"] and (max_chunk is None or c["nb"] <= max_chunk)
        assert all(c["b0"] <= it[0] < c["b0"] + c["nb"] for it in p["items"][pos:pos + c["nitems"]])
        pos, b = pos + c["nitems"], b + c["nb"]
    assert pos == len(p["items"]) and b == len(counts) and p["last_chunks"] == len(p["chunks"])


@pytest.mark.parametrize("tag", ["plain", "san"])
def test_planner(dump, tag):
    exe = dump[tag]
    for F in K.FS:
        p = _plan(exe, OFFSETS, 128, F)
        _check_plan(p, OFFSETS, F)
        assert p["last_chunks"] == 1 and p["W"] == 256
    p21 = _plan(exe, OFFSETS, 128, 21)
    assert np.diff(p21["pack_offsets"]).tolist() == [0, 1, 1, 1, 1, 1, 2, 2, 4, 0, 6]   # packs of 63 rows
    for cap, chunks in ((1, 11), (2, 6)):
        p = _plan(exe, OFFSETS, 64, 8, ["RAGGED_ITEM=64", f"MAX_CHUNK={cap}"])
        _check_plan(p, OFFSETS, 8, max_chunk=cap)
        assert p["last_chunks"] == chunks and p["W"] == 64
        assert p["items"] == _plan(exe, OFFSETS, 64, 8, ["RAGGED_ITEM=64"])["items"]    # the cut does not depend on the chunking
    # the rows of Z bound a chunk: fp64 at D = 128 is 1024 bytes a row, 262144 rows in 256 MiB
    long = np.concatenate([[0], np.cumsum([100_000, 100_000, 100_000, 300_000, 10, 0, 262_144, 1])]).tolist()
    p = _plan(exe, long, 128, 64)
    _check_plan(p, long, 64)
    # (200 000 | 100 000 | 300 000 alone, over the bound | 10 + 0 | 262 144 exactly | 1)
    assert [c["nb"] for c in p["chunks"]] == [2, 1, 1, 2, 1, 1] and p["max_rows"] == 300_000
    # ... and four times as many rows at fp32, D = 50 (DP = 64: 256 bytes a row)
    p = _plan(exe, long, 50, 3, elem=4)
    _check_plan(p, long, 3)
    assert p["last_chunks"] == 1
    # the images bound it too: 73 728-byte fp64 images, 3640 of them
    many = list(range(0, 4001))
    p = _plan(exe, many, 128, 8)
    _check_plan(p, many, 8)
    assert p["chunks"][0]["nb"] == (256 << 20) // 73728 and p["last_chunks"] == 2


# ---- the code object ---------------------------------------------------------------------------------------------------------------
def _kfold_lds_bytes(elem, D, repo_root):
    """kfold_lds_bytes (csrc/blr_kfold.hpp) from the constants the sources state"""
    csrc = os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc")
    kf = open(os.path.join(csrc, "blr_kfold.hpp")).read()
    cov = open(os.path.join(csrc, "blr_cov_batched.hpp")).read()
    fmax = int(re.search(r"constexpr int kFoldMax = (\d+);", kf).group(1))
    assert re.search(r"constexpr int kFoldLdg = kFoldMax \+ 1;", kf) and re.search(r"constexpr int kCovTile = (\d+);", cov).group(1) == "64"
    assert "return (tile > block ? tile : block) + (size_t)5 * kFoldMax * sizeof(double);" in kf
    assert "return (size_t)kCovTile * (size_t)(DP + 16 / (int)elem) * elem;" in cov
    DP = 16 * ((D + 15) // 16)
    return max(64 * (DP + 16 // elem) * elem, fmax * (fmax + 1) * 8) + 5 * fmax * 8


def test_new_kernels_stay_within_their_launch_bounds(tmp_path, repo_root):
    """__launch_bounds__(256, 2), kfold_kernel's: at most 256 registers a lane, no scratch, no spill; the fold kernel's LDS is all
    dynamic, kfold_lds_bytes at its launch, and fits twice into the CU's 160 KiB (the figures: DESIGN.md K27)."""
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    so = shutil.copy(_abi.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    cos = [p for p in os.listdir(tmp_path) if "gfx950" in p]
    assert cos
    notes = "".join(subprocess.run([readelf, "--notes", str(tmp_path / c)], check=True, capture_output=True, text=True).stdout for c in sorted(cos))
    props, name = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            props.setdefault(name, {})[m.group(1)] = int(m.group(2))
    new = {k: v for k, v in props.items() if re.search(r"kfold_ragged_(whiten_)?kernel", k)}
    assert len(new) == 6, sorted(new)  # 2 x (2 whitening layouts + the fold kernel)
    old = {k: v for k, v in props.items() if re.search(r"3blr12kfold_kernelI", k)}
    assert len(old) == 2, sorted(old)
    for k, v in {**new, **old}.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 256 and v["max_flat_workgroup_size"] == 256, (k, v)
        assert v["group_segment_fixed_size"] == 0, (k, v)  # all of it dynamic
    abi = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_abi.hip")).read()
    assert re.search(r"lds_k = kfold_lds_bytes\(sizeof\(T\), \(int\)D\);\n(.*\n){1,24}?.*hipLaunchKernelGGL\(kfold_ragged_kernel<T>, dim3\(\(unsigned\)npacks\), "
                     r"dim3\(kThreads\), lds_k,", abi)
    hpp = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_kfold_ragged.hpp")).read()
    assert "__launch_bounds__(kThreads, 2) void kfold_ragged_kernel" in hpp and "kfold_pack<T>(smem, p);" in hpp
    assert _kfold_lds_bytes(8, 128, repo_root) == 69120 and _kfold_lds_bytes(4, 128, repo_root) == 36352
    for elem in (8, 4):
        for D in (1, 5, 64, 128):
            assert 2 * _kfold_lds_bytes(elem, D, repo_root) <= 160 * 1024


def test_the_fold_body_exists_once(repo_root):
    """kfold_kernel and kfold_ragged_kernel call one body: the Cholesky sweep is written once"""
    csrc = os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("blr_kfold.hpp", "blr_kfold_ragged.hpp"))
    assert text.count("const double rinv = 1.0 / sqrt(piv);") == 1 and text.count("kfold_pack<T>(smem, p);") == 2


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", K.DS)
def test_gpu_test_inputs_have_no_near_degenerate_fold(D):
    """The largest eigenvalue of any fold's H~ (closed_form's fourth output) for every count, F, D, noise kind and element type
    tests/test_kfold_ragged_gpu.py uses: at most 0.9, so no pivot of I - H~ is below 0.1 and no GPU test leans on a fold the
    state barely contains."""
    P = K.batch(D)
    worst = 0.0
    for noise in K.NOISES:
        for dtype in (np.float64, np.float32):
            for F in K.FS:
                for b in range(P.nb):
                    if P.counts[b]:
                        worst = max(worst, P.reference(noise, dtype, F, b)[3])
    print("largest eigenvalue of any H~ at D =", D, worst)
    assert worst <= 0.9


def test_gpu_test_inputs_of_the_large_d_route():
    P = K.batch(K.LARGE_D, counts=K.LARGE_COUNTS)
    assert max(P.reference("diagonal", np.float64, K.LARGE_F, b)[3] for b in range(P.nb) if P.counts[b]) <= 0.9
