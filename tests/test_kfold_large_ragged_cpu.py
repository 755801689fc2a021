"""CPU-side checks of the ragged large-fold leave-fold-out predictives (blr_kfold_large_ragged_*, its two host helpers,
kfold_large_ragged, cross_validate_ragged): the symbols are declared, exported and bound with one arity; the two
tables against NumPy; the argument checks that need no device, one per documented position; the host-only planner
(tools/kfold_large_ragged_plan_dump.cpp, also built and run with the host sanitizers as a stand-alone program); the new kernels'
resources from the compiled code object; and that no fold of the inputs the GPU tests use is near-degenerate."""
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

import _kfold_large_ragged_data as K

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARITY = {"blr_kfold_large_ragged_f64": 23, "blr_kfold_large_ragged_f32": 23, "blr_kfold_large_ragged_fold_sizes": 4,
         "blr_kfold_large_ragged_fold_offsets": 4}
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
    assert "function kfold_large_ragged!(" in jl and hasattr(_abi.Handle, "kfold_large_ragged")
    for fn in ("kfold_large_ragged", "cross_validate_ragged"):
        assert getattr(blr_amd, fn) is getattr(R, fn) and fn in blr_amd.__all__ and fn in R.__all__
    block = header[header.rindex("/* ----", 0, header.index("int blr_kfold_large_ragged_f64")):header.index("int blr_kfold_large_ragged_f64")]
    block = re.sub(r"\s*\n \* ", " ", block)  # (the comment's line breaks)
    assert "Bit promises" in block and "bit for bit what blr_kfold_large_batched_* with B = 1, N = N_b, F = F_b writes on that slice" in block


# ---- the two tables ------------------------------------------------------------------------------------------------------------------
def _offsets(counts, lead=K.LEAD):
    return np.concatenate([[lead], lead + np.cumsum(counts)]).astype(np.int64)


def _sizes(B, offsets, Kf, out="alloc"):
    fs = np.full(max(B, 0), -7, dtype=np.int64) if isinstance(out, str) else out
    return _abi.load_library().blr_kfold_large_ragged_fold_sizes(B, _abi._ptr(offsets), Kf, _abi._ptr(fs)), fs


def _fold_offsets(B, offsets, sizes, out="alloc"):
    fo = np.full(max(B, 0) + 1, -7, dtype=np.int64) if isinstance(out, str) else out
    return _abi.load_library().blr_kfold_large_ragged_fold_offsets(B, _abi._ptr(offsets), _abi._ptr(sizes), _abi._ptr(fo)), fo


@pytest.mark.parametrize("Kf", [1, 2, 5, 10, 1024])
def test_fold_sizes_and_offsets_against_numpy(Kf):
    counts = np.array(K.COUNTS + [3, 9, 1024, 1025])  # N_b = 0, N_b < K and K = 1 among them
    off = _offsets(counts)
    rc, fs = _sizes(len(counts), off, Kf)
    assert rc == 0 and fs.tolist() == np.maximum(1, -(-counts // Kf)).tolist()
    rc, fo = _fold_offsets(len(counts), off, fs)
    want = [0 if n == 0 else -(-n // f) for n, f in zip(counts.tolist(), fs.tolist())]
    assert rc == 0 and fo.tolist() == np.concatenate([[0], np.cumsum(want)]).tolist()
    assert all(w <= Kf for w in want) and all(w == min(n, Kf) for w, n in zip(want, counts.tolist()) if n % Kf == 0 or n < Kf)


def test_fold_offsets_of_the_gpu_batch_and_one_fold():
    off = _offsets(K.COUNTS)
    rc, fo = _fold_offsets(len(K.COUNTS), off, I64(*K.FOLDS))
    assert rc == 0 and fo.tolist() == K.batch(5).fold_offsets().tolist()
    assert np.diff(fo).tolist() == [0, 1, 7, 1, 2, 4, 2, 2, 2]  # (7, 100): F_b > N_b is one fold


def test_table_argument_errors():
    off = I64(0, 3, 5)
    assert _sizes(-1, I64(0), 5)[0] == -4
    assert _sizes(2, None, 5)[0] == -6 and _sizes(2, I64(0, 3, 2), 5)[0] == -6 and _sizes(2, I64(-1, 3, 5), 5)[0] == -6
    assert _sizes(2, off, 0)[0] == -3 and _sizes(2, off, 1025)[0] == -3
    assert _sizes(2, off, 5, out=None)[0] == -7
    assert _sizes(0, None, 5, out=None)[0] == 0
    assert _fold_offsets(-1, I64(0), I64(1))[0] == -4
    assert _fold_offsets(2, I64(0, 3, 2), I64(1, 1))[0] == -6
    assert _fold_offsets(2, off, None)[0] == -7 and _fold_offsets(2, off, I64(1, 0))[0] == -7
    assert _fold_offsets(2, I64(0, 3, 3 + 1025), I64(1, 1))[0] == -7  # 1025 folds
    assert _fold_offsets(2, I64(0, 3, 3 + 1024), I64(1, 1))[0] == 0
    assert _fold_offsets(2, off, I64(1, 1), out=None)[0] == -21
    rc, fo = _fold_offsets(0, None, None)
    assert rc == 0 and fo.tolist() == [0]


# ---- argument errors of the entry points through a NULL handle ----------------------------------------------------------------------
def _kf(name, **kw):
    D = 4
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=2, D=D, offsets=I64(0, 3, 5), fold_sizes=I64(2, 1), X=np.zeros((D, 5)), ldx=D,
             y=np.zeros(5), noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(2), strides=1, mw=np.zeros((2, D)), stridemw=D, T=np.zeros((2, D, D)),
             ldt=D, strideT=D * D, km=np.zeros(5), kv=np.zeros(5), kl=np.zeros(4), tot=np.zeros(2), info=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(_abi.load_library(), name)(None, a["memspace"], a["layout"], a["B"], a["D"], p(a["offsets"]), p(a["fold_sizes"]), p(a["X"]),
                                              a["ldx"], p(a["y"]), a["noise_kind"], p(a["s"]), a["strides"], p(a["mw"]), a["stridemw"], p(a["T"]),
                                              a["ldt"], a["strideT"], p(a["km"]), p(a["kv"]), p(a["kl"]), p(a["tot"]), p(a["info"]))


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_argument_errors_without_a_device(suf):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    name = f"blr_kfold_large_ragged_{suf}"
    assert _kf(name, memspace=7) == -2
    assert _kf(name, layout=2) == -3
    assert _kf(name, B=-1) == -4
    assert _kf(name, D=0) == -5 and _kf(name, D=129, ldx=129, ldt=129) == -5   # no route beyond D = 128
    assert _kf(name, D=128, ldx=128, ldt=128) == -1
    assert _kf(name, offsets=I64(0, 3, 2)) == -6               # a decreasing entry
    assert _kf(name, offsets=I64(-1, 3, 5)) == -6              # a negative entry
    assert _kf(name, offsets=None) == -6                       # NULL with B > 0
    assert _kf(name, offsets=I64(0, 3, 3 + 2**30 + 1)) == -6   # a regressor beyond 2^30
    assert _kf(name, fold_sizes=None) == -7                    # NULL with B > 0
    assert _kf(name, fold_sizes=I64(2, 0)) == -7               # an entry < 1
    assert _kf(name, offsets=I64(0, 3, 3 + 1025), X=np.zeros((4, 1028)), ldx=4) == -7   # 1025 folds of one
    assert _kf(name, offsets=I64(0, 3, 3 + 1024), X=np.zeros((4, 1027)), ldx=4) == -1
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
    assert _kf(name, memspace=7, layout=2, fold_sizes=None) == -2  # the ranges come first, in the order of the arguments
    assert _kf(name, B=0) == 0 and _kf(name, B=0, offsets=None, fold_sizes=None, info=None) == 0
    assert _kf(name) == -1                                     # valid arguments and a NULL handle
    assert _kf(name, km=None, kv=None, kl=None, tot=None) == -1  # every output may be NULL
    assert _kf(name, offsets=I64(2, 2, 5)) == -1               # an empty regressor and offsets[0] > 0 are valid
    assert _kf(name, fold_sizes=I64(10**9, 1)) == -1           # F_b > N_b: one fold


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def _splits(nf):
    s = min(max(nf // 1024, 1), 8)
    c = -(-(-(-nf // s)) // 64) * 64
    return s, max(c, 64)


@pytest.fixture(scope="module")
def dump(tmp_path_factory, repo_root):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc in this image")
    d = tmp_path_factory.mktemp("kfold_large_ragged_plan")
    src = os.path.join(repo_root, "tools", "kfold_large_ragged_plan_dump.cpp")
    exes = {}
    for tag, extra in (("plain", []), ("san", ["-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"])):
        exe = str(d / f"kfold_large_ragged_plan_dump_{tag}")
        r = subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", *extra, "-o", exe, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        exes[tag] = exe
    return exes


def _plan(exe, offsets, sizes, D, options=(), cus=256, elem=8):
    r = subprocess.run([exe, str(cus), str(elem), str(D), *options, "--", *map(str, offsets), "--", *map(str, sizes)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout)


def _check_plan(p, offsets, sizes, cus=256, max_chunk=None):
    """the NumPy restatement: records, the three tables (disjoint, complete, in order) and the chunk bounds"""
    counts = np.diff(offsets).tolist()
    stat, red, pred, fo, slot, tiles = [], [], [], [0], 0, 0
    folds_of = []
    for b, (n, F0) in enumerate(zip(counts, sizes)):
        F = min(F0, max(n, 1))
        nf = 0 if n == 0 else -(-n // F)
        r = p["regs"][b]
        assert (r["row0"], r["n"], r["F"], r["nfolds"], r["fold0"], r["slot0"], r["S"]) == (offsets[b], n, F, nf, fo[-1], slot, _splits(F)[0])
        rows = [min(F, n - f * F) for f in range(nf)]
        assert sum(rows) == n and all(x >= 1 for x in rows)
        folds_of.append(rows)
        fo.append(fo[-1] + nf)
        slot += (nf - 1) * _splits(F)[0] + _splits(rows[-1])[0] if nf else 0
        tiles += sum(-(-x // 64) for x in rows)
    assert p["fold_offsets"] == fo
    tpg = max(4, -(-tiles // (2 * cus)))
    assert p["tiles_per_group"] == tpg
    for b, rows in enumerate(folds_of):
        for f, x in enumerate(rows):
            S = _splits(x)[0]
            stat += [[b, f, sp, S] for sp in range(S)]
            red += [[b, f, 0, S]] if S > 1 else []
            ng = -(-(-(-x // 64)) // tpg)
            pred += [[b, f, g, ng] for g in range(ng)]
    assert p["stat"] == stat and p["red"] == red and p["pred"] == pred
    # a block covers [sp c, min((sp + 1) c, n_f)): the blocks of a fold tile it, whole stages of 64, none empty
    for b, f, sp, S in stat:
        c = _splits(folds_of[b][f])[1]
        assert c % 64 == 0 and sp * c < folds_of[b][f] <= S * c
    b = 0
    pos = dict(stat=0, red=0, pred=0)
    for c in p["chunks"]:
        assert c["b0"] == b and c["nb"] >= 1 and c["nb"] <= 65535 and (max_chunk is None or c["nb"] <= max_chunk)
        r0 = p["regs"][c["b0"]]
        assert c["fold0"] == r0["fold0"] == fo[c["b0"]] and c["nfolds"] == fo[c["b0"] + c["nb"]] - fo[c["b0"]] and c["slot0"] == r0["slot0"]
        end = p["regs"][c["b0"] + c["nb"]]["slot0"] if c["b0"] + c["nb"] < len(counts) else slot
        assert c["nslots"] == end - c["slot0"] == c["nstat"]
        for key in ("stat", "red", "pred"):
            assert c[key + "0"] == pos[key]
            assert all(c["b0"] <= it[0] < c["b0"] + c["nb"] for it in p[key][pos[key]:pos[key] + c["n" + key]])
            pos[key] += c["n" + key]
            assert c["n" + key] <= p["max_grid"] or c["nb"] == 1
        for n_, bytes_ in ((c["nslots"], p["stat_bytes"]), (c["nfolds"], p["u_bytes"]), (c["nfolds"], p["image_bytes"])):
            assert n_ * bytes_ <= 256 << 20 or c["nb"] == 1      # never fewer than one regressor
        assert c["nb"] <= p["max_nb"] and c["nfolds"] <= p["max_folds"] and c["nslots"] <= p["max_slots"]
        b += c["nb"]
    assert b == len(counts) and p["last_chunks"] == len(p["chunks"]) and all(pos[k] == len(p[k]) for k in pos)


@pytest.mark.parametrize("tag", ["plain", "san"])
def test_planner(dump, tag):
    exe = dump[tag]
    off = _offsets(K.COUNTS).tolist()
    for D in (5, 128):
        p = _plan(exe, off, K.FOLDS, D)
        _check_plan(p, off, K.FOLDS)
        assert p["last_chunks"] == 1 and p["tiles_per_group"] == 4
    # (2148, 2048): a two-block fold and a one-block last fold -> three slots, not four; (4200, 2100): 2 + 2
    assert [r["S"] for r in p["regs"]][-2:] == [2, 2] and p["chunks"][0]["nslots"] == 0 + 1 + 7 + 1 + 2 + 4 + 2 + 3 + 4
    assert p["red"] == [[7, 0, 0, 2], [8, 0, 0, 2], [8, 1, 0, 2]]
    for cap, chunks in ((1, 9), (2, 5)):
        q = _plan(exe, off, K.FOLDS, 17, [f"MAX_CHUNK={cap}"])
        _check_plan(q, off, K.FOLDS, max_chunk=cap)
        assert q["last_chunks"] == chunks
        assert (q["stat"], q["red"], q["pred"]) == (p["stat"], p["red"], p["pred"])   # the tables do not depend on the chunking
    # the factors bound a chunk: 131 072-byte fp64 factors at D = 128, 2048 folds -> 204 regressors of ten folds (the 73 728-byte images
    # would allow 364)
    many = list(range(0, 100 * 1001, 100))
    p = _plan(exe, many, [10] * 1000, 128)
    _check_plan(p, many, [10] * 1000)
    assert p["u_bytes"] == 131072 and p["image_bytes"] == 73728
    assert p["chunks"][0]["nb"] == (256 << 20) // 131072 // 10 and p["last_chunks"] == 5
    # ... at D = 90 the images do: 64 800-byte factors, 3640 images -> 364 regressors
    p = _plan(exe, many, [10] * 1000, 90)
    _check_plan(p, many, [10] * 1000)
    assert p["chunks"][0]["nb"] == (256 << 20) // 73728 // 10 and p["last_chunks"] == 3
    # the statistics bound it: 67 072-byte slots at D = 128, 4002 of them; a regressor of 8 x 8192-row folds takes 64
    long = [0] + np.cumsum([65536] * 70).tolist()
    p = _plan(exe, long, [8192] * 70, 128, elem=4)
    _check_plan(p, long, [8192] * 70)
    assert p["stat_bytes"] == 67072 and p["chunks"][0]["nb"] == (256 << 20) // 67072 // 64 and p["last_chunks"] == 2
    assert p["tiles_per_group"] == -(-70 * 1024 // 512)
    # one long regressor among short ones: its folds are cut into groups, the short ones are not
    mix = [0, 1024, 1024 + (1 << 20), 2048 + (1 << 20)]
    p = _plan(exe, mix, [103, 104858, 103], 64)
    _check_plan(p, mix, [103, 104858, 103])
    assert max(it[3] for it in p["pred"] if it[0] == 1) > 1 and all(it[3] == 1 for it in p["pred"] if it[0] != 1)


# ---- the code object ---------------------------------------------------------------------------------------------------------------
def test_new_kernels_resources(tmp_path, repo_root):
    """No kflr_* kernel uses more scratch than its kfl_* sibling in the same build (the siblings' own: at most the known 124 B of
    kfl_stats32_kernel<ROWVECS> in fp32, the spills of phase_gram at NB = 4, 7, 8 in fp64); none exceeds 160 KB of LDS or 256
    registers a lane; the bodies exist once."""
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
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            props.setdefault(name, {})[m.group(1)] = int(m.group(2))
    new = {k: v for k, v in props.items() if re.match(r"_ZN3blr\d+kflr_", k)}
    assert len(new) == 24 + 2 + 16 + 2 + 4, sorted(new)  # fp64 statistics, fp32 statistics, factor, reduce, predict
    csrc = os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc")
    lds = {}
    for k, v in new.items():
        sib = re.sub(r"^_ZN3blr(\d+)kflr_", lambda m: f"_ZN3blr{int(m.group(1)) - 1}kfl_", k).replace("8KflrArgs", "7KflArgs")
        assert sib in props, (k, sib)
        print(k, v, props[sib]["private_segment_fixed_size"])
        assert v["private_segment_fixed_size"] <= props[sib]["private_segment_fixed_size"], (k, v, props[sib])
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 256 and v["max_flat_workgroup_size"] == 256, (k, v)
        assert v.get("group_segment_fixed_size", 0) <= 64, (k, v)  # static LDS: at most the block reduction's scratch
        lds[k] = v
    assert max(v["private_segment_fixed_size"] for k, v in props.items() if "kfl_stats32_kernel" in k) <= 124
    # the dynamic LDS the host asks for, from the constants the sources state: SmallCfg<double, 8>::LDS_BYTES is asserted to fit twice
    # into 160 KB where kfl_factor_body is compiled; the predict kernel's and the fp32 statistics kernel's at D = 128
    hpp = open(os.path.join(csrc, "blr_kfold_large.hpp")).read()
    assert 'static_assert(2 * C::LDS_BYTES <= 160 * 1024' in hpp
    assert "return (size_t)kCovTile * (size_t)(DP + 16 / (int)elem) * elem + (size_t)kCovMaxD * elem + (size_t)2 * NB * (NB + 1) * 64 * elem;" in hpp
    assert "return ((size_t)kKflTile * (DP + 1) + 2 * kKflTile + 128) * sizeof(double);" in hpp
    for elem in (8, 4):
        assert 64 * (128 + 16 // elem) * elem + 128 * elem + 2 * 8 * 9 * 64 * elem <= 160 * 1024
    assert (64 * 129 + 2 * 64 + 128) * 8 + 64 <= 160 * 1024
    # one body each, called from both kernels
    rag = open(os.path.join(csrc, "blr_kfold_large_ragged.hpp")).read()
    for body in ("kfl_stats_body<T, NB, MODE>(smem, v);", "kfl_stats32_body<LAYOUT>(smem, scr, v);", "kfl_factor_body<T, NB>(smem, v);",
                 "kfl_predict_body<T, LAYOUT>(smem, v);"):
        assert hpp.count(body) == 1 and rag.count(body) == 1, body
    assert (hpp + rag).count("phase_chol<T, NB, 2>(smem, D, 1)") == 1 and (hpp + rag).count("phase_gram<T, NB, MODE>(smem)") == 1
    assert hpp.count("kfl_reduce_body(") == 2 and rag.count("kfl_reduce_body(") == 1


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,counts,folds", [(D, None, None) for D in K.DS] + [(K.BIG_D, K.BIG_COUNTS, K.BIG_FOLDS)])
def test_gpu_test_inputs_have_no_near_degenerate_fold(D, counts, folds):
    """Every fold of every input tests/test_kfold_large_ragged_gpu.py uses factors in the float64 reference with finite outputs, and
    the cancellation max diag(A) / min diag(A_f) stays below K.CANCEL_CAP (its reasoning: tests/_kfold_large_ragged_data.py)."""
    P = K.batch(D, counts, folds)
    worst = 0.0
    for noise in K.NOISES:
        for dtype in (np.float64, np.float32):
            for b in range(P.nb):
                m, v, lp, cancel = P.reference(noise, dtype, b)   # (np.linalg.cholesky raises on a fold that does not factor)
                assert np.all(np.isfinite(m)) and np.all(np.isfinite(v)) and np.all(np.isfinite(lp)) and np.all(v > 0)
                assert len(lp) == K.nfolds(P.counts[b], P.folds[b])
                worst = max(worst, cancel)
    print("largest cancellation at D =", D, worst)
    assert worst <= K.CANCEL_CAP
