"""CPU-side checks of the ragged condition / forget pair (blr_update_factor_ragged_*, blr_downdate_factor_ragged_*,
ResidentPosteriorBatch): the host-only planner, built with the HOST compiler (tools/revise_ragged_plan_dump.cpp, also
with the host sanitizers as a stand-alone program); the symbols declared, exported and bound with one arity; the argument checks that
need no device; the new kernels' resources from the compiled code object."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as Rg

import _revise_ragged_data as R

NAMES = [f"blr_{d}_factor_ragged_{s}" for d in ("update", "downdate") for s in ("f64", "f32")]
COUNTS = list(R.COUNTS)
OFFSETS = np.concatenate([[0], np.cumsum(COUNTS)]).tolist()


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory, repo_root):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler in this image")
    d = tmp_path_factory.mktemp("revise_ragged_plan")
    src = os.path.join(repo_root, "tools", "revise_ragged_plan_dump.cpp")
    exes = {}
    for tag, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"])):
        exe = str(d / f"revise_ragged_plan_dump_{tag}")
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *extra, "-o", exe, src], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        exes[tag] = exe
    return exes


def _plan(exe, direction, D, offsets, *options):
    r = subprocess.run([exe, direction, str(D), *options, "--", *map(str, offsets)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout)


def test_planner_header_needs_no_hip(repo_root):
    text = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_revise_ragged_plan.hpp")).read()
    assert set(re.findall(r"#include\s+([<\"][^>\"]+[>\"])", text)) == {"<algorithm>", "<cstdint>", "<vector>"}


@pytest.mark.parametrize("tag", ["plain", "san"])
def test_planner_lists(dump, tag):
    exe = dump[tag]
    # counts [0, 1, 2, 16, 17, 3, 0, 1, 40] at D = 40: longest first, ties by index
    p = _plan(exe, "update", 40, OFFSETS)
    assert (p["idle"], p["sweep"], p["refit"]) == ([0, 6], [1, 7], [8, 4, 3, 5, 2]) and not p["serial"] and p["last_chunks"] == 2
    p = _plan(exe, "update", 40, OFFSETS, "SWEEP=always")
    assert (p["idle"], p["sweep"], p["refit"]) == ([0, 6], [3, 5, 2, 1, 7], [8, 4])   # k <= 16 sweeps; 17 and 40 re-factor
    p = _plan(exe, "update", 40, OFFSETS, "SWEEP=never")
    assert (p["idle"], p["sweep"], p["refit"]) == ([0, 6], [], [8, 4, 3, 5, 2, 1, 7]) and p["last_chunks"] == 1
    p = _plan(exe, "downdate", 40, OFFSETS, "SWEEP=never")                            # (SWEEP does not route a downdate)
    assert (p["idle"], p["sweep"], p["refit"]) == ([0, 6], [8, 4, 3, 5, 2, 1, 7], []) and not p["serial"]
    for direction, mode in (("update", "auto"), ("update", "always"), ("update", "never"), ("downdate", "auto")):
        q = _plan(exe, direction, 40, OFFSETS, f"SWEEP={mode}")
        assert (q["sweep"], q["refit"], q["idle"]) == tuple(R.routes(COUNTS, 40, direction, mode))  # the GPU tests' restatement
    # MAX_CHUNK = 2: the lists do not change, the launches do
    q = _plan(exe, "update", 40, OFFSETS, "MAX_CHUNK=2")
    p = _plan(exe, "update", 40, OFFSETS)
    assert (q["idle"], q["sweep"], q["refit"]) == (p["idle"], p["sweep"], p["refit"]) and q["chunk"] == 2 and q["last_chunks"] == 1 + 3
    assert _plan(exe, "downdate", 40, OFFSETS, "MAX_CHUNK=2")["last_chunks"] == 4
    # B = 0, and all idle
    p = _plan(exe, "update", 40, [0])
    assert (p["idle"], p["sweep"], p["refit"], p["last_chunks"]) == ([], [], [], 0)
    p = _plan(exe, "downdate", 40, [5, 5, 5, 5])
    assert (p["idle"], p["sweep"], p["refit"], p["last_chunks"]) == ([0, 1, 2], [], [], 0)
    # D > 128 and NO_DOWNDATE_LDS: one after the other
    p = _plan(exe, "update", 160, [0, 0, 2, 7], "SWEEP=always")
    assert p["serial"] and (p["idle"], p["sweep"], p["refit"], p["last_chunks"]) == ([0], [], [2, 1], 2)
    p = _plan(exe, "downdate", 160, [0, 0, 2, 7])
    assert p["serial"] and (p["idle"], p["sweep"], p["refit"]) == ([0], [2, 1], [])
    assert _plan(exe, "downdate", 40, OFFSETS, "NO_DOWNDATE_LDS=1")["serial"] and not _plan(exe, "update", 40, OFFSETS, "NO_DOWNDATE_LDS=1")["serial"]


def test_route_of_a_regressor_does_not_depend_on_the_others(dump):
    """regressor 2 of five, every k from 0 to 18, while the others' counts (and B) change"""
    exe = dump["plain"]
    rng = np.random.Generator(np.random.PCG64(5))

    def where(p, b):
        return [n for n in ("idle", "sweep", "refit") if b in p[n]]

    for direction, opts in (("update", ()), ("update", ("SWEEP=always",)), ("update", ("SWEEP=never",)), ("downdate", ())):
        for k in range(19):
            seen = set()
            for others in ([0, 0, 0, 0], [1, 1, 1, 1], [40, 2, 17, 1], rng.integers(0, 50, size=4).tolist(), rng.integers(0, 50, size=9).tolist()):
                counts = others[:2] + [k] + others[2:]
                p = _plan(exe, direction, 64, np.concatenate([[3], 3 + np.cumsum(counts)]).tolist(), *opts)
                w = where(p, 2)
                assert len(w) == 1
                seen.add(w[0])
            assert len(seen) == 1, (direction, opts, k, seen)


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------
def _arity(text, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return len([p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()])


def test_symbols_declared_exported_bound_and_one_arity(repo_root):
    header = open(os.path.join(repo_root, "include", "blr_mi355x.h")).read()
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    integ = open(os.path.join(repo_root, "INTEGRATION.md")).read()
    lib = _abi.load_library()
    for name in NAMES:
        assert hasattr(lib, name) and name in _abi.EXPORTED_SYMBOLS
        assert _arity(header, name) == len(_abi._SIGS[name][0]) == 19
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m and len([t for t in m.group(1).split(",") if t.strip()]) == 19, name
        assert name[:-4] in integ
    assert "function update_factor_ragged!(" in jl and "function downdate_factor_ragged!(" in jl
    assert hasattr(_abi.Handle, "update_factor_ragged") and hasattr(_abi.Handle, "downdate_factor_ragged")
    block = header[header.rindex("/* ----", 0, header.index("int blr_update_factor_ragged_f64")):header.index("int blr_update_factor_ragged_f64")]
    block = re.sub(r"\s*\n \* ", " ", block)  # (the comment's line breaks)
    for phrase in ("repeated conditioning", "Bit promises", "B = 1, k = k_b", "bit-for-bit untouched", "ragged_sweep", "no float atomics"):
        assert phrase in block, phrase


def test_resident_posterior_batch_exists():
    assert blr_amd.ResidentPosteriorBatch is Rg.ResidentPosteriorBatch and "ResidentPosteriorBatch" in blr_amd.__all__
    for m in ("condition", "forget", "state", "regressors"):
        assert callable(getattr(blr_amd.ResidentPosteriorBatch, m))


# ---- argument errors through a NULL handle ---------------------------------------------------------------------------------------------
I64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731


def _call(name, **kw):
    D = 4
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=2, D=D, offsets=I64(0, 3, 5), X=np.zeros((D, 5)), ldx=D, y=np.zeros(5),
             noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(2), strides=1, mw=np.zeros((2, D)), stridemw=D, T=np.zeros((2, D, D)), ldt=D,
             strideT=D * D, lp=np.zeros(2), info=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(_abi.load_library(), name)(None, a["memspace"], a["layout"], a["B"], a["D"], p(a["offsets"]), p(a["X"]), a["ldx"], p(a["y"]),
                                              a["noise_kind"], p(a["s"]), a["strides"], p(a["mw"]), a["stridemw"], p(a["T"]), a["ldt"],
                                              a["strideT"], p(a["lp"]), p(a["info"]))


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry points too)
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, D=0) == -5 and _call(name, D=8193, ldx=8193, ldt=8193) == -5
    assert _call(name, offsets=I64(0, 3, 2)) == -6               # a decreasing entry
    assert _call(name, offsets=I64(-1, 3, 5)) == -6              # a negative entry
    assert _call(name, offsets=None) == -6                       # NULL with B > 0
    assert _call(name, X=None) == -7
    assert _call(name, ldx=3) == -8                              # ColVecs: ldx < D
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -8  # RowVecs: ldx < offsets[B]
    assert _call(name, y=None) == -9
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -10       # dense noise
    assert _call(name, s=None) == -11
    assert _call(name, strides=-1) == -12
    assert _call(name, mw=None) == -13
    assert _call(name, stridemw=3) == -14
    assert _call(name, T=None) == -15
    assert _call(name, ldt=3) == -16
    assert _call(name, strideT=15) == -17
    assert _call(name, info=None) == -19
    assert _call(name, memspace=7, layout=2, ldt=0) == -2        # in the order of the arguments
    assert _call(name, B=0) == 0
    assert _call(name) == -1                                     # valid arguments and a NULL handle
    assert _call(name, lp=None) == -1                            # logpdf may be NULL
    assert _call(name, offsets=I64(2, 2, 5), X=np.zeros((4, 5))) == -1  # an idle regressor and offsets[0] > 0 are valid
    assert _call(name, offsets=I64(5, 5, 5), X=None, y=None) == -1      # all idle: no data is needed


# ---- the code object -------------------------------------------------------------------------------------------------------------------
def test_new_kernels_do_not_spill_and_share_the_lifted_bodies(tmp_path, repo_root):
    """the four new instantiations keep the registers of the kernels whose bodies they share (no scratch, no spill), and each body is
    written once"""
    csrc = os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc")
    up, dn, rr = (open(os.path.join(csrc, f)).read() for f in ("blr_update.hpp", "blr_downdate.hpp", "blr_revise_ragged.hpp"))
    assert (up + rr).count("rank1_sweep_body<T>(smem,") == 2 and up.count("void rank1_sweep_body(") == 1
    assert (dn + rr).count("downdate_lds_body<T>(smem,") == 2 and dn.count("void downdate_lds_body(") == 1
    assert (up + dn).count("const T h2 = aj * aj + bj * bj;") == 1 and (up + dn).count("if (iscr[1] != 0) break;") == 1
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
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            props.setdefault(name, {})[m.group(1)] = int(m.group(2))
    pick = lambda pat: {k: v for k, v in props.items() if re.search(pat, k)}
    new = pick(r"update_ragged_sweep_kernel|downdate_ragged_kernel|revise_ragged_idle_kernel")
    assert len(new) == 5, sorted(new)
    old = pick(r"3blr18rank1_sweep_kernelI|3blr19downdate_lds_kernelI")
    assert len(old) == 4, sorted(old)
    for k, v in {**new, **old}.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    for suf in ("IdE", "IfE"):
        for a, b in (("rank1_sweep_kernel", "update_ragged_sweep_kernel"), ("downdate_lds_kernel", "downdate_ragged_kernel")):
            (va,), (vb,) = pick(a + suf).values(), pick(b + suf).values()
            assert va["vgpr_count"] == vb["vgpr_count"], (a, b, suf, va, vb)
