"""CPU-side checks of the ragged evidence grid (blr_logpdf_grid_ragged_*, logpdf_grid_ragged, posterior_best_ragged; DESIGN.md
K30): the symbols declared, exported and bound with one arity; the argument checks that need no device; the host-only planner, built
with the HOST compiler (tools/grid_ragged_plan_dump.cpp, also with the host sanitizers as a stand-alone program); the algebra on the
oracle at unequal counts; the new kernels' resources from the compiled code object."""
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as Rg
from oracle import blr_oracle as O

NAMES = ("blr_logpdf_grid_ragged_f64", "blr_logpdf_grid_ragged_f32")
ARITY = 33
COUNTS = [0, 1, 64, 1023, 2047, 2048, 2049, 9000, 70000]


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
        assert _arity(header, name) == len(_abi._SIGS[name][0]) == ARITY
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m and len([t for t in m.group(1).split(",") if t.strip()]) == ARITY, name
        assert name[:-4] in integ
    assert _abi._SIGS[NAMES[0]] == _abi._SIGS[NAMES[1]]
    assert "function logpdf_grid_ragged!(" in jl
    assert hasattr(_abi.Handle, "logpdf_grid_ragged")
    block = header[header.rindex("/* ----", 0, header.index("int blr_logpdf_grid_ragged_f64")):header.index("int blr_logpdf_grid_ragged_f64")]
    block = re.sub(r"\s*\n \* ", " ", block)  # (the comment's line breaks)
    for phrase in ("bayesian_linear_regression.jl:55-58", "map over fxs of different lengths", "B = 1 on its slice", "independent of B",
                   "permutation of the batch", "host and device memspace give the same bits", "no float atomics"):
        assert phrase in block, phrase


def test_python_surface():
    for name in ("logpdf_grid_ragged", "posterior_best_ragged"):
        assert getattr(blr_amd, name) is getattr(Rg, name)
        assert name in blr_amd.__all__ and name in Rg.__all__


# ---- argument errors through a NULL handle ---------------------------------------------------------------------------------------------
I64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731


def _call(name, **kw):
    D, G = 4, 5
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=2, D=D, offsets=I64(0, 3, 5), X=np.zeros((D, 5)), ldx=D, y=np.zeros(5),
             noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(2), strides=1, prior_kind=_abi.PRIOR_DENSE, mw=np.zeros((2, D)), stridemw=D,
             Lw=np.zeros((2, D, D)), ldl=D, strideLw=D * D, G=G, alpha=np.ones(G), stride_alpha=0, tau=np.ones(G), stride_tau=0,
             logpdf=np.zeros((2, G)), stride_lp=G, best=None, mw_best=None, stride_mwbest=D, T_best=None, ldt=D, strideT=D * D,
             info=np.zeros((2, G), dtype=np.int32), stride_info=G)
    a.update(kw)
    p = _abi._ptr
    return getattr(_abi.load_library(), name)(
        None, a["memspace"], a["layout"], a["B"], a["D"], p(a["offsets"]), p(a["X"]), a["ldx"], p(a["y"]), a["noise_kind"], p(a["s"]),
        a["strides"], a["prior_kind"], p(a["mw"]), a["stridemw"], p(a["Lw"]), a["ldl"], a["strideLw"], a["G"], p(a["alpha"]),
        a["stride_alpha"], p(a["tau"]), a["stride_tau"], p(a["logpdf"]), a["stride_lp"], p(a["best"]), p(a["mw_best"]),
        a["stride_mwbest"], p(a["T_best"]), a["ldt"], a["strideT"], p(a["info"]), a["stride_info"])


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    T = np.zeros((2, 4, 4))
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, D=0) == -5 and _call(name, D=8193, ldx=8193, ldl=8193) == -5
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
    assert _call(name, prior_kind=_abi.PRIOR_UPPER_FACTOR) == -13
    assert _call(name, mw=None) == -14
    assert _call(name, Lw=None) == -16
    assert _call(name, ldl=3) == -17
    assert _call(name, G=-1) == -19
    assert _call(name, stride_alpha=3) == -21
    assert _call(name, stride_tau=3) == -23
    assert _call(name, logpdf=None) == -24
    assert _call(name, stride_lp=4) == -25                       # stride_lp < G
    assert _call(name, mw_best=np.zeros(8), stride_mwbest=3) == -28  # overlapping mw_best
    assert _call(name, T_best=T, ldt=3) == -30
    assert _call(name, T_best=T, strideT=15) == -31              # overlapping T_best
    assert _call(name, info=None) == -32
    assert _call(name, stride_info=4) == -33
    assert _call(name, memspace=7, layout=2, stride_lp=0) == -2  # in the order of the arguments
    assert _call(name) == -1                                     # valid arguments and a NULL handle
    assert _call(name, alpha=None, tau=None) == -1
    assert _call(name, offsets=I64(2, 2, 5), X=np.zeros((4, 5))) == -1  # an empty regressor and offsets[0] > 0 are valid
    assert _call(name, offsets=I64(5, 5, 5), X=None, y=None) == -1      # no observation at all: no data is needed
    assert _call(name, noise_kind=_abi.NOISE_DIAGONAL, s=np.ones(5)) == -1


@pytest.mark.parametrize("name", NAMES)
def test_limits_are_argument_errors_on_g_before_anything_runs(name):
    """B G < 2^24 and sum_b S_b < 2^24 (S_b = 8 from 8192 observations on), else -19 -- with a NULL handle: nothing has run"""
    G = 1 << 20
    off16 = np.arange(17, dtype=np.int64)
    big = dict(G=G, stride_lp=G, stride_info=G, ldx=4)
    assert _call(name, B=16, offsets=off16, **big) == -19                # 16 * 2^20 = 2^24
    assert _call(name, B=15, offsets=off16[:16], **big) == -1
    assert _call(name, B=1 << 24, offsets=np.zeros((1 << 24) + 1, dtype=np.int64), G=0, stride_lp=0, stride_info=0) == -19  # (G = 0 counts as 1)
    nb = 1 << 21
    offsets = 8192 * np.arange(nb + 1, dtype=np.int64)                   # 2^21 regressors of 8 column blocks: 2^24 slots
    assert _call(name, B=nb, offsets=offsets, G=1, stride_lp=1, stride_info=1) == -19
    assert _call(name, B=nb - 1, offsets=offsets[:nb], G=1, stride_lp=1, stride_info=1) == -1
    assert _call(name, B=nb, offsets=offsets, G=1, stride_lp=1, stride_info=1, D=129, ldx=129, ldl=129) == -1  # (D > 128: no slots)
    assert _call(name, B=nb, offsets=offsets, G=1, stride_lp=0, stride_info=1) == -25                         # the other checks come first


def test_factor_prior_error_text():
    """the text blr_logpdf_grid_* uses (read from the source: a NULL handle keeps no text)"""
    src = open(os.path.join(os.path.dirname(_abi.LIB_PATH), "blr_abi.hip")).read()
    body = src[src.index("int logpdf_grid_ragged(blr_handle* h"):]
    assert "pass a carried-forward factor as U'U" in body[:body.index("if (!h) return -1;")]


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory, repo_root):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler in this image")
    d = tmp_path_factory.mktemp("grid_ragged_plan")
    src = os.path.join(repo_root, "tools", "grid_ragged_plan_dump.cpp")
    exes = {}
    for tag, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"])):
        exe = str(d / f"grid_ragged_plan_dump_{tag}")
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *extra, "-o", exe, src], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        exes[tag] = exe
    return exes


def _plan(exe, counts, first=0):
    offsets = np.concatenate([[first], first + np.cumsum(counts)]).astype(np.int64).tolist()
    r = subprocess.run([exe, *map(str, offsets)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout)


def grid_splits(N):
    """csrc/blr_grid.hpp grid_splits, restated"""
    S = max(1, min(8, N // 1024))
    c = -(-N // S)
    return S, max(-(-c // 64) * 64, 64)


def test_planner_header_needs_no_hip(repo_root):
    text = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_grid_ragged_plan.hpp")).read()
    assert set(re.findall(r"#include\s+([<\"][^>\"]+[>\"])", text)) == {"<algorithm>", "<cstdint>", "<vector>"}
    grid = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_grid.hpp")).read()
    body = lambda t, name: re.sub(r"\s+|const ", "", t[t.index(f"inline void {name}("):].split("\n}\n")[0].split("{", 1)[1])  # noqa: E731
    assert body(text, "grid_ragged_splits") == body(grid, "grid_splits")  # the restatement is the original, token for token


@pytest.mark.parametrize("tag", ["plain", "san"])
def test_planner_items_slots_and_order(dump, tag):
    counts = [COUNTS[i] for i in (4, 0, 8, 2, 6, 1, 7, 3, 5)]  # scrambled
    p = _plan(dump[tag], counts, first=11)
    nb = len(counts)
    S = [grid_splits(n)[0] for n in counts]
    assert S == [1, 1, 8, 1, 2, 1, 8, 1, 2]
    assert p["slot0"] == np.concatenate([[0], np.cumsum(S)]).tolist() and p["slots"] == sum(S) == len(p["items"]) and p["reduce"]
    by_reg = {b: sorted((it for it in p["items"] if it["reg"] == b), key=lambda it: it["slot"]) for b in range(nb)}
    assert sorted(it["slot"] for it in p["items"]) == list(range(sum(S)))  # dense
    for b, n in enumerate(counts):
        Sb, chunk = grid_splits(n)
        its = by_reg[b]
        # the boundaries of grid_splits(N_b), block 0 first: every observation in exactly one item
        assert [(it["slot"], it["n0"], it["n"]) for it in its] == [(p["slot0"][b] + k, k * chunk, max(0, min(chunk, n - k * chunk))) for k in range(Sb)]
        assert sum(it["n"] for it in its) == n
    # longest block first, ties by (regressor, block)
    key = [(-it["n"], it["reg"], it["slot"]) for it in p["items"]]
    assert key == sorted(key)
    assert p["items"][0]["n"] == 8768 and p["items"][0]["reg"] == 2  # ceil(70000 / 8) in whole stages of 64
    # all S_b = 1: no reduce launch; B = 0: nothing
    q = _plan(dump[tag], [5, 0, 1023])
    assert not q["reduce"] and q["slot0"] == [0, 1, 2, 3] and [it["reg"] for it in q["items"]] == [2, 0, 1]
    e = _plan(dump[tag], [])
    assert e["items"] == [] and e["slot0"] == [0] and e["slots"] == 0


def test_plan_of_a_regressor_does_not_depend_on_the_others(dump):
    exe = dump["plain"]
    rng = np.random.Generator(np.random.PCG64(5))
    for n in COUNTS:
        seen = set()
        for others in ([0, 0, 0, 0], [1, 1, 1, 1], [9000, 2, 2049, 64], rng.integers(0, 5000, size=4).tolist(), rng.integers(0, 5000, size=9).tolist()):
            counts = others[:2] + [n] + others[2:]
            p = _plan(exe, counts, first=3)
            its = sorted((it for it in p["items"] if it["reg"] == 2), key=lambda it: it["slot"])
            seen.add(tuple((it["slot"] - p["slot0"][2], it["n0"], it["n"]) for it in its))
        assert len(seen) == 1, (n, seen)


# ---- the algebra, per regressor of a packed batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,noise,prior", [(7, "diag", "dense"), (32, "iso", "diag")])
def test_formula_block_agrees_with_the_oracle(D, noise, prior):
    """the algebra of csrc/blr_grid_ragged.hpp in numpy, fp64: the statistics of a regressor summed over its column blocks in the
    plan's order, the regressor's own N in the evidence, against logpdf_literal / posterior_literal with Lw = alpha L0, Sy = tau S0"""
    rng = np.random.Generator(np.random.PCG64(4343 + D))
    for N in (1, 150, 2049):
        X, mw, L0, s0 = O.generate_toy_problem(rng, N, D, dense_noise_cov=False)
        if noise == "iso":
            s0 = np.full(N, 0.8)
        if prior == "diag":
            L0 = np.diag(np.exp(0.3 * rng.standard_normal(D)))
        y = rng.standard_normal(N)
        W = 1.0 / s0
        d = y - X.T @ mw
        S, chunk = grid_splits(N)
        G0, b0, q0, l0 = np.zeros((D, D)), np.zeros(D), 0.0, 0.0
        for k in range(S):
            sl = slice(k * chunk, min(N, (k + 1) * chunk))
            G0 += (X[:, sl] * W[sl]) @ X[:, sl].T
            b0 += X[:, sl] @ (W[sl] * d[sl])
            q0 += float(d[sl] @ (W[sl] * d[sl]))
            l0 += float(np.sum(np.log(s0[sl])))
        ld0 = np.linalg.slogdet(L0)[1]
        for a in (0.1, 1.0, 10.0):
            for t in (0.1, 1.0, 10.0):
                T = np.linalg.cholesky(a * L0 + G0 / t).T
                u = np.linalg.solve(T.T, b0 / t)
                lp = -0.5 * (N * math.log(2 * math.pi) + N * math.log(t) + l0 + q0 / t + 2 * np.sum(np.log(np.diag(T))) - D * math.log(a)
                             - ld0 - u @ u)
                m = mw + np.linalg.solve(T, u)
                lp_o = O.logpdf_literal(mw, a * L0, X, t * s0, y)
                m_o, _, A_o = O.posterior_literal(mw, a * L0, X, t * s0, y)
                assert abs(lp - lp_o) <= 1e-10 * abs(lp_o)
                assert np.linalg.norm(m - m_o) <= 1e-10 * np.linalg.norm(m_o)
                assert np.max(np.abs(T.T @ T - A_o)) <= 1e-10 * np.max(np.abs(A_o))


# ---- the copied kernel bodies ------------------------------------------------------------------------------------------------------------
def _body(text, name):
    """the body of `void name(...)`, comments and white space removed"""
    i = text.index("{", text.index(f"void {name}("))
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            break
        j += 1
    return re.sub(r"\s+", "", re.sub(r"//[^\n]*", "", text[i + 1:j]))


def _sub(body, pairs):
    for old, new in pairs:
        old, new = re.sub(r"\s+", "", old), re.sub(r"\s+", "", new)
        assert old in body, old
        body = body.replace(old, new)
    return body


def test_copied_kernel_bodies_are_the_originals_with_the_stated_differences(repo_root):
    """csrc/blr_grid_ragged.hpp carries copies of three kernel bodies of csrc/blr_grid.hpp: the copies are the originals
    token for token once the differences K30 states are applied -- the slot and N of a regressor come from the plan's tables, the
    constants carry this unit's names, the phases its TAG.  A change to one side that the other does not follow fails here."""
    csrc = os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc")
    grid, ragged = (open(os.path.join(csrc, f)).read() for f in ("blr_grid.hpp", "blr_grid_ragged.hpp"))
    names = [("kGridNoBad", "kEvidenceNoBad"), ("grid_stat_elems", "evidence_stat_elems")]
    # the per-setting kernel: the whole body
    want = _sub(_body(grid, "grid_eval_kernel"), names + [
        ("const int64_t slot = reg * a.S;", "const int64_t slot = a.slot0[reg];"),
        ("phase_chol<T, NB, 1>", "phase_chol<T, NB, kEvidenceTag>"),
        ("phase_backsolve<T, NB, 1>", "phase_backsolve<T, NB, kEvidenceTag>"),
        ("N = (double)a.N;", "N = (double)(int)(a.offsets[reg + 1] - a.offsets[reg]);")])
    assert _body(ragged, "ragged_evidence_eval_kernel") == want
    # the statistics kernel: from the Gram phase on (in front of it the context comes from the item and `offsets` instead of strides)
    tail = lambda b: b[b.index("phase_gram<T,NB,MODE>(smem);"):]  # noqa: E731
    assert tail(_body(ragged, "ragged_evidence_stats_kernel")) == tail(_sub(_body(grid, "grid_stats_kernel"), names))
    head = _body(ragged, "ragged_evidence_stats_kernel")
    head = head[:head.index("phase_gram<T,NB,MODE>(smem);")]
    for field in ("ctx->X=", "ctx->y=", "ctx->s=", "ctx->mw=", "ctx->Lw=ctx->mw;", "ctx->ldx=a.ldx;", "ctx->ldl=0;", "ctx->D=a.D;", "ctx->N=it.n;",
                  "ctx->noise_kind=a.noise_kind;", "ctx->prior_kind=kEvidencePriorNone;"):
        assert field in head, field
    # the reduce kernel: the sums (in front of them the slot comes from slot0 instead of reg * S)
    sums = lambda b: b[b.index("for(intidx="):]  # noqa: E731
    want = _sub(sums(_body(grid, "grid_reduce_kernel")), [("a.S", "S"), ("reg * S", "slot")])
    assert sums(_body(ragged, "ragged_evidence_reduce_kernel")) == want
    consts = lambda t, n: re.search(rf"constexpr int {n} = ([^;]+);", t).group(1)  # noqa: E731
    assert consts(grid, "kGridNoBad") == consts(ragged, "kEvidenceNoBad") and consts(grid, "kGridPriorNone") == consts(ragged, "kEvidencePriorNone")


# ---- the code object -------------------------------------------------------------------------------------------------------------------
def test_new_kernels_keep_the_grid_kernels_bounds(tmp_path):
    """the bounds of tests/test_grid_cpu.py on the new kernels: at most 256 registers; the statistics kernel -- a thin caller of
    phase_gram -- no more scratch than fused_small_kernel of the same <T, NB, MODE> and at most 4 spilled registers; the per-setting
    kernel at most 128 B of scratch and 12 spills"""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    so = shutil.copy(_abi.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    cos = [p for p in os.listdir(tmp_path) if "gfx950" in p]
    assert cos, "no gfx950 code object in the library"
    notes = "".join(subprocess.run([readelf, "--notes", str(tmp_path / c)], check=True, capture_output=True, text=True).stdout for c in sorted(cos))
    props, name = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            props.setdefault(name, {})[m.group(1)] = int(m.group(2))
    new = {k: v for k, v in props.items() if re.search(r"ragged_evidence_(stats|reduce|eval)_kernel", k)}
    stats = [k for k in new if "ragged_evidence_stats_kernel" in k]
    assert len(stats) == 48 and len([k for k in new if "ragged_evidence_eval_kernel" in k]) == 16
    assert len([k for k in new if "ragged_evidence_reduce_kernel" in k]) == 2
    assert not [k for k in new if re.search(r"grid_(eval|stats|prior)_kernel", k)]  # (tests/test_grid_cpu.py counts those names)
    for k, v in new.items():
        assert v["vgpr_count"] <= 256, (k, v)
        if k in stats:
            twin = k.replace("28ragged_evidence_stats_kernel", "18fused_small_kernel").replace("18RaggedEvidenceArgs", "13PosteriorArgs")
            assert twin in props, twin
            assert v["private_segment_fixed_size"] <= props[twin]["private_segment_fixed_size"], (k, v, props[twin])
            assert v["vgpr_spill_count"] <= 4, (k, v)
        else:
            assert v["private_segment_fixed_size"] <= 128, (k, v)
            assert v["vgpr_spill_count"] <= 12, (k, v)
