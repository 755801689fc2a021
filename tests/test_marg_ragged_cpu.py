"""CPU-side checks of the ragged marginals and leave-one-out (blr_marginals_ragged_*, blr_loo_ragged_*): the symbols
are declared, exported and bound with one arity in the header, the binding and the Julia shim; the argument checks that need no
device; the host-only planner of the work items (tools/ragged_items_dump.cpp, also built and run with the host sanitizers as a
stand-alone program); the routing of the Python front end with the handle's methods replaced; and the new kernels' register and
LDS limits from the compiled code object."""
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

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARITY = {"blr_marginals_ragged_f64": 20, "blr_marginals_ragged_f32": 20, "blr_loo_ragged_f64": 22, "blr_loo_ragged_f32": 22}
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
    assert "function marginals_ragged!(" in jl and "function loo_ragged!(" in jl
    assert hasattr(_abi.Handle, "marginals_ragged") and hasattr(_abi.Handle, "loo_ragged")
    for name in ("mean_ragged", "var_ragged", "mean_and_var_ragged", "loo_ragged"):
        assert getattr(blr_amd, name) is getattr(R, name) and name in blr_amd.__all__ and name in R.__all__
    for sym in ("blr_marginals_ragged_f64", "blr_loo_ragged_f64"):
        block = header[header.rindex("/* ----", 0, header.index(f"int {sym}")):header.index(f"int {sym}")]
        block = re.sub(r"\s*\n \* ", " ", block)  # (the comment's line breaks)
        assert "map over fxs of different lengths" in block and "Bit promises" in block


def test_ragged_item_switch_is_documented_and_parsed(repo_root):
    """RAGGED_ITEM in the places tests/test_abi_cpu.py asks of every other switch: blr_host.hpp's tables, the header, the README's
    switch paragraph and the binding's set_option docstring."""
    host = open(os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc", "blr_host.hpp")).read()
    assert re.search(r'Y\("RAGGED_ITEM", set_ragged_item\)', host) and host.count("BLR_PLANNER_OPTIONS(BLR_X)") == 2
    header = open(os.path.join(repo_root, "include", "blr_mi355x.h")).read()
    opts = header[header.index("MAX_CHUNK = 1..65535") - 600:header.index("MAX_CHUNK = 1..65535")]
    assert "RAGGED_ITEM" in opts
    assert "`RAGGED_ITEM" in open(os.path.join(repo_root, "README.md")).read()
    assert "RAGGED_ITEM" in _abi.Handle.set_option.__doc__


def _marg(name, **kw):
    D = 4
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=2, D=D, offsets=I64(0, 3, 5), X=np.zeros((D, 5)), ldx=D,
             noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(2), strides=1, prior_kind=_abi.PRIOR_DENSE, mw=np.zeros(D), stridemw=0, Lw=np.eye(D),
             ldl=D, strideLw=0, mean=np.zeros(5), var=np.zeros(5), info=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(_abi.load_library(), name)(None, a["memspace"], a["layout"], a["B"], a["D"], p(a["offsets"]), p(a["X"]), a["ldx"], a["noise_kind"],
                                              p(a["s"]), a["strides"], a["prior_kind"], p(a["mw"]), a["stridemw"], p(a["Lw"]), a["ldl"], a["strideLw"],
                                              p(a["mean"]), p(a["var"]), p(a["info"]))


def _loo(name, **kw):
    D = 4
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=2, D=D, offsets=I64(0, 3, 5), X=np.zeros((D, 5)), ldx=D, y=np.zeros(5),
             noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(2), strides=1, mw=np.zeros((2, D)), stridemw=D, T=np.zeros((2, D, D)), ldt=D,
             strideT=D * D, lm=np.zeros(5), lv=np.zeros(5), ll=np.zeros(5), tot=np.zeros(2), info=np.zeros(2, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(_abi.load_library(), name)(None, a["memspace"], a["layout"], a["B"], a["D"], p(a["offsets"]), p(a["X"]), a["ldx"], p(a["y"]),
                                              a["noise_kind"], p(a["s"]), a["strides"], p(a["mw"]), a["stridemw"], p(a["T"]), a["ldt"], a["strideT"],
                                              p(a["lm"]), p(a["lv"]), p(a["ll"]), p(a["tot"]), p(a["info"]))


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_argument_errors_without_a_device(suf):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry points too)
    for call, name, pos in ((_marg, f"blr_marginals_ragged_{suf}", dict(noise=-9, s=-10, ld=-16, info=-20)),
                            (_loo, f"blr_loo_ragged_{suf}", dict(noise=-10, s=-11, ld=-16, info=-22))):
        assert call(name, offsets=I64(0, 3, 2)) == -6               # a decreasing entry
        assert call(name, offsets=I64(-1, 3, 5)) == -6              # a negative entry
        assert call(name, offsets=None) == -6                       # NULL with B > 0
        assert call(name, offsets=I64(0, 3, 3 + 2**30 + 1)) == -6   # a regressor beyond 2^30
        assert call(name, ldx=3) == -8                              # ColVecs: ldx < D
        assert call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -8  # RowVecs: ldx < offsets[B]
        assert call(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1
        assert call(name, noise_kind=_abi.NOISE_DENSE) == pos["noise"]
        assert call(name, **({"ldl": 3} if call is _marg else {"ldt": 3})) == pos["ld"]
        assert call(name, info=None) == pos["info"]
        assert call(name, X=None) == -7
        assert call(name, s=None) == pos["s"]
        assert call(name, B=0) == 0
        assert call(name) == -1                                     # valid arguments and a NULL handle
        assert call(name, offsets=I64(2, 2, 5)) == -1               # an empty regressor and offsets[0] > 0 are valid
    assert _loo(f"blr_loo_ragged_{suf}", y=None) == -9
    # var == NULL: neither s nor Lw is read
    assert _marg(f"blr_marginals_ragged_{suf}", var=None, s=None, Lw=None) == -1


# ---- the planner -------------------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 15, 16, 17, 63, 64, 65, 0, 5000, 64, 64, 0, 200]
OFFSETS = np.concatenate([[5], 5 + np.cumsum(COUNTS)]).tolist()


@pytest.fixture(scope="module")
def dump(tmp_path_factory, repo_root):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc in this image")
    d = tmp_path_factory.mktemp("ragged_items")
    src = os.path.join(repo_root, "tools", "ragged_items_dump.cpp")
    exes = {}
    for tag, extra in (("plain", []), ("san", ["-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"])):
        exe = str(d / f"ragged_items_dump_{tag}")
        r = subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", *extra, "-o", exe, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        exes[tag] = exe
    return exes


def _plan(exe, offsets, options=(), cus=256, elem=8):
    r = subprocess.run([exe, str(cus), str(elem), *options, "--", *map(str, offsets)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout)


def _check_plan(p, offsets):
    counts = np.diff(offsets)
    W = p["W"]
    assert W % 64 == 0 and W >= 64
    covered = [np.zeros(n, dtype=int) for n in counts]
    for reg, t0, nt in p["items"]:
        assert nt >= 1 and 16 * t0 < counts[reg] and (16 * t0) % W == 0       # inside ONE regressor, at an item boundary
        lo, hi = 16 * t0, min(16 * (t0 + nt), counts[reg])
        assert 16 * (t0 + nt) < counts[reg] + 16 and hi - lo <= W               # no tile past the regressor, at most W observations
        covered[reg][lo:hi] += 1
    assert all(np.all(c == 1) for c in covered)                                 # every observation exactly once; an empty regressor has no item
    regs = [it[0] for it in p["items"]]
    assert regs == sorted(regs)
    pos = b = 0
    for c in p["chunks"]:
        assert c["b0"] == b and c["nb"] >= 1 and c["item0"] == pos and c["nb"] <= 65535 and c["nb"] * p["image_bytes"] <= 256 << 20
        assert all(c["b0"] <= it[0] < c["b0"] + c["nb"] for it in p["items"][pos:pos + c["nitems"]])
        pos, b = pos + c["nitems"], b + c["nb"]
    assert pos == len(p["items"]) and b == len(counts) and p["last_chunks"] == len(p["chunks"])
    for reg, n in enumerate(counts):
        assert sum(1 for it in p["items"] if it[0] == reg) == -(-int(n) // W)


@pytest.mark.parametrize("tag", ["plain", "san"])
def test_planner(dump, tag):
    exe = dump[tag]
    base = _plan(exe, OFFSETS)
    _check_plan(base, OFFSETS)
    assert base["W"] == 256 and base["last_chunks"] == 1                         # 5 549 observations over 512 slots: the floor
    forced = _plan(exe, OFFSETS, ["RAGGED_ITEM=64"])
    _check_plan(forced, OFFSETS)
    assert forced["W"] == 64 and sum(1 for it in forced["items"] if it[0] == 9) == 79
    chunked = _plan(exe, OFFSETS, ["RAGGED_ITEM=64", "MAX_CHUNK=3"])
    _check_plan(chunked, OFFSETS)
    assert chunked["last_chunks"] == 5 and chunked["items"] == forced["items"] and all(c["nb"] <= 3 for c in chunked["chunks"])
    # one regressor far longer than the default W, fp32 images
    long = [0, 3_000_000, 3_000_100]
    p = _plan(exe, long, elem=4)
    _check_plan(p, long)
    assert p["W"] == 5888 and len(p["items"]) == 511
    # the order of equal-count neighbours does not matter: regressors 10 and 11 both hold 64 observations
    cnt = list(COUNTS)
    cnt[10], cnt[11] = cnt[11], cnt[10]
    assert _plan(exe, np.concatenate([[5], 5 + np.cumsum(cnt)]).tolist()) == base
    # a chunk's images stay within 256 MiB: 73 728-byte fp64 images, 3640 of them
    many = list(range(0, 4001))
    p = _plan(exe, many)
    _check_plan(p, many)
    assert p["chunks"][0]["nb"] == (256 << 20) // 73728 and p["last_chunks"] == 2


# ---- routing of the Python front end ---------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []
        self.next = 1000

    def device_alloc(self, n):
        self.next += 1000
        return self.next

    def device_free(self, p):
        pass

    def memcpy_h2d(self, d, a):
        pass

    def memcpy_d2h(self, a, d):
        a[...] = 0

    def posterior_ragged(self, *args):
        self.calls.append(("posterior_ragged", args))

    def loo_ragged(self, *args):
        self.calls.append(("loo_ragged", args))

    def marginals_ragged(self, *args):
        self.calls.append(("marginals_ragged", args))
        args[-1][...] = 0


def test_routing(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(3)
    D, off = 6, [0, 3, 3, 10, 15]
    f = R.BayesianLinearRegressor(rng.standard_normal(D), R.Diagonal(np.ones(D)))
    X = np.asfortranarray(rng.standard_normal((D, 15)))
    out = R.loo_ragged(f, R.ColVecs(X), off, R.Diagonal(np.ones(15)), rng.standard_normal(15))
    assert [k for k, _ in rec.calls] == ["posterior_ragged", "loo_ragged"] and len(out) == 4 and out[2].mean.shape == (7,)
    pa, la = rec.calls[0][1], rec.calls[1][1]
    assert pa[1] == la[1] == _abi.MEM_DEVICE and pa[5].tolist() == la[5].tolist() == off
    assert (pa[6], pa[8], pa[10]) == (la[6], la[8], la[10])          # X, y, s: the same device pointers
    assert (pa[18], pa[20]) == (la[12], la[14])                      # the state goes from one call to the other on the device
    rec.calls.clear()
    m = R.mean_ragged(f, R.ColVecs(X), off)
    assert [k for k, _ in rec.calls] == ["marginals_ragged"] and m.shape == (15,)
    a = rec.calls[0][1]
    assert a[9] is None and a[14] is None and a[18] is None and a[17] is m  # s, Lw and var are NULL
    rec.calls.clear()
    R.mean_and_var_ragged(f, R.ColVecs(X), off, 0.5)
    a = rec.calls[0][1]
    assert a[9] is not None and a[14] is not None and a[17] is not None and a[18] is not None


# ---- the code object ---------------------------------------------------------------------------------------------------------------
def test_new_kernels_stay_within_their_launch_bounds(tmp_path):
    """256 threads = one wave per SIMD: 512 registers a lane at one workgroup per CU, 256 at the two per CU the gemm-form kernels are
    bound to (their 74 752 / 37 376 bytes of dynamic LDS fit twice into 160 KiB); no scratch, no spill."""
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
        m = re.match(r"\s+(?:- )?\.(name|vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            props.setdefault(name, {})[m.group(1)] = int(m.group(2))
    new = {k: v for k, v in props.items() if re.search(r"marg_ragged_(gemm|rows)_kernel|loo_ragged_(check|total)_kernel", k)}
    assert len(new) == 15, sorted(new)  # 2 x (4 gemm + 2 rows + 1 check) + the total
    for k, v in new.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        regs = v["vgpr_count"] + v.get("agpr_count", 0)
        assert regs <= (256 if "gemm" in k else 512), (k, v)
        assert v["group_segment_fixed_size"] <= 4096, (k, v)


def test_gemm_form_lds_fits_twice_per_cu(repo_root):
    """The dynamic LDS of marg_ragged_gemm_kernel is MargGemmCfg<T>::LDS_BYTES at its launch (blr_abi.hip): evaluated from the
    constants of blr_marg_image.hpp as the source states them, two workgroups must fit the CU's 160 KiB."""
    csrc = os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc")
    img = open(os.path.join(csrc, "blr_marg_image.hpp")).read()
    abi = open(os.path.join(csrc, "blr_abi.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(gk, dim3\(\(unsigned\)c\.nitems\), dim3\(kThreads\), G::LDS_BYTES,", abi)
    kpb = int(re.search(r"constexpr int kPB = (\d+);", img).group(1))
    nfrag = eval(re.search(r"NFRAG = ([0-9 *]+);", img).group(1))
    assert re.search(r"IMG_ELEMS = NFRAG \* 64;", img) and re.search(r"OFF_MW = IMG_ELEMS \* \(int\)sizeof\(T\);", img)
    assert re.search(r"LDS_BYTES = OFF_MW \+ kPB \* \(int\)sizeof\(T\);", img)
    hpp = open(os.path.join(csrc, "blr_marg_ragged.hpp")).read()
    assert "__launch_bounds__(kThreads, 2) void marg_ragged_gemm_kernel" in hpp
    for size in (8, 4):
        assert 2 * (nfrag * 64 + kpb) * size <= 160 * 1024


LOG2PI = float(np.log(2.0 * np.pi))


def test_closed_form_against_literal_refits():
    """The reference of tests/test_marg_ragged_gpu.py itself, once, at the smallest shape: the header's closed form (float64 /
    longdouble) against posterior_literal refits without observation n."""
    from oracle import blr_oracle as O

    rng = np.random.Generator(np.random.PCG64(4242))
    D, N = 17, 17
    X = rng.standard_normal((D, N)) * (0.7 / np.sqrt(D))
    y, s, mw0 = rng.standard_normal(N), np.exp(0.3 * rng.standard_normal(N)), rng.standard_normal(D)
    U = np.triu(rng.standard_normal((D, D))) * (0.3 / np.sqrt(D))
    U[np.diag_indices(D)] = 1.0 + np.abs(U[np.diag_indices(D)])
    Lw = U.T @ U
    mwp, T, _ = O.posterior_literal(mw0, Lw, X, np.diag(s), y)
    Z = np.linalg.solve(T.T, X)
    sig2 = np.sum(Z * Z, axis=0).astype(np.longdouble)
    omh = (s.astype(np.longdouble) - sig2) / s
    r = y - (X.T @ mwp).astype(np.longdouble)
    m, v = y - r / omh, s / omh
    lp = -0.5 * (LOG2PI + np.log(s.astype(np.longdouble)) - np.log(omh) + r * r / (s * omh))
    for n in range(N):
        rest = [i for i in range(N) if i != n]
        mr, Tr, _ = O.posterior_literal(mw0, Lw, X[:, rest], np.diag(s[rest]), y[rest])
        z = np.linalg.solve(Tr.T, X[:, n])
        var, mean = z @ z + s[n], X[:, n] @ mr
        assert float(m[n]) == pytest.approx(mean, rel=1e-9, abs=1e-9) and float(v[n]) == pytest.approx(var, rel=1e-9)
        assert float(lp[n]) == pytest.approx(-0.5 * (LOG2PI + np.log(var) + (y[n] - mean) ** 2 / var), rel=1e-9, abs=1e-9)
