"""CPU-side checks of the batched predictive covariance (blr_mean_and_cov_batched_*, cov_map, mean_and_cov_map, ResidentPosterior.cov,
ResidentColumnsPosterior.cov): the symbols are declared, exported and bound, the header, the binding and the Julia shim
agree on the arity, the argument checks that need no device (they come before the handle check), the routing of the Python functions
with the handle replaced by a recorder, and the register / scratch limits of cov_whiten_kernel and cov_tiles_kernel from the compiled
code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

SYMS = ("blr_mean_and_cov_batched_f64", "blr_mean_and_cov_batched_f32")
ARITY = 25


def _header(repo_root):
    return open(os.path.join(repo_root, "include", "blr_mi355x.h")).read()


def _arity(text, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return len([p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()])


def test_symbols_declared_exported_and_bound(repo_root):
    header = _header(repo_root)
    lib = _abi.load_library()
    for name in SYMS:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert _arity(header, name) == len(_abi._SIGS[name][0]) == ARITY
    assert _abi._SIGS[SYMS[0]] == _abi._SIGS[SYMS[1]]
    assert hasattr(_abi.Handle, "mean_and_cov_batched")
    block = header[header.index("joint predictive covariance of a batch of regressors"):header.index("int blr_mean_and_cov_batched_f64")]
    assert ":33" in block and ":35-38" in block and ":45" in block and "loop of blr_mean_and_cov_*" in block
    assert "correct, not fast" in block and "bit-reproducible" in block and "exactly symmetric" in block
    assert "strideX = 0" in block and "strideLw = 0" in block and "65535" in block and "256 MiB" in block and "synchronises" in block


def test_python_surface():
    for name in ("cov_map", "mean_and_cov_map"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__
    assert callable(blr_amd.ResidentPosterior.cov) and callable(blr_amd.ResidentPosterior.mean_and_cov)
    assert callable(blr_amd.ResidentColumnsPosterior.cov)


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function mean_and_cov_batched!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_mean_and_cov_batched_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, N, B = 4, 5, 2
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=B, D=D, N=N, X=np.zeros((D, N * B)), ldx=D, strideX=D * N,
             noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(N * N * B), lds=N, strides=1, prior_kind=_abi.PRIOR_UPPER_FACTOR, mw=np.zeros(D * B),
             stridemw=D, Lw=np.eye(D), ldl=D, strideLw=0, mean=np.zeros(N * B), stridemean=N, C=np.zeros(N * N * B), ldc=N, strideC=N * N,
             info=np.zeros(B, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], p(a["X"]), a["ldx"], a["strideX"], a["noise_kind"],
                              p(a["s"]), a["lds"], a["strides"], a["prior_kind"], p(a["mw"]), a["stridemw"], p(a["Lw"]), a["ldl"],
                              a["strideLw"], p(a["mean"]), a["stridemean"], p(a["C"]), a["ldc"], a["strideC"], p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, D=0) == -5
    assert _call(name, D=8193) == -5
    assert _call(name, N=-1) == -6
    assert _call(name, N=16385) == -6                                 # the bound of blr_mean_and_cov_*
    assert _call(name, X=None) == -7
    assert _call(name, ldx=3) == -8
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -8
    assert _call(name, strideX=-1) == -9
    assert _call(name, noise_kind=7) == -10
    assert _call(name, s=None) == -11
    assert _call(name, noise_kind=_abi.NOISE_DENSE, lds=4, strides=25) == -12   # dense noise with lds < N
    assert _call(name, strides=-1) == -13
    assert _call(name, prior_kind=7) == -14
    assert _call(name, mw=None) == -15
    assert _call(name, Lw=None) == -17
    assert _call(name, ldl=3) == -18                                  # ldl < D
    assert _call(name, prior_kind=_abi.PRIOR_DENSE, ldl=3) == -18
    assert _call(name, strideLw=-1) == -19
    assert _call(name, stridemean=4) == -21                           # overlapping outputs for B = 2
    assert _call(name, ldc=4) == -23                                  # ldc < N
    assert _call(name, strideC=24) == -24
    assert _call(name, ldc=6, strideC=29) == -24                      # strideC < ldc * N
    assert _call(name, info=None) == -25
    # the ranges come first, in the order of the arguments
    assert _call(name, memspace=7, layout=2, noise_kind=7) == -2
    assert _call(name, N=16385, ldx=0) == -6
    # nothing to do: a no-op, whatever else is passed
    assert _call(name, B=0, info=None, X=None) == 0
    assert _call(name, N=0, info=None, X=None, ldc=-1) == 0
    assert _call(name, mean=None, C=None, info=None, X=None) == 0
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1
    assert _call(name, strideX=0, strides=0, stridemw=0, strideLw=0) == -1              # shared inputs
    assert _call(name, mean=None, mw=None, stridemean=0) == -1                          # covariance only
    assert _call(name, C=None, s=None, Lw=None, ldc=0, strideC=0) == -1                 # mean only
    assert _call(name, B=1, stridemean=0, strideC=0) == -1                              # a single regressor: any output stride
    assert _call(name, noise_kind=_abi.NOISE_DIAGONAL, strides=5) == -1
    assert _call(name, noise_kind=_abi.NOISE_DENSE, lds=5, strides=25) == -1
    assert _call(name, prior_kind=_abi.PRIOR_DIAGONAL, ldl=1, strideLw=4) == -1
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1
    assert _call(name, N=16384, X=np.zeros(1), ldx=4, s=np.ones(1), ldc=16384, strideC=16384 * 16384, stridemean=16384) == -1


class _Recorder:
    """stands in for the library handle: records the entry points; the zero status lets the unpacking go through"""

    def __init__(self):
        self.calls = []
        self.bufs = {}

    # device memory as host arrays, keyed by a made-up pointer
    def device_alloc(self, nbytes):
        ptr = 4096 * (len(self.bufs) + 1)
        self.bufs[ptr] = np.zeros(max(int(nbytes), 1), dtype=np.uint8)
        return ptr

    def device_free(self, ptr):
        self.bufs.pop(ptr, None)

    def memcpy_h2d(self, dptr, host):
        raw = np.asarray(host).reshape(-1, order="A").view(np.uint8)
        self.bufs[dptr][:raw.size] = raw

    def memcpy_d2h(self, host, dptr):
        flat = host.reshape(-1, order="A").view(np.uint8)
        flat[...] = self.bufs[dptr][:flat.size]

    def mean_and_cov_batched(self, *args):
        self.calls.append(("batched", args))
        return 0

    def mean_and_cov(self, *args):
        self.calls.append(("single", args))
        return 0


def _problem(rng, D, N, x=None):
    f = R.BayesianLinearRegressor(rng.standard_normal(D), R.Diagonal(np.exp(0.1 * rng.standard_normal(D))))
    x = R.ColVecs(np.asfortranarray(rng.standard_normal((D, N)))) if x is None else x
    return f(x, R.Diagonal(np.exp(rng.standard_normal(N))))


def test_equal_shapes_make_one_batched_call(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(5)
    D, N, nb = 6, 5, 4
    fxs = [_problem(rng, D, N) for _ in range(nb)]
    out = R.mean_and_cov_map(fxs)
    assert [k for k, _ in rec.calls] == ["batched"] and len(out) == nb
    assert all(m.shape == (N,) and c.shape == (N, N) for m, c in out)
    (dtype, memspace, layout, B, D_, N_, X, ldx, strideX, noise_kind, s, lds, strides, prior_kind, mw, stridemw, Lw, ldl, strideLw,
     mean, stridemean, Cov, ldc, strideC, info) = rec.calls[0][1]
    assert (dtype, memspace, layout, B, D_, N_) == (np.float64, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, nb, D, N)
    assert (ldx, strideX, noise_kind, lds, strides) == (D, D * N, _abi.NOISE_DIAGONAL, N, N)
    assert (prior_kind, stridemw, ldl, strideLw) == (_abi.PRIOR_DIAGONAL, D, 1, D)
    assert (stridemean, ldc, strideC) == (N, N, N * N) and info.shape == (nb,)
    assert np.array_equal(X[2].reshape((D, N), order="F"), fxs[2].x.X) and np.array_equal(mw[3], fxs[3].f.mw)
    # the covariances alone: mean and mw are not passed
    rec.calls.clear()
    out = R.cov_map(fxs)
    assert [k for k, _ in rec.calls] == ["batched"] and [c.shape for c in out] == [(N, N)] * nb
    a = rec.calls[0][1]
    assert a[14] is None and a[19] is None and a[21] is not None


def test_a_shared_input_object_is_passed_once(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(6)
    D, N, nb = 6, 5, 3
    x = R.ColVecs(np.asfortranarray(rng.standard_normal((D, N))))
    fxs = [_problem(rng, D, N, x) for _ in range(nb)]
    R.cov_map(fxs)
    assert [k for k, _ in rec.calls] == ["batched"]
    a = rec.calls[0][1]
    assert a[3] == nb and a[8] == 0 and a[6].shape == (D, N)  # strideX == 0: one copy of X


def test_mixed_shapes_fall_back_to_the_loop(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: rec)
    rng = np.random.default_rng(7)
    D = 6
    fxs = [_problem(rng, D, n) for n in (5, 4, 5)]
    out = R.mean_and_cov_map(fxs)
    assert [k for k, _ in rec.calls] == ["single"] * 3
    assert [c.shape for _, c in out] == [(5, 5), (4, 4), (5, 5)]
    rec.calls.clear()
    assert R.cov_map([]) == [] and R.mean_and_cov_map([]) == [] and rec.calls == []
    # a prior that is not positive definite is reported with its position, before any call
    bad = R.BayesianLinearRegressor(np.zeros(D), R.Diagonal(-np.ones(D)))(fxs[0].x, 0.1)
    with pytest.raises(_abi.PosDefException) as e:
        R.cov_map([fxs[0], bad])
    assert e.value.index == 1 and rec.calls == []


def test_resident_cov_passes_the_resident_pointers(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_abi, "default_handle", lambda: rec)
    rng = np.random.default_rng(8)
    D, N, S = 6, 5, 3
    Lw = R.PDMat(np.triu(rng.standard_normal((D, D))) + 3.0 * np.eye(D))
    st = R.ResidentPosterior(R.BayesianLinearRegressor(rng.standard_normal(D), Lw))
    X = np.asfortranarray(rng.standard_normal((D, N)))
    m, Cv = st.mean_and_cov(R.ColVecs(X), 0.5)
    assert [k for k, _ in rec.calls] == ["batched"] and m.shape == (N,) and Cv.shape == (N, N)
    a = rec.calls[0][1]
    assert a[1] == _abi.MEM_DEVICE and a[3:6] == (1, D, N) and a[9] == _abi.NOISE_ISOTROPIC and a[13] == _abi.PRIOR_UPPER_FACTOR
    assert a[14] == st._mw.ptr and a[16] == st._T.ptr and a[17] == D  # no copy of the factor
    rec.calls.clear()
    cols = R.ResidentColumnsPosterior([R.BayesianLinearRegressor(rng.standard_normal(D), Lw) for _ in range(S)])
    Cv = cols.cov(R.ColVecs(X), R.Diagonal(np.ones(N)))
    assert [k for k, _ in rec.calls] == ["batched"] and Cv.shape == (N, N)
    a = rec.calls[0][1]
    assert a[3] == 1 and a[9] == _abi.NOISE_DIAGONAL and a[14] is None and a[19] is None and a[16] == cols._T.ptr  # ONE call, mean = NULL


def test_cov_kernel_resources(tmp_path):
    """Registers and scratch of every cov_whiten_kernel / cov_tiles_kernel instantiation from the code object's notes: at most 256
    registers each, and no scratch and no spilled register in any of the six (this build gives cov_whiten_kernel
    fp64 ColVecs / RowVecs 114 / 189 registers, fp32 108 / 156; cov_tiles_kernel fp64 108, fp32 69 -- all with 0 B of scratch)."""
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
    whiten = {k: v for k, v in props.items() if "cov_whiten_kernel" in k}
    tiles = {k: v for k, v in props.items() if "cov_tiles_kernel" in k}
    assert len(whiten) == 4, sorted(whiten)  # two element types, ColVecs and RowVecs
    assert len(tiles) == 2, sorted(tiles)    # two element types
    for k, v in {**whiten, **tiles}.items():
        assert v["vgpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_spill_count"] == 0, (k, v)
