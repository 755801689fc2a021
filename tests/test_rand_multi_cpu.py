"""CPU-side checks of the multi-output draws (blr_rand_multi_batched_*, ResidentColumnsPosterior.rand, rand_columns,
rand_columns_map): the symbols are declared, exported and bound, the header, the binding and the Julia shim agree on
the arity, the argument checks that need no device (they come before the handle check), the routing and the RNG order of the Python
functions with the handle replaced by a recorder, and the register / scratch limits of rand_cols_solve_kernel and
rand_cols_project_kernel from the compiled code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

SYMS = ("blr_rand_multi_batched_f64", "blr_rand_multi_batched_f32")
ARITY = 34


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
    assert hasattr(_abi.Handle, "rand_multi_batched")
    block = header[header.index("draws from a batched multi-output state"):header.index("int blr_rand_multi_batched_f64")]
    assert ":49-53" in block and "sampling_functions.jl:16-49" in block and "S calls of blr_rand_batched_*" in block
    assert "correct, not fast" in block and "synchronises" in block and "No float atomics" in block and "NOT promised" in block
    assert "strideX = 0" in block and "strideLw = 0" in block and "strideM = 0" in block
    assert "65535" in block and "256 MiB" in block and "MAX_CHUNK" in block and "last_chunks" in block and "workspace_bytes" in block
    assert "S*R <= 2^20" in block and "(-30)" in block and "(-33)" in block and "-17" in block


def test_python_surface():
    for name in ("rand_columns", "rand_columns_map"):
        assert getattr(blr_amd, name) is getattr(R, name)
        assert name in blr_amd.__all__ and name in R.__all__
    assert callable(blr_amd.ResidentColumnsPosterior.rand)


def test_julia_shim_calls_both_symbols_with_the_header_arity(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    header = _header(repo_root)
    assert "function rand_multi_batched!(" in jl
    for name in SYMS:
        m = re.search(rf"ccall\(\(:{name}, LIB\), Cint,\s*\(([^)]*)\)", jl)
        assert m, name
        types = [t for t in m.group(1).split(",") if t.strip()]
        assert len(types) == _arity(header, name) == ARITY, name


def _call(name, **kw):
    """blr_rand_multi_batched_* with a NULL handle and valid arguments except those in kw."""
    lib = _abi.load_library()
    D, N, B, S, Rr = 4, 5, 2, 3, 2
    SR = S * Rr
    a = dict(memspace=_abi.MEM_HOST, layout=_abi.LAYOUT_COLVECS, B=B, D=D, N=N, S=S, R=Rr, X=np.zeros(D * N * B), ldx=D, strideX=D * N,
             noise_kind=_abi.NOISE_ISOTROPIC, s=np.ones(B), strides=1, prior_kind=_abi.PRIOR_UPPER_FACTOR, M=np.zeros(D * S * B), ldm=D,
             strideM=D * S, Lw=np.eye(D), ldl=D, strideLw=0, Z1=np.zeros(D * SR * B), ldz1=D, strideZ1=D * SR, Z2=np.zeros(N * SR * B),
             ldz2=N, strideZ2=N * SR, W=np.zeros(D * SR * B), ldw=D, strideW=D * SR, Y=np.zeros(N * SR * B), ldy=N, strideY=N * SR,
             info=np.zeros(B, dtype=np.int32))
    a.update(kw)
    p = _abi._ptr
    return getattr(lib, name)(None, a["memspace"], a["layout"], a["B"], a["D"], a["N"], a["S"], a["R"], p(a["X"]), a["ldx"], a["strideX"],
                              a["noise_kind"], p(a["s"]), a["strides"], a["prior_kind"], p(a["M"]), a["ldm"], a["strideM"], p(a["Lw"]),
                              a["ldl"], a["strideLw"], p(a["Z1"]), a["ldz1"], a["strideZ1"], p(a["Z2"]), a["ldz2"], a["strideZ2"],
                              p(a["W"]), a["ldw"], a["strideW"], p(a["Y"]), a["ldy"], a["strideY"], p(a["info"]))


@pytest.mark.parametrize("name", SYMS)
def test_argument_errors_without_a_device(name):
    # (the checks read no element of the data: the float64 buffers only provide non-NULL pointers for the f32 entry point too)
    assert _call(name, memspace=7) == -2
    assert _call(name, layout=2) == -3
    assert _call(name, B=-1) == -4
    assert _call(name, D=0) == -5
    assert _call(name, D=8193) == -5
    assert _call(name, N=-1) == -6
    assert _call(name, N=(1 << 30) + 1) == -6
    assert _call(name, S=-1) == -7
    assert _call(name, R=-1) == -8
    assert _call(name, S=1 << 10, R=(1 << 10) + 1) == -8              # S*R > 2^20
    assert _call(name, X=None) == -9
    assert _call(name, ldx=3) == -10
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=4) == -10
    assert _call(name, strideX=-1) == -11
    assert _call(name, noise_kind=7) == -12
    assert _call(name, noise_kind=_abi.NOISE_DENSE) == -12            # dense noise is not taken
    assert _call(name, s=None) == -13
    assert _call(name, strides=-1) == -14
    assert _call(name, prior_kind=7) == -15
    assert _call(name, M=None) == -16
    assert _call(name, ldm=3) == -17                                  # ldm < D
    assert _call(name, strideM=-1) == -18
    assert _call(name, Lw=None) == -19
    assert _call(name, ldl=3) == -20
    assert _call(name, strideLw=-1) == -21
    assert _call(name, Z1=None) == -22
    assert _call(name, ldz1=3) == -23
    assert _call(name, strideZ1=-1) == -24
    assert _call(name, ldz2=4) == -26
    assert _call(name, strideZ2=-1) == -27
    assert _call(name, ldw=3) == -29
    assert _call(name, strideW=4 * 6 - 1) == -30                      # overlapping outputs for B = 2: strideW < ldw * S * R
    assert _call(name, ldw=5, strideW=29) == -30
    assert _call(name, ldy=4) == -32
    assert _call(name, strideY=5 * 6 - 1) == -33                      # strideY < ldy * S * R
    assert _call(name, ldy=6, strideY=35) == -33
    assert _call(name, info=None) == -34
    # the ranges come first, in the order of the arguments
    assert _call(name, memspace=7, layout=2, noise_kind=7) == -2
    # valid arguments and a NULL handle: -1
    assert _call(name) == -1
    assert _call(name, strideX=0, strides=0, strideM=0, strideLw=0) == -1               # shared inputs
    assert _call(name, Z2=None, s=None) == -1                                           # noise-free: s is not needed ...
    assert _call(name, Z2=None, s=None, noise_kind=_abi.NOISE_DENSE) == -1              # ... and noise_kind is ignored
    assert _call(name, Y=None, X=None) == -1                                            # weights only: X is not needed
    assert _call(name, W=None) == -1
    assert _call(name, N=0, X=None) == -1
    assert _call(name, B=1, strideW=0, strideY=0) == -1                                 # a single regressor: any output stride
    assert _call(name, noise_kind=_abi.NOISE_DIAGONAL, s=np.ones(10), strides=5) == -1
    assert _call(name, prior_kind=_abi.PRIOR_DIAGONAL, ldl=1, strideLw=4) == -1
    assert _call(name, layout=_abi.LAYOUT_ROWVECS, ldx=5) == -1
    assert _call(name, S=1 << 10, R=1 << 10, B=1) == -1                                 # S*R = 2^20 is in range


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

    def rand_multi_batched(self, *args):
        self.calls.append(("multi", args))
        return 0

    def rand_batched(self, *args):
        self.calls.append(("batched", args))
        return 0

    def rand(self, *args):
        self.calls.append(("single", args))
        return 0

    def sample_weights(self, *args):
        self.calls.append(("weights", args))
        return 0


class _RecordingRng:
    """a generator that notes the shape of every block of normals it is asked for"""

    def __init__(self, seed=0):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.shapes = []

    def standard_normal(self, shape):
        self.shapes.append(tuple(shape))
        return self.rng.standard_normal(shape)


def _columns(rng, D, S, Lw=None):
    Lw = Lw if Lw is not None else R.PDMat(np.triu(rng.standard_normal((D, D))) + 3.0 * np.eye(D))
    return [R.BayesianLinearRegressor(rng.standard_normal(D), Lw) for _ in range(S)]


# positions of the arguments of Handle.rand_multi_batched in a recorded call
(I_MEM, I_B, I_D, I_N, I_S, I_R, I_X, I_STRIDEX, I_NK, I_PK, I_M, I_LDM, I_STRIDEM, I_LW, I_STRIDELW, I_Z1, I_STRIDEZ1, I_Z2, I_W,
 I_Y) = 1, 3, 4, 5, 6, 7, 8, 10, 11, 14, 15, 16, 17, 18, 20, 21, 23, 24, 27, 30


def test_rand_columns_routing(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_abi, "default_handle", lambda: rec)
    rng = np.random.default_rng(3)
    D, N, S, Rr = 6, 5, 3, 4
    x = R.ColVecs(np.asfortranarray(rng.standard_normal((D, N))))
    sy = R.Diagonal(np.exp(rng.standard_normal(N)))
    fs = _columns(rng, D, S)
    # columns that share precision, x and noise: ONE call, B = 1
    out = R.rand_columns(np.random.default_rng(1), [f(x, sy) for f in fs], Rr)
    assert [k for k, _ in rec.calls] == ["multi"] and [o.shape for o in out] == [(N, Rr)] * S
    a = rec.calls[0][1]
    assert a[I_MEM] == _abi.MEM_HOST and (a[I_B], a[I_D], a[I_N], a[I_S], a[I_R]) == (1, D, N, S, Rr)
    assert a[I_NK] == _abi.NOISE_DIAGONAL and a[I_PK] == _abi.PRIOR_UPPER_FACTOR and a[I_LDM] == D and a[I_W] is None
    np.testing.assert_array_equal(a[I_M].reshape((D, S), order="F"), np.stack([f.mw for f in fs], axis=1))
    assert a[I_Z1].shape == (1, D * S * Rr) and a[I_Z2].shape == (1, N * S * Rr)
    # regressors: weights only, arrays of function samples
    rec.calls.clear()
    out = R.rand_columns(np.random.default_rng(1), fs, Rr)
    assert [k for k, _ in rec.calls] == ["multi"] and all(o.shape == (Rr,) and isinstance(o[0], R.BLRFunctionSample) for o in out)
    a = rec.calls[0][1]
    assert a[I_N] == 0 and a[I_X] is None and a[I_Y] is None and a[I_Z2] is None and a[I_W].shape == (1, D * S * Rr)
    # mixed columns (two precision objects; unequal noise; two x objects) fall back to the route of rand_map
    for fxs in ([fs[0](x, sy), _columns(rng, D, 1)[0](x, sy)], [fs[0](x, sy), fs[1](x, 0.5)],
                [fs[0](x, sy), fs[1](R.ColVecs(x.X.copy()), sy)]):
        rec.calls.clear()
        out = R.rand_columns(np.random.default_rng(1), fxs, Rr)
        assert "multi" not in [k for k, _ in rec.calls] and rec.calls and len(out) == 2
    # dense noise: one call per column, as rand_map
    rec.calls.clear()
    monkeypatch.setattr(rec, "rand_dense_noise", lambda *args: rec.calls.append(("dense", args)) or 0, raising=False)
    R.rand_columns(np.random.default_rng(1), [f(x, np.eye(N)) for f in fs], Rr)
    assert "multi" not in [k for k, _ in rec.calls]


def test_rand_columns_map_routing(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_abi, "default_handle", lambda: rec)
    rng = np.random.default_rng(4)
    D, N, S, Rr, nb = 6, 5, 3, 2, 4
    x = R.ColVecs(np.asfortranarray(rng.standard_normal((D, N))))
    fss = [_columns(rng, D, S) for _ in range(nb)]
    # one shared x object across the problems: passed once, strideX = 0
    out = R.rand_columns_map(np.random.default_rng(1), [[f(x, 0.3) for f in fs] for fs in fss], Rr)
    assert [k for k, _ in rec.calls] == ["multi"] and len(out) == nb and all(len(o) == S and o[0].shape == (N, Rr) for o in out)
    a = rec.calls[0][1]
    assert (a[I_B], a[I_S], a[I_R]) == (nb, S, Rr) and a[I_STRIDEX] == 0 and a[I_X] is x.X or a[I_X].shape == (D, N)
    assert a[I_STRIDEM] == D * S and a[I_STRIDELW] == D * D and a[I_STRIDEZ1] == D * S * Rr and a[I_M].shape == (nb, D * S)
    # an x object per problem: stacked
    rec.calls.clear()
    xs = [R.ColVecs(np.asfortranarray(rng.standard_normal((D, N)))) for _ in range(nb)]
    R.rand_columns_map(np.random.default_rng(1), [[f(xb, 0.3) for f in fs] for fs, xb in zip(fss, xs)], Rr)
    a = rec.calls[0][1]
    assert [k for k, _ in rec.calls] == ["multi"] and a[I_STRIDEX] == D * N and a[I_X].shape == (nb, D * N)
    # problems of two shapes: one call each
    rec.calls.clear()
    x2 = R.ColVecs(np.asfortranarray(rng.standard_normal((D, N + 2))))
    out = R.rand_columns_map(np.random.default_rng(1), [[f(x, 0.3) for f in fss[0]], [f(x2, 0.3) for f in fss[1]]], Rr)
    assert [k for k, _ in rec.calls] == ["multi", "multi"] and [c[1][I_B] for c in rec.calls] == [1, 1]
    assert out[1][0].shape == (N + 2, Rr)
    assert R.rand_columns_map(np.random.default_rng(1), [], Rr) == []
    # a prior that is not positive definite is reported with the problem's position
    bad = _columns(rng, D, S, Lw=R.Diagonal(-np.ones(D)))
    with pytest.raises(_abi.PosDefException) as e:
        R.rand_columns_map(np.random.default_rng(1), [[f(x, 0.3) for f in fss[0]], [f(x, 0.3) for f in bad]], Rr)
    assert e.value.index == 1


def test_resident_columns_rand_passes_the_resident_pointers(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_abi, "default_handle", lambda: rec)
    rng = np.random.default_rng(8)
    D, N, S, Rr = 6, 5, 3, 4
    st = R.ResidentColumnsPosterior(_columns(rng, D, S))
    X = np.asfortranarray(rng.standard_normal((D, N)))
    Y = st.rand(np.random.default_rng(1), R.ColVecs(X), Rr, Sy=0.5)
    assert [k for k, _ in rec.calls] == ["multi"] and Y.shape == (N, S, Rr) and Y.flags.f_contiguous
    a = rec.calls[0][1]
    assert a[I_MEM] == _abi.MEM_DEVICE and (a[I_B], a[I_D], a[I_N], a[I_S], a[I_R]) == (1, D, N, S, Rr)
    assert a[I_NK] == _abi.NOISE_ISOTROPIC and a[I_PK] == _abi.PRIOR_UPPER_FACTOR
    assert a[I_M] == st._M.ptr and a[I_LW] == st._T.ptr and a[I_LDM] == D and a[I_W] is None  # no copy of the factor
    assert a[I_Z2] is not None
    rec.calls.clear()
    st.rand(np.random.default_rng(1), R.ColVecs(X), Rr)  # noise-free function values
    assert [k for k, _ in rec.calls] == ["multi"] and rec.calls[0][1][I_Z2] is None
    with pytest.raises(NotImplementedError):
        st.rand(np.random.default_rng(1), R.ColVecs(X), Rr, Sy=np.eye(N))


def test_rng_order(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_abi, "default_handle", lambda: rec)
    rng = np.random.default_rng(9)
    D, N, S, Rr = 6, 5, 3, 4
    fs = _columns(rng, D, S)
    x = R.ColVecs(np.asfortranarray(rng.standard_normal((D, N))))
    z1, z2 = (Rr, D), (Rr, N)  # _randn draws the transpose: memory order == draw order
    r = _RecordingRng()
    R.rand_columns(r, [f(x, 0.3) for f in fs], Rr)
    assert r.shapes == [z1, z2] * S                      # Z1_0, Z2_0, Z1_1, Z2_1, ...
    r = _RecordingRng()
    R.rand_columns(r, fs, Rr)
    assert r.shapes == [z1] * S                          # regressors: Z1_c only
    r = _RecordingRng()
    R.rand_columns_map(r, [[f(x, 0.3) for f in fs]] * 2, Rr)
    assert r.shapes == [z1, z2] * (2 * S)
    st = R.ResidentColumnsPosterior(fs)
    r = _RecordingRng()
    st.rand(r, x, Rr, Sy=0.3)
    assert r.shapes == [z1, z2] * S
    r = _RecordingRng()
    st.rand(r, x, Rr)
    assert r.shapes == [z1] * S
    # the same stream as the per-column loop: the normals handed to the library are the loop's
    rec.calls.clear()
    R.rand_columns(np.random.default_rng(5), [f(x, 0.3) for f in fs], Rr)
    a = rec.calls[0][1]
    g = np.random.default_rng(5)
    for c in range(S):
        Z1c, Z2c = R._randn(g, D, Rr, np.float64), R._randn(g, N, Rr, np.float64)
        np.testing.assert_array_equal(a[I_Z1][0].reshape((D, S * Rr), order="F")[:, c * Rr:(c + 1) * Rr], Z1c)
        np.testing.assert_array_equal(a[I_Z2][0].reshape((N, S * Rr), order="F")[:, c * Rr:(c + 1) * Rr], Z2c)


def test_rand_multi_kernel_resources(tmp_path):
    """Registers and scratch of every rand_cols_solve_kernel / rand_cols_project_kernel instantiation from the code object's notes: at
    most 256 registers each, and no scratch and no spilled vector register in any of the six."""
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
    solve = {k: v for k, v in props.items() if "rand_cols_solve_kernel" in k}
    project = {k: v for k, v in props.items() if "rand_cols_project_kernel" in k}
    assert len(solve) == 2, sorted(solve)      # two element types
    assert len(project) == 4, sorted(project)  # two element types, ColVecs and RowVecs
    for k, v in {**solve, **project}.items():
        assert v["vgpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_spill_count"] == 0, (k, v)
