"""CPU-side checks of the batched draws (blr_rand_batched_*, rand_map): the symbols are declared, exported and bound, the Julia
shim calls them, and rand_map's normals, packing and grouping (with the library call replaced by a recorder)."""
import os
import re

import numpy as np
import pytest

import blr_amd
from blr_amd import _abi
from blr_amd import regressor as R

SYMS = ("blr_rand_batched_f64", "blr_rand_batched_f32")


def test_symbols_declared_exported_and_bound(repo_root):
    header = open(os.path.join(repo_root, "include", "blr_mi355x.h")).read()
    lib = _abi.load_library()
    for name in SYMS:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS and len(_abi._SIGS[name][0]) == 32
    assert hasattr(_abi.Handle, "rand_batched")
    assert "rand_map" in blr_amd.__all__ and blr_amd.rand_map is R.rand_map
    assert hasattr(blr_amd.ResidentPosterior, "rand")


def test_julia_shim_calls_both_symbols(repo_root):
    jl = open(os.path.join(repo_root, "julia", "BLRMI355X.jl")).read()
    for name in SYMS:
        assert re.search(rf"ccall\(\(:{name}, LIB\)", jl), name
    assert "function rand_map(" in jl and "function rand_batched!(" in jl


class _Recorder:
    """Stands in for the library handle: records every call and fills the outputs with recognisable values."""

    def __init__(self):
        self.calls = []

    def rand_batched(self, dtype, memspace, layout, B, D, N, S, X, ldx, strideX, noise_kind, s, strides, prior_kind, mw, stridemw,
                     Lw, ldl, strideLw, Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info):
        self.calls.append(("rand_batched", dict(dtype=dtype, memspace=memspace, layout=layout, B=B, D=D, N=N, S=S, X=X, ldx=ldx,
                                                strideX=strideX, noise_kind=noise_kind, s=s, strides=strides, prior_kind=prior_kind,
                                                mw=mw, stridemw=stridemw, Lw=Lw, ldl=ldl, strideLw=strideLw, Z1=Z1, ldz1=ldz1,
                                                strideZ1=strideZ1, Z2=Z2, ldz2=ldz2, strideZ2=strideZ2, W=W, ldw=ldw, strideW=strideW,
                                                Y=Y, ldy=ldy, strideY=strideY)))
        for b in range(B):
            if Y is not None:
                Y[b, :] = b
            if W is not None:
                W[b, :] = b
        info[:] = 0
        return 0

    def rand(self, dtype, memspace, layout, D, N, S, X, ldx, noise_kind, s, prior_kind, mw, Lw, ldl, Z1, ldz1, Z2, ldz2, Y, ldy):
        self.calls.append(("rand", dict(D=D, N=N, S=S, Z1=Z1.copy(), Z2=Z2.copy())))
        Y[...] = -1
        return 0

    def sample_weights(self, dtype, memspace, D, S, prior_kind, mw, Lw, ldl, Z, ldz, W, ldw):
        self.calls.append(("sample_weights", dict(D=D, S=S, Z=Z.copy())))
        W[...] = -1
        return 0


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(R, "_handle", lambda: r)
    return r


def _fx(rng, D, N, x=None, prior="factor", dt=np.float64, Sy=None):
    mw = rng.standard_normal(D).astype(dt)
    Lw = {"factor": R.PDMat(np.eye(D)), "dense": np.eye(D), "diag": R.Diagonal(np.ones(D))}[prior]
    x = x if x is not None else R.ColVecs(np.asfortranarray(rng.standard_normal((D, N)).astype(dt)))
    return R.BayesianLinearRegressor(mw, Lw)(x, R.Diagonal(np.full(N, 0.5, dtype=dt)) if Sy is None else Sy)


def test_rand_map_draw_order_and_packing(rec):
    rng = np.random.default_rng(0)
    D, N, S, nb = 4, 6, 3, 5
    fxs = [_fx(rng, D, N) for _ in range(nb)]
    out = R.rand_map(np.random.default_rng(7), fxs, S)
    assert [c[0] for c in rec.calls] == ["rand_batched"]
    a = rec.calls[0][1]
    # normals in the reference's order: Z1_b (D x S) then Z2_b (N x S), problem by problem, each filled column-major
    r = np.random.default_rng(7)
    for b in range(nb):
        Z1 = r.standard_normal((S, D)).T
        Z2 = r.standard_normal((S, N)).T
        np.testing.assert_array_equal(a["Z1"][b].reshape((D, S), order="F"), Z1)
        np.testing.assert_array_equal(a["Z2"][b].reshape((N, S), order="F"), Z2)
    assert (a["B"], a["D"], a["N"], a["S"], a["memspace"], a["layout"]) == (nb, D, N, S, _abi.MEM_HOST, _abi.LAYOUT_COLVECS)
    assert (a["ldx"], a["strideX"]) == (D, D * N)
    assert (a["ldz1"], a["strideZ1"], a["ldz2"], a["strideZ2"]) == (D, D * S, N, N * S)
    assert (a["ldy"], a["strideY"], a["W"]) == (N, N * S, None)
    assert (a["stridemw"], a["ldl"], a["strideLw"], a["prior_kind"]) == (D, D, D * D, _abi.PRIOR_UPPER_FACTOR)
    assert (a["noise_kind"], a["strides"]) == (_abi.NOISE_DIAGONAL, N)
    np.testing.assert_array_equal(a["X"][2].reshape((D, N), order="F"), fxs[2].x.X)
    assert len(out) == nb and all(y.shape == (N, S) for y in out)
    assert [float(y[0, 0]) for y in out] == list(range(nb))


def test_rand_map_shares_one_candidate_set(rec):
    rng = np.random.default_rng(1)
    D, N = 3, 16
    X = R.ColVecs(np.asfortranarray(rng.standard_normal((D, N))))
    R.rand_map(np.random.default_rng(0), [_fx(rng, D, N, x=X, Sy=0.1) for _ in range(4)], 1)
    a = rec.calls[0][1]
    assert a["strideX"] == 0 and a["X"].size == D * N
    assert (a["noise_kind"], a["strides"]) == (_abi.NOISE_ISOTROPIC, 1)


def test_rand_map_of_regressors_draws_weights_only(rec):
    rng = np.random.default_rng(2)
    D, S = 5, 4
    fs = [R.BayesianLinearRegressor(rng.standard_normal(D), R.Diagonal(np.ones(D))) for _ in range(3)]
    fs[1] = R.BasisFunctionRegressor(fs[1], lambda x: x)
    out = R.rand_map(np.random.default_rng(3), fs, S)
    assert [c[0] for c in rec.calls] == ["rand_batched"]
    a = rec.calls[0][1]
    assert (a["N"], a["X"], a["Y"], a["Z2"], a["ldw"], a["strideW"]) == (0, None, None, None, D, D * S)
    r = np.random.default_rng(3)
    for b in range(3):
        np.testing.assert_array_equal(a["Z1"][b].reshape((D, S), order="F"), r.standard_normal((S, D)).T)
    assert all(o.shape == (S,) and isinstance(o[0], R.BLRFunctionSample) for o in out)
    assert out[1][0].phi is fs[1].phi and out[0][0].phi is None
    assert np.all(out[2][0].w == 2)


@pytest.mark.parametrize("mix", ["shape", "dtype", "layout", "prior", "dense_noise"])
def test_rand_map_mixed_problems_fall_back_one_by_one(rec, mix):
    rng = np.random.default_rng(4)
    D, N, S = 4, 6, 2
    fxs = [_fx(rng, D, N) for _ in range(3)]
    if mix == "shape":
        fxs[1] = _fx(rng, D, N + 1)
    elif mix == "dtype":
        fxs[1] = _fx(rng, D, N, dt=np.float32)
    elif mix == "layout":
        fxs[1] = _fx(rng, D, N, x=R.RowVecs(np.asfortranarray(rng.standard_normal((N, D)))))
    elif mix == "prior":
        fxs[1] = _fx(rng, D, N, prior="dense")
    else:
        fxs[1] = _fx(rng, D, N, Sy=np.eye(N) * 0.5)
        rec.rand_dense_noise = lambda *a: rec.calls.append(("rand_dense_noise", {})) or 0
    out = R.rand_map(np.random.default_rng(5), fxs, S)
    kinds = [c[0] for c in rec.calls]
    assert "rand_batched" not in kinds and len(kinds) == 3
    # the normals still follow the problem order: the first single call got the first two draws
    r = np.random.default_rng(5)
    np.testing.assert_array_equal(rec.calls[0][1]["Z1"], r.standard_normal((S, D)).T)
    np.testing.assert_array_equal(rec.calls[0][1]["Z2"], r.standard_normal((S, N)).T)
    assert len(out) == 3


def test_rand_map_reports_the_failing_problem(rec):
    rng = np.random.default_rng(6)
    fxs = [_fx(rng, 3, 4, prior="diag") for _ in range(3)]
    fxs[2] = R.BayesianLinearRegressor(np.zeros(3), R.Diagonal(np.array([1.0, -1.0, 1.0])))(fxs[0].x, 0.1)
    with pytest.raises(_abi.PosDefException) as e:
        R.rand_map(np.random.default_rng(0), fxs, 2)
    assert (e.value.index, e.value.info) == (2, 2)
    assert rec.calls == []
    assert R.rand_map(np.random.default_rng(0), [], 2) == []
