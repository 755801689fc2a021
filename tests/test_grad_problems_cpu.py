"""tests/_grad_problems.py without a GPU: its longdouble truth against the oracle and against finite differences of the evidence,
the conditioning of every lattice problem, the coverage the lattice promises, and the host restatement of the route gate and the
launch grid for every case of tests/test_grad_lattice_gpu.py -- a change of the launch heuristics must fail HERE instead of
silently moving a GPU case off the walk it was written for.  The CU count enters the product route's grid only; the handle does not
expose it, so the restatement uses 256 (an MI355X) and is repeated for a partitioned part's smaller counts."""
import numpy as np
import pytest

import _grad_problems as GP
from oracle import blr_oracle as O

F64, F32, LD = GP.F64, GP.F32, GP.LD


def _oracle(p, b):
    """O.logpdf_grad on regressor b (fp64) -> the outputs in _grad_problems' names and index order"""
    P = p["P"][b]
    Lw = P if p["prior"] != "factor" else P.T @ P
    s = p["s"][b] if p["noise"] == "diag" else float(p["s"][b, 0])
    lp, g = O.logpdf_grad(p["mw"][b], Lw, np.ascontiguousarray(p["X"][b].T), s, p["y"][b])
    return {"logpdf": np.array(lp), "dX": g["X"].T, "dy": g["y"], "ds": g["s"], "dmw": g["mw"], "mw_post": g["mw_post"], "Ainv": g["Ainv"]}


HANDFUL = [(3, 17, 65, "dense", "diag"), (3, 128, 80, "factor", "iso"), (3, 33, 130, "diag", "diag"), (2, 1, 1, "diag", "iso"),
           (3, 100, 64, "dense", "iso")]


@pytest.mark.parametrize("B,D,N,prior,noise", HANDFUL, ids=[f"D{h[1]}-N{h[2]}-{h[3]}-{h[4]}" for h in HANDFUL])
def test_truth_agrees_with_the_oracle(B, D, N, prior, noise):
    # The oracle runs in fp64 on problems whose cond(A) is below 6 (the lattice's worst): a few eps of the largest entry of each
    # output.  Measured worst over these five problems and all outputs: 5.9e-16 -- the bound is 4 x that, 2.5e-15.
    p = GP.problem(F64, B, D, N, prior, noise)
    t = GP.truth(p)
    assert all(v.dtype == LD for v in t.values())
    worst = 0.0
    for b in range(B):
        o = _oracle(p, b)
        for k in GP.OUTPUTS:
            e = float(GP.errors(k, o[k][None], t[k][b][None])[0])
            worst = max(worst, e)
            assert e <= 2.5e-15, (k, b, e)
    print("worst error of the fp64 oracle against the longdouble truth:", worst)


def test_fp32_truth_is_the_fp64_closed_form_on_rounded_inputs():
    p = GP.problem(F32, 3, 17, 65, "factor", "diag")
    for k in ("X", "y", "s", "mw", "P"):
        assert np.array_equal(p[k], p[k].astype(F32).astype(F64)), k
    t, yd = GP.truth(p), GP.yardstick(p)
    assert all(v.dtype == F64 for v in t.values()) and all(v.dtype == F32 for v in yd.values())
    for b in range(3):
        o = _oracle(p, b)
        for k in GP.OUTPUTS:
            assert float(GP.errors(k, o[k][None], t[k][b][None])[0]) <= 2.5e-15, (k, b)
            assert float(GP.errors(k, yd[k][b][None], t[k][b][None])[0]) <= 1e-4, (k, b)  # (the yardstick is the same quantity)


def test_truth_agrees_with_finite_differences_of_the_evidence():
    # D = 3, N = 5, central differences of the LONGDOUBLE evidence with h = 2^-20: truncation h^2 f'''/6 ~ 1e-12 x O(1..100), rounding
    # eps_ld |f| / h ~ 1e-12 -- bound 1e-9 of the largest entry of each gradient (three orders above both, six below a wrong formula).
    h = LD(2.0) ** -20
    for prior, noise in (("dense", "diag"), ("factor", "iso")):
        p = GP.problem(F64, 2, 3, 5, prior, noise)
        t = GP.truth(p)
        ev = lambda q: GP.closed_form(q, LD, GP._LoopLin, only_logpdf=True)["logpdf"]  # noqa: E731

        def fd(key, index):
            qp, qm = dict(p), dict(p)
            for q, sign in ((qp, 1), (qm, -1)):
                a = p[key].astype(LD)
                a[(slice(None),) + index] += sign * h
                q[key] = a
            return (ev(qp) - ev(qm)) / (2 * h)

        g = {"dX": np.zeros((2, 5, 3), dtype=LD), "dy": np.zeros((2, 5), dtype=LD), "dmw": np.zeros((2, 3), dtype=LD)}
        for n in range(5):
            g["dy"][:, n] = fd("y", (n,))
            for d in range(3):
                g["dX"][:, n, d] = fd("X", (n, d))
        for d in range(3):
            g["dmw"][:, d] = fd("mw", (d,))
        if noise == "diag":
            g["ds"] = np.zeros((2, 5), dtype=LD)
            for n in range(5):
                g["ds"][:, n] = fd("s", (n,))
            ds_truth = t["ds"]
        else:  # isotropic: the gradient in the one variance is the sum of the per-observation entries (include/blr_mi355x.h)
            g["ds"] = fd("s", (0,))[:, None]
            ds_truth = t["ds"].sum(axis=1, keepdims=True)
        for k, ref in (("dX", t["dX"]), ("dy", t["dy"]), ("dmw", t["dmw"]), ("ds", ds_truth)):
            e = GP.errors(k, g[k], ref)
            print(prior, noise, k, "finite differences against the closed form:", e)
            assert (e <= 1e-9).all(), (prior, noise, k, e)


def test_every_lattice_problem_is_well_conditioned():
    seen = set()
    for c in GP.ALL_CASES:
        p = GP.case_problem(c)
        seen.add(GP._key(p))
        assert p["cond"].shape == (c["B"],) and (p["cond"] <= GP.COND_MAX).all(), (c["id"], p["cond"].max())
    print(len(seen), "problems, worst cond(A):", max(GP.problem(*k)["cond"].max() for k in seen))


def test_the_sweep_lattice_covers_what_it_promises():
    cases = GP.SWEEP_BLOCKS
    assert len({c["id"] for c in GP.ALL_CASES}) == len(GP.ALL_CASES)
    for dt, lay in GP.DTL:
        mine = [c for c in cases if c["dt"] == dt and c["layout"] == lay]
        assert sorted(c["D"] for c in mine) == sorted(GP.SWEEP_DS)
    for axis, values in (("N", GP.SWEEP_NS), ("noise", GP.NOISES), ("prior", GP.PRIORS)):
        for dt in (F64, F32):
            assert {c[axis] for c in cases if c["dt"] == dt} == set(values), (axis, dt)
        for lay in ("col", "row"):
            assert {c[axis] for c in cases if c["layout"] == lay} == set(values), (axis, lay)
    assert all(c["B"] == 3 and c["ainv"] and c["xpad"] and c["dxpad"] and c["xstride_pad"] for c in cases)
    prod = [c for c in GP.PRODUCTS if c["B"] == 3 and c["N"] <= 130]
    for dt, lay in GP.DTL:
        assert {c["N"] for c in prod if c["dt"] == dt and c["layout"] == lay} == {64, 65, 79, 80, 130}
        assert {c["noise"] for c in prod if c["dt"] == dt} == set(GP.NOISES)


@pytest.mark.parametrize("c", GP.ALL_CASES, ids=[c["id"] for c in GP.ALL_CASES])
def test_every_case_lands_on_the_walk_it_claims(c):
    route, walk = c["claim"]
    assert GP.takes_products(c) == (route == "product"), c["id"]
    if route == "product":
        assert c["D"] == 128 and c["N"] >= 64
        if walk is not None:
            assert GP.product_walk(c) == walk
        if c["B"] >= GP.CUS:
            for cus in (256, 128, 64, 32):  # (a partitioned part reports its share)
                assert GP.per_reg(c, cus) == 1 and len(GP.product_walk(c, cus)) == 1
        return
    if walk is not None:
        assert GP.sweep_walk(c) == walk and GP.per_reg(c) == len(walk)
    else:
        assert GP.per_reg(c) == len(GP.sweep_walk(c)) and all(len(w) == 1 for w in GP.sweep_walk(c))  # B = 3: a workgroup per tile
    if route.startswith("sweep-vec"):  # every regressor on the vector loads with prefetch; dX by vector or by scalar stores
        assert GP.sweep_vec_paths(c) == (True, route == "sweep-vec"), c["id"]


def test_the_walk_cases_are_the_walks_of_the_issue():
    by = {tuple(c["claim"][1]): c for c in GP.SWEEP_WALKS if c["dt"] == F64}
    assert set(by) == {("rr", "rp"), ("rrrp",), ("rrp", "rp")}
    assert GP.per_reg(by[("rr", "rp")]) == 2 and GP.per_reg(by[("rrrp",)]) == 1       # two real tiles; real then pseudo; one walks all
    vecs = [c for c in GP.SWEEP_WALKS if c["D"] == 128]
    assert all(c["no_gemm"] and c["N"] == 130 and c["layout"] == "col" for c in vecs)  # workgroup 0: tiles 0, 2, 4 -- prefetches 0 + 2
    assert sorted(GP.sweep_vec_paths(c) for c in vecs if c["dt"] == F32) == [(True, False), (True, True)]


def test_floors_and_input_padding():
    assert max(GP.FLOOR.values()) <= GP.FLOOR_MAX and set(GP.FLOOR) == {(k, d) for k in GP.OUTPUTS for d in ("f64", "f32")}
    for c in GP.ALL_CASES:  # every batched input other than X sits at strides above the tight ones, NaN in the gaps
        st, D, N = GP.in_strides(c), c["D"], c["N"]
        assert st["y"] > N and st["mw"] > D and st["s"] > (N if c["noise"] == "diag" else 1)
        assert (st["ldl"] == 1 and st["Lw"] > D) if c["prior"] == "diag" else (st["ldl"] > D and st["Lw"] > st["ldl"] * D)
    for prior in GP.PRIORS:
        c = GP.case(F32, "col", 3, 5, 7, prior, "iso")
        ins, _ = GP.pack(c)
        st = GP.in_strides(c)
        assert ins["y"].size == 3 * st["y"] and np.isnan(ins["y"]).sum() == 3 * 3 and np.isnan(ins["s"]).sum() == 3 * 3
        assert np.isnan(ins["Lw"]).sum() == (3 * 3 if prior == "diag" else 3 * (3 * 5 + 5)) and np.isnan(ins["mw"]).sum() == 9
        p = GP.case_problem(c)
        first = ins["Lw"][st["Lw"]:st["Lw"] + 5]  # regressor 1: the diagonal, or column 0 of the matrix
        want = p["P"][1] if prior == "diag" else (p["P"][1][:, 0] if prior == "dense" else p["P"][1][0, 0] * np.eye(5)[0])
        assert np.array_equal(first, want.astype(F32))


def test_the_gate_cases_break_one_condition_each():
    for dt in (F64, F32):
        size = np.dtype(dt).itemsize
        g = [c for c, _ in GP.GATES if c["dt"] == dt]
        same = [s for c, s in GP.GATES if c["dt"] == dt]
        assert same == [True] * 4 + [False] * 2
        ok = lambda c: (c["N"] >= 64, c["ldx"] % GP.VEC[dt] == 0, (c["strideX"] * size) % 16 == 0, c["base_off"] == 0)  # noqa: E731
        assert [ok(c) for c in g[:5]] == [(False, True, True, True), (True, False, True, True), (True, True, False, True),
                                          (True, True, True, False), (True, True, True, True)]
        assert g[1]["ldx"] == (129 if dt == F64 else 130)
        assert g[5]["layout"] == "row" and g[5]["ldx"] % 2 == 1
        assert [GP.takes_products(c) for c in g] == [False] * 4 + [True] * 2
        assert not any(GP.takes_products(dict(c, no_gemm=True)) for c in g)
