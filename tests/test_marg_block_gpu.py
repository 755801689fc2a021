"""marg_blocksub_kernel<T, RT> (csrc/blr_marginals.hpp; launched by marginals_large_group, csrc/blr_abi.hip) over block counts, tile
walks and batch grids.  The kernel issues its 16-byte loads from inline asm and keeps its s_waitcnt counts by hand, prefetches the
inputs two blocks ahead -- across the end of a tile into the workgroup's next one -- and renumbers the workgroups of a batch per XCD.
Which of that a call runs is decided by the launch rule, so every test first asserts blr_get_stat "marg_block_rt" / "marg_block_walk"
/ "marg_block_renumbered" against the rule as tests/_marg_block_problems.py restates it: a case that runs elsewhere fails.

A batch of B = cus regressors has grid 1 x cus: one workgroup walks all tiles of a regressor, renumbered when 8 | cus; B = cus + 1
walks alike without renumbering.  "Shared" cases pass X and the factor with stride 0 and give each regressor its own prior mean and
noise, so one fp64 triangular solve is the reference of the whole batch.

References: tests/_seam_problems.marginals_ref in fp64 on operands already rounded to the element type.  Tolerances: those of
test_large_d_marginals and of TOL["marginals"] in tests/test_chunk_seams_gpu.py (fp64 1e-10, fp32 3e-4; mean rtol = rt, atol = 10 rt;
var rtol = rt), with the priors built as those tests build them."""
import numpy as np
import pytest

import _marg_block_problems as MB

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DTYPES = [F32, F64]
ids_dt = lambda d: np.dtype(d).name  # noqa: E731


@pytest.fixture(scope="module")
def handle():
    from blr_amd import _abi
    h = _abi.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def stats(h):
    return h.get_stat("marg_block_rt"), h.get_stat("marg_block_walk"), h.get_stat("marg_block_renumbered")


def assert_route(h, dt, D, N, B, cus, prior="factor"):
    """the three stats of the call just made against the rule -> them"""
    want, got = MB.expected_block_route(dt, D, N, B, cus, prior=prior), stats(h)
    print(f"route {np.dtype(dt).name} D={D} N={N} B={B} cus={cus} {prior}: (rt, walk, renumbered) = {got}, the rule says {want}")
    assert all(w is None or w == g for w, g in zip(want, got)), (got, want)
    return got


def check(dt, mean, var, mean_o, var_o, what=""):
    rt = MB.TOL[np.dtype(dt).name]
    if mean is not None:
        print(what, "mean: max abs err", np.abs(mean - mean_o).max())
        np.testing.assert_allclose(mean, mean_o, rtol=rt, atol=10 * rt, err_msg=f"{what} mean")
    print(what, "var: max rel err", (np.abs(var - var_o) / var_o).max())
    np.testing.assert_allclose(var, var_o, rtol=rt, err_msg=f"{what} var")


def run_shared(h, dt, p, B=None, regs=None):
    """blr_marginals_batched_* on a shared problem (X and the factor at stride 0; diagonal noise), host memspace: the whole batch, or
    the regressors `regs` one call each (B = 1) -> mean, var [B | len(regs), N] as fp64"""
    from blr_amd import _abi
    D, N = p["D"], p["N"]
    X, U = p["X"].astype(dt), p["Ucm"].astype(dt)
    if regs is None:
        mw, s = p["mw"][:B].astype(dt), p["s"][:B].astype(dt)
        mean, var = np.full((B, N), np.nan, dtype=dt), np.full((B, N), np.nan, dtype=dt)
        info = np.full(B, 99, dtype=np.int32)
        h.marginals_batched(dt, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, B, D, N, X, D, 0, _abi.NOISE_DIAGONAL, s, N, _abi.PRIOR_UPPER_FACTOR, mw, D, U, D, 0,
                            mean, N, var, N, info)
        assert not info.any(), info
        return mean.astype(F64), var.astype(F64)
    out = []
    for b in regs:
        m, v = run_shared(h, dt, {**p, "mw": p["mw"][b:b + 1], "s": p["s"][b:b + 1]}, B=1)
        out.append((m[0], v[0]))
    return np.stack([m for m, _ in out]), np.stack([v for _, v in out])


# ---- (a) blocks x types: every NC the tile allows, last blocks of 1, 7 and 8 column tiles; N = 72 is tiles of 32, 32 and 8 rows ------
A_WIDTHS = [(F32, D) for D in (144, 240, 256, 272, 400, 640, 1040, 1136, 1152)] + [(F64, D) for D in (144, 240, 256, 272, 384, 496, 512)]


@pytest.mark.parametrize("dt,D", A_WIDTHS, ids=[f"{ids_dt(d)}-{D}" for d, D in A_WIDTHS])
def test_blocks_and_types(handle, cus, dt, D):
    N = 72
    p = MB.shared_problem(dt, D, N, cus)
    mean, var = run_shared(handle, dt, p, B=cus)
    got = assert_route(handle, dt, D, N, cus, cus)
    assert got == (32, 3, int(cus % 8 == 0)), got   # one workgroup per regressor walks the three tiles
    check(dt, mean, var, p["mean"], p["lat"][None] + p["s"], f"B = {cus}")
    mean, var = run_shared(handle, dt, p, B=1)
    got = assert_route(handle, dt, D, N, 1, cus)
    assert got == ((16 if dt == F32 else 32), 1, 0), got
    check(dt, mean, var, p["mean"][:1], p["lat"][None] + p["s"][:1], "B = 1")


# ---- (b) walk lengths at NC = 2 and 3: last tiles of 32 rows and of 1 row, with and without renumbering ---------------------------
@pytest.mark.parametrize("N,walk", [(32, 1), (33, 2), (64, 2), (65, 3), (97, 4)])
@pytest.mark.parametrize("D", [144, 256, 272])
@pytest.mark.parametrize("dt", DTYPES, ids=ids_dt)
def test_walk_lengths(handle, cus, dt, D, N, walk):
    p = MB.shared_problem(dt, D, N, cus + 1)
    for B in (cus, cus + 1):
        mean, var = run_shared(handle, dt, p, B=B)
        got = assert_route(handle, dt, D, N, B, cus)
        assert got[:2] == (32, walk), got
        check(dt, mean, var, p["mean"][:B], p["lat"][None] + p["s"][:B], f"B = {B}")  # every regressor of the batch


# ---- (c) distinct regressors under renumbering: a wrong regressor index reads another's factor or writes another's outputs ---------
def run_distinct(h, dt, p, prior, noise="diag", with_mean=True, bad_value=None):
    """Every operand per regressor, ldx and ldl one 16-byte vector beyond D, outputs N + 5 apart in buffers of -7; regressors
    {0, 7, 8, B - 1} get a factor (precision) that is none.  -> (mean | None, var) payloads [B, N] fp64, info, bad, gaps kept"""
    from blr_amd import _abi
    D, N, B = p["D"], p["N"], p["B"]
    ld = D + 16 // np.dtype(dt).itemsize
    bad = sorted({0, 7, 8, B - 1})
    Lw = p["Lw"].copy()
    Lw[bad, 2, 2] = bad_value
    X, Lw = MB.pad_ld(p["X"], ld).astype(dt), MB.pad_ld(Lw, ld).astype(dt)
    mw = p["mw"].astype(dt)
    if noise == "diag":
        s, nk, ss = p["s"].astype(dt), _abi.NOISE_DIAGONAL, N
    elif noise == "iso":
        s, nk, ss = p["s1"].astype(dt), _abi.NOISE_ISOTROPIC, 1
    else:  # one scalar for the whole batch
        s, nk, ss = p["s1"][:1].astype(dt), _abi.NOISE_ISOTROPIC, 0
    so = N + 5
    mean = np.full(B * so, MB.FILL, dtype=dt) if with_mean else None
    var = np.full(B * so, MB.FILL, dtype=dt)
    info = np.full(B, 99, dtype=np.int32)
    pk = _abi.PRIOR_UPPER_FACTOR if prior == "factor" else _abi.PRIOR_DENSE
    h.marginals_batched(dt, _abi.MEM_HOST, _abi.LAYOUT_COLVECS, B, D, N, X, ld, N * ld, nk, s, ss, pk, mw, D, Lw, ld, D * ld, mean, so, var, so, info)
    pay = lambda a: None if a is None else a.reshape(B, so)[:, :N].astype(F64)  # noqa: E731
    gaps = all(a is None or bool((a.reshape(B, so)[:, N:] == MB.FILL).all()) for a in (mean, var))
    return pay(mean), pay(var), info, bad, gaps


def check_distinct(dt, p, noise, mean, var, info, bad, gaps):
    B = p["B"]
    good = [b for b in range(B) if b not in bad]
    print("info of the broken regressors", info[bad].tolist(), "others non-zero:", np.flatnonzero(info[good]).tolist())
    assert (info[bad] == 3).all() and not info[good].any(), info
    assert gaps, "an output gap was overwritten"
    for a in (mean, var):
        assert a is None or (a[bad] == MB.FILL).all(), "a broken regressor's outputs were written"
    noise_o = {"diag": p["s"], "iso": p["s1"][:, None], "iso0": p["s1"][:1, None]}[noise]
    var_o = p["lat"] + noise_o
    check(dt, None if mean is None else mean[good], var[good], p["mean"][good], var_o[good], f"B = {B}, {noise}")


@pytest.mark.parametrize("noise,with_mean", [("diag", True), ("iso", True), ("iso0", True), ("diag", False)],
                         ids=["diag_noise", "iso_per_regressor", "iso_shared", "mean_null"])
@pytest.mark.parametrize("extra", [0, 1], ids=["B=cus", "B=cus+1"])
@pytest.mark.parametrize("dt", DTYPES, ids=ids_dt)
def test_distinct_regressors_factor(handle, cus, dt, extra, noise, with_mean):
    D, N, B = 144, 70, cus + extra
    p = MB.distinct_problem(dt, D, N, B, "factor")
    mean, var, info, bad, gaps = run_distinct(handle, dt, p, "factor", noise, with_mean, bad_value=-1.0)
    got = assert_route(handle, dt, D, N, B, cus)
    assert got == (32, 3, int(B % 8 == 0)), got
    check_distinct(dt, p, noise, mean, var, info, bad, gaps)


@pytest.mark.parametrize("extra", [0, 1], ids=["B=cus", "B=cus+1"])
@pytest.mark.parametrize("dt", DTYPES, ids=ids_dt)
def test_distinct_regressors_dense(handle, cus, dt, extra):
    """the factor the kernel sees has order DP = 384, the inputs 272 features (Dx < D); the batch goes in chol_large's groups, so the
    walk and the renumbering are read from the stat, not predicted"""
    D, N, B = 272, 70, cus + extra
    p = MB.distinct_problem(dt, D, N, B, "dense")
    mean, var, info, bad, gaps = run_distinct(handle, dt, p, "dense", bad_value=-50.0)
    got = assert_route(handle, dt, D, N, B, cus, prior="dense")
    assert got[0] == 32 and 1 <= got[1] <= 3 and got[2] in (0, 1), got
    check_distinct(dt, p, "diag", mean, var, info, bad, gaps)


# ---- (d) fp64: the walk has the bits of the single trip -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [144, 512])
def test_fp64_walk_has_the_bits_of_the_single_trip(handle, cus, D):
    """both runs use marg_blocksub_kernel<double, 32>, and a tile's arithmetic does not depend on which workgroup runs it"""
    N = 72
    p = MB.shared_problem(F64, D, N, cus)
    mean, var = run_shared(handle, F64, p, B=cus)
    assert assert_route(handle, F64, D, N, cus, cus)[:2] == (32, 3)
    regs = sorted({0, 9 % cus, cus - 1})
    mean1, var1 = run_shared(handle, F64, p, regs=regs)
    assert assert_route(handle, F64, D, N, 1, cus) == (32, 1, 0)
    for k, b in enumerate(regs):
        print("regressor", b, "walk vs alone: max abs diff", np.abs(mean[b] - mean1[k]).max(), np.abs(var[b] - var1[k]).max())
        assert np.array_equal(mean[b], mean1[k]) and np.array_equal(var[b], var1[k]), b


# ---- (e) the edge of the route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,block", [(F32, 1152, True), (F32, 1168, False), (F64, 512, True), (F64, 528, False), (F64, 576, False)],
                         ids=["float32-1152", "float32-1168", "float64-512", "float64-528", "float64-576"])
def test_edge_of_the_route(handle, cus, dt, D, block):
    """16 | D on both sides of the largest tile: beyond it the call reports marg_block_rt = 0 and still matches through the tall
    sweep (fp64: 640 columns take 172 032 bytes of LDS, so D = 576 is beyond)"""
    N = 72
    p = MB.shared_problem(dt, D, N, 1)
    mean, var = run_shared(handle, dt, p, B=1)
    got = assert_route(handle, dt, D, N, 1, cus)
    assert (got[0] != 0) == block and (block or got == (0, 0, 0)), got
    check(dt, mean, var, p["mean"], p["lat"][None] + p["s"], "B = 1")
