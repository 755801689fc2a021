"""Problems, references and lattices of the 16-bit feature routes (blr_posterior_batched_x16: fused_x16_kernel, DESIGN.md K31;
blr_marginals_batched_x16: marg_planes_x16_kernel + marginals_x16_kernel, K32).  A plain module (CPU only), shared by
tests/test_x16_gpu.py, tests/test_x16_marg_gpu.py, tests/test_x16_lattice_gpu.py and tests/test_x16_problems_cpu.py.

Inputs: fixed PCG64 seeds; features are float32 draws rounded to the format, or small integers times a power of two; every element of
X outside the logical matrix (rows between the matrix and ldx, gaps between regressors) is NaN; outputs are pre-filled (NaN / 7)."""
from collections import namedtuple

import numpy as np

import blr_amd as R
from blr_amd import _abi
from oracle import blr_oracle as O

XKINDS = ("col_al", "col_odd", "row_al", "row_odd")
PRIORS = ("diag", "factor", "dense")
NB = 5
EPS32 = float(np.finfo(np.float32).eps)
EXACT_LIMIT = 1 << 24  # integers below it (in magnitude) are fp32 values, and so is every sum of them that stays below it


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------
def x_layout(xkind, D, N):
    """-> (col, aligned, rows, cols, ldx, strideX).  *_al: ldx and strideX multiples of 8 elements (16 bytes); *_odd: both odd."""
    col, aligned = xkind.startswith("col"), xkind.endswith("_al")
    rows, cols = (D, N) if col else (N, D)
    ldx = max(8, -(-rows // 8) * 8) if aligned else (rows + 1) | 1
    strideX = ldx * cols if aligned else (ldx * cols + 2) | 1
    return col, aligned, rows, cols, ldx, strideX


def expected_route(entry, fmt, layout, D, ldx, strideX, base_offset_bytes=0, B=2, options=()):
    """The kernel blr_posterior_batched_x16 (entry "posterior") / blr_marginals_batched_x16 ("marginals") names in blr_last_route:
    the two al16 / fast predicates of csrc/blr_abi.hip.  layout: "col" / "row"; base_offset_bytes: X's distance from a 16-byte
    boundary (0 in host memspace: the staged copy is aligned); options: the handle's flag options that are set."""
    rowv = {"col": False, "row": True}[layout]
    al16 = base_offset_bytes % 16 == 0 and ldx % 8 == 0 and (B == 1 or strideX % 8 == 0)
    fast = al16 and (rowv or D % 8 == 0)
    if entry == "posterior":
        fast = fast and "NO_LDSDMA" not in options
        return f"fused_x16_kernel<{fmt}, {2 * ((D + 31) // 32)}, {(2 if fast else 0) + (1 if rowv else 0)}>"
    if entry == "marginals":  # (NO_LDSDMA does not speak of 16-byte register loads)
        return f"marginals_x16_kernel<{fmt}, {(2 if fast else 0) + (1 if rowv else 0)}>"
    raise ValueError(entry)


def declared_mode(xkind, D):
    """the loader a problem of this layout kind is built for (host memspace, no options)"""
    col, aligned = xkind.startswith("col"), xkind.endswith("_al")
    return (2 if aligned and (not col or D % 8 == 0) else 0) + (0 if col else 1)


def post_stages(N, mode):
    """(nst, nfull) of phase_gram_x16: stages of 32 observations, and how many of them travel by LDS-DMA"""
    return -(-N // 32), (N // 32 if mode >= 2 else 0)


def marg_blocks(D):
    """(nJ, nK): 16-column blocks of the triangle, k-steps of 32 features"""
    return (D + 15) // 16, (D + 31) // 32


def marg_walk(N, nb, cus, image):
    """(groups, most tiles one wave walks) of marginals_x16_kernel: the launch arithmetic of blr_marginals_batched_x16 for a chunk of
    nb regressors on a device with `cus` compute units; four waves per workgroup, wave w of group x starts at tile 4 x + w"""
    ntiles = -(-N // 16)
    if image:
        groups = max(1, min(-(-ntiles // 16), -(-2 * cus // nb)))
    else:
        groups = max(1, min(-(-ntiles // 4), -(-8 * cus // nb)))
    return groups, -(-ntiles // (4 * groups))


def marg_least_walk(N, nb, cus, image):
    """the fewest tiles any wave of the launch walks"""
    groups, _ = marg_walk(N, nb, cus, image)
    return (-(-N // 16)) // (4 * groups)


# ---- problems -------------------------------------------------------------------------------------------------------------------------
def _problem(fmt, xkind, D, N, prior, ints=False, seed=0, nb=NB, scale=1.0):
    """nb regressors with strides of their own.  *_al: ldx and strideX multiples of 8 elements (16 bytes); *_odd: odd ldx and strideX.
    Features are float32 draws rounded to the format (ints: ((7 d + 3 n + b) mod 17 - 8) * scale, scale a power of two); gaps of X
    hold NaN."""
    rng = np.random.Generator(np.random.PCG64(1000 * D + N + seed))
    d, n, b = np.arange(D)[None, :, None], np.arange(N)[None, None, :], np.arange(nb)[:, None, None]
    Xf = (((7 * d + 3 * n + b) % 17 - 8) * scale).astype(np.float32) if ints else rng.standard_normal((nb, D, N)).astype(np.float32)
    X16 = R.bf16_bits(Xf) if fmt == "bf16" else Xf.astype(np.float16)
    Xw = R.widen16(X16, fmt)  # (nb, D, N): the exact float32 values the kernel sees
    col, aligned, rows, cols, ldx, strideX = x_layout(xkind, D, N)
    buf = np.full(max(nb * strideX, 8), 0x7FC0 if fmt == "bf16" else np.nan, dtype=X16.dtype)
    for i in range(nb):
        buf[i * strideX:i * strideX + ldx * cols].reshape((ldx, cols), order="F")[:rows, :] = X16[i] if col else X16[i].T
    if ints:
        y = rng.integers(-4, 5, size=(nb, N)).astype(np.float32)
        mw, s = np.zeros((nb, D), np.float32), np.ones(nb, np.float32)
    else:
        w = rng.standard_normal(D) / np.sqrt(D)
        y = (np.einsum("bdn,d->bn", Xw.astype(float), w) + 0.8 * rng.standard_normal((nb, N))).astype(np.float32)
        mw, s = (0.2 * rng.standard_normal((nb, D))).astype(np.float32), np.exp(0.3 * rng.standard_normal(nb) - 0.5).astype(np.float32)
    if prior == "diag":
        Lw = np.ones((nb, D), np.float32) if ints else np.exp(0.3 * rng.standard_normal((nb, D))).astype(np.float32)
        dense, ldl = list(Lw), 1
    else:
        Lw, dense, ldl = np.zeros((nb, D * D), np.float32), [], D
        for i in range(nb):
            if prior == "factor":  # multiples of 1/8: U'U is exact in fp32 too
                U = np.triu(rng.integers(-1, 2, size=(D, D)) / 8.0, 1) + np.diag(1.0 + rng.integers(0, 5, size=D) / 8.0)
                Lw[i], M = U.reshape(-1, order="F"), (U.T @ U).astype(np.float32)
            else:
                Bm = rng.standard_normal((D, D)) / np.sqrt(D)
                M = (Bm @ Bm.T + np.eye(D)).astype(np.float32)
                M = np.triu(M) + np.triu(M, 1).T
                Lw[i] = M.reshape(-1, order="F")
            dense.append(M)
    kind = {"diag": _abi.PRIOR_DIAGONAL, "dense": _abi.PRIOR_DENSE, "factor": _abi.PRIOR_UPPER_FACTOR}[prior]
    return dict(D=D, N=N, nb=nb, dtype=np.float32, xfmt=_abi.X_BF16 if fmt == "bf16" else _abi.X_F16, fmt=fmt, xkind=xkind, X=buf, Xw=Xw,
                ldx=ldx, strideX=strideX, layout=_abi.LAYOUT_COLVECS if col else _abi.LAYOUT_ROWVECS, y=y, s=s, mw=mw, Lw=Lw, ldl=ldl,
                dense=dense, prior_kind=kind, route=f"fused_x16_kernel<{fmt}, {2 * ((D + 31) // 32)}, {declared_mode(xkind, D)}>")


def _marg_problem(fmt, xkind, D, N, prior, diag_noise, ints=False, nb=NB, scale=1.0, noise_ints=False):
    """_problem (X in every layout with NaN in the gaps, nb regressors with strides of their own) with the noise of the marginals
    entry point.  ints: s = 1, or with noise_ints integers 1 .. 4 (per input under diagonal noise, per regressor otherwise)."""
    q = _problem(fmt, xkind, D, N, prior, ints=ints, nb=nb, scale=scale)
    rng = np.random.Generator(np.random.PCG64(77 * D + N))
    if noise_ints:
        q["s"] = rng.integers(1, 5, size=(nb, N) if diag_noise else nb).astype(np.float32)
    elif diag_noise:
        q["s"] = np.ones((nb, N), np.float32) if ints else np.exp(0.3 * rng.standard_normal((nb, N)) - 0.5).astype(np.float32)
    q.update(noise_kind=_abi.NOISE_DIAGONAL if diag_noise else _abi.NOISE_ISOTROPIC, strides=N if diag_noise else 1,
             route=f"marginals_x16_kernel<{fmt}, {declared_mode(xkind, D)}>")
    return q


def _out(N, nb=NB):
    return dict(mean=np.full((nb, N + 3), np.nan, np.float32), var=np.full((nb, N + 5), np.nan, np.float32), info=np.full(nb, 7, np.int32))


def staged_bytes(*dicts):
    """bytes of every array a host-memspace call on these operands stages"""
    return sum(v.nbytes for d in dicts for v in d.values() if isinstance(v, np.ndarray) and v.ndim <= 2 and v is not d.get("Xw"))


def post_call(hd, q, o, memspace=_abi.MEM_HOST, **over):
    """blr_posterior_batched_x16 on a _problem into the buffers of _small_d_problems._outputs (device memspace: torch tensors)"""
    a = dict(q, noise_kind=_abi.NOISE_ISOTROPIC, strides=1)
    a.update(over)
    p = (lambda x: x.data_ptr()) if memspace == _abi.MEM_DEVICE else (lambda x: x)
    return hd.posterior_batched_x16(a["xfmt"], memspace, a["layout"], a["nb"], a["D"], a["N"], p(a["X"]), a["ldx"], a["strideX"], p(a["y"]), a["N"],
                                    a["noise_kind"], p(a["s"]), a["strides"], a["prior_kind"], p(a["mw"]), a["D"], p(a["Lw"]), a["ldl"],
                                    a["Lw"].shape[1], p(o["mw_post"]), o["stride_mwpost"], p(o["T"]), o["ldt"], o["strideT"], p(o["A"]), o["ldt"],
                                    o["strideT"], p(o["lp"]), p(o["info"]))


def marg_call(hd, q, o, mean=True, var=True, memspace=_abi.MEM_HOST, **over):
    """blr_marginals_batched_x16 on a _marg_problem into the buffers of _out; s / Lw may be None (a mean-only call)"""
    a = dict(q, **over)
    p = (lambda x: None if x is None else x.data_ptr()) if memspace == _abi.MEM_DEVICE else (lambda x: x)
    return hd.marginals_batched_x16(a["xfmt"], memspace, a["layout"], a["nb"], a["D"], a["N"], p(a["X"]), a["ldx"], a["strideX"],
                                    a["noise_kind"], p(a["s"]), a["strides"], a["prior_kind"], p(a["mw"]), a["D"], p(a["Lw"]), a["ldl"],
                                    a["D"] if a["Lw"] is None else a["Lw"].shape[1], p(o["mean"]) if mean else None, o["mean"].shape[1],
                                    p(o["var"]) if var else None, o["var"].shape[1], p(o["info"]))


# ---- the marginals' reference and bound --------------------------------------------------------------------------------------------
def _oracle(q, b, dtype):
    """(mean, var) of regressor b by oracle.blr_oracle in `dtype`, on the exactly widened features and the fp32-rounded mw, Lw, s."""
    D, X = q["D"], np.asfortranarray(q["Xw"][b], dtype=dtype)
    mw, s = q["mw"][b].astype(dtype), (q["s"][b] if q["noise_kind"] == _abi.NOISE_DIAGONAL else q["s"][b:b + 1].repeat(q["N"])).astype(dtype)
    if q["prior_kind"] == _abi.PRIOR_UPPER_FACTOR:
        return O.marginals_direct(mw, q["Lw"][b].reshape((D, D), order="F").astype(dtype), X, s)
    Lw = q["Lw"][b].astype(dtype) if q["prior_kind"] == _abi.PRIOR_DIAGONAL else np.asarray(q["dense"][b], dtype=dtype)
    return O.mean(mw, X), O.var(mw, Lw, X, s)


def _rel(got, ref):
    return float(np.max(np.abs(np.asarray(got, float) - ref)) / np.max(np.abs(ref)))


def oracle_yardsticks(q, b):
    """-> (fp64 reference, fp32 oracle, (yard of mean, yard of var)) of regressor b: the errors of the float32 oracle against the fp64 one"""
    ref, f32 = _oracle(q, b, np.float64), _oracle(q, b, np.float32)
    for k in range(2):
        assert f32[k].dtype == np.float32
    return ref, f32, tuple(_rel(f32[k], ref[k]) for k in range(2))


def _assert_within_oracle(q, o, regs=None):
    """Regressor by regressor: bound = 4 x the relative error (max abs over max abs) the same oracle function makes in float32 on that
    regressor's inputs + 4 eps32 (cases fp32 LAPACK solves all but exactly); the yardstick is the reference's own error, not the
    kernel's, and it is non-zero and finite in every case here (tests/test_x16_problems_cpu.py checks that for the lattice)."""
    N = q["N"]
    for b in (range(q["nb"]) if regs is None else regs):
        ref, f32 = _oracle(q, b, np.float64), _oracle(q, b, np.float32)
        for k, name in enumerate(("mean", "var")):
            assert f32[k].dtype == np.float32
            yard, err = _rel(f32[k], ref[k]), _rel(o[name][b, :N], ref[k])
            print(f"{q['route']} D={q['D']} N={N} regressor {b} {name}: error {err:.3g}, fp32 oracle {yard:.3g}")
            assert 0 < yard < np.inf and err <= 4 * yard + 4 * EPS32, (q["route"], b, name, err, yard)
    assert np.all(np.isnan(o["mean"][:, N:])) and np.all(np.isnan(o["var"][:, N:]))  # nothing written behind the N outputs


# ---- the two lattices ------------------------------------------------------------------------------------------------------------------
PostCase = namedtuple("PostCase", "id fmt xkind D N prior NB mode route")
MargCase = namedtuple("MargCase", "id fmt xkind D N prior diag_noise nJ mode route")
LATTICE_NB = 3          # regressors of a posterior lattice case
MARG_LATTICE_NB = 5     # ... of a marginals lattice case (N = 293: 19 tiles, two workgroups per regressor on the image path)
POST_DS = {2: (1, 17, 24, 32), 4: (33, 56, 64), 6: (65, 88, 96), 8: (97, 100, 104, 120, 127, 128)}
POST_NS = (0, 1, 31, 32, 33, 96, 97, 128, 160, 161, 293, 320)
POST_RING_NS = (160, 293, 161, 320)   # neighbours alternate between one ring revolution ({160, 161}) and two ({293, 320})
POST_SEAM_NS = (0, 1, 31, 32, 33, 96, 97, 128)
MARG_DS = (8, 24, 33, 64, 88, 97, 104, 113, 120, 127)
MARG_NS = (15, 16, 17, 128, 293)


def _post_lattice():
    """Every (fmt, D, layout kind) cell once with a ring N: the cells of one (fmt, NB, MODE) take POST_RING_NS in turn, from a start
    that differs between the groups; five cells of every eight of a MODE also take the next seam N of that MODE."""
    rows, in_group, in_mode, seams = [], {}, {}, {}
    for f, fmt in enumerate(("bf16", "f16")):
        for nb16, Ds in POST_DS.items():
            for i, D in enumerate(Ds):
                for k, xkind in enumerate(XKINDS):
                    mode = declared_mode(xkind, D)
                    j = in_group.get((fmt, nb16, mode), 0)
                    in_group[fmt, nb16, mode] = j + 1
                    Ns = [POST_RING_NS[(j + nb16 // 2 + f) % 4]]
                    c = in_mode.get(mode, 0)
                    in_mode[mode] = c + 1
                    if c % 8 < 5:
                        Ns.append(POST_SEAM_NS[seams.get(mode, 0) % 8])
                        seams[mode] = seams.get(mode, 0) + 1
                    for N in Ns:
                        prior = PRIORS[(i + k + f + POST_NS.index(N)) % 3]
                        rows.append(PostCase(f"{fmt}-{xkind}-D{D}-N{N}-{prior}", fmt, xkind, D, N, prior, nb16, mode,
                                             f"fused_x16_kernel<{fmt}, {nb16}, {mode}>"))
    return tuple(rows)


def _marg_lattice():
    """Every (fmt, D, layout kind) cell at one N, every second cell at a second one; the (prior, noise) pair runs with the cell and
    the N.  Then N = 293 with a factor and a dense prior in every (fmt, MODE)."""
    rows, c = [], 0
    for f, fmt in enumerate(("bf16", "f16")):
        for D in MARG_DS:
            for k, xkind in enumerate(XKINDS):
                Ns = [MARG_NS[c % 5]] + ([MARG_NS[(c + 2) % 5]] if c % 2 == 0 else [])
                for which, N in enumerate(Ns):
                    pair = (k + 4 * f + 3 * which) % 6  # (all six over the eight cells of a D)
                    rows.append((fmt, xkind, D, N, PRIORS[pair % 3], pair >= 3))
                c += 1
        for k, xkind in enumerate(XKINDS):
            for prior, D in (("factor", 120 if k % 2 == 0 else 127), ("dense", 104 if k % 2 == 0 else 113)):
                rows.append((fmt, xkind, D, 293, prior, (k + f) % 2 == 1))
    rows = list(dict.fromkeys(rows))
    return tuple(MargCase(f"{fmt}-{xkind}-D{D}-N{N}-{prior}-{'diagnoise' if dn else 'iso'}", fmt, xkind, D, N, prior, dn, marg_blocks(D)[0],
                          declared_mode(xkind, D), f"marginals_x16_kernel<{fmt}, {declared_mode(xkind, D)}>")
                 for fmt, xkind, D, N, prior, dn in rows)


POST_LATTICE = _post_lattice()
MARG_LATTICE = _marg_lattice()


def post_lattice_problem(case):
    return _problem(case.fmt, case.xkind, case.D, case.N, case.prior, nb=LATTICE_NB)


def marg_lattice_problem(case):
    return _marg_problem(case.fmt, case.xkind, case.D, case.N, case.prior, case.diag_noise, nb=MARG_LATTICE_NB)


# ---- exact cases: small integers times a power of two, references in int64 ------------------------------------------------------------------
EXACT_NB = 3
GRAM_EXACT_DS, GRAM_EXACT_NS = (64, 100, 120, 127, 128), (128, 160, 293, 320)
MARG_EXACT_DS, MARG_EXACT_NS = (97, 113, 127), (128, 293)
SUBNORMAL = 2.0 ** -24  # the smallest fp16 subnormal: k SUBNORMAL, |k| <= 8, are fp16 subnormals (and bf16 / fp32 normals)
PURE_DS, PURE_N = (5, 24), 131


def features_as_integers(q, scale=1.0):
    """(nb, D, N) int64: the widened features over `scale`; asserts that the format held every scaled value exactly"""
    K = np.rint(q["Xw"].astype(np.float64) / scale)
    assert np.array_equal(K * scale, q["Xw"].astype(np.float64)) and np.max(np.abs(K), initial=0) <= 8
    return K.astype(np.int64)


def gram_exact_problem(fmt, xkind, D, N, scale=1.0, nb=EXACT_NB):
    """Integer features in [-8, 8] times `scale`, diagonal prior scale^2, unit noise, zero prior mean: Lw' = scale^2 (I + K K').
    -> (q, K K' + I per regressor in int64, the largest sum of |terms| of any entry)"""
    q = _problem(fmt, xkind, D, N, "diag", ints=True, nb=nb, scale=scale)
    q["Lw"] = np.full((nb, D), scale * scale, np.float32)
    q["dense"] = list(q["Lw"])
    K = features_as_integers(q, scale)
    ref = np.stack([np.eye(D, dtype=np.int64) + K[b] @ K[b].T for b in range(nb)])
    return q, ref, int(max(np.max(np.abs(K[b]) @ np.abs(K[b]).T) for b in range(nb))) + 1


def marg_exact_problem(fmt, xkind, D, N, diag_noise, scale=1.0, nb=EXACT_NB):
    """The construction of test_x16_marginals_exact_on_integers: features K scale, U = scale (I + N0) with N0 in rows < D / 2 and columns
    >= D / 2 (three entries of +-1 per column), so U^-1 = (I - N0) / scale exactly and z = (I - N0)'K; mw = integers in [-3, 3] over
    scale; integer noise 1 .. 4.  -> (q, mean, var as float32 (nb, N), the largest sum of |terms| behind any of z, mean, var)"""
    q = _marg_problem(fmt, xkind, D, N, "factor", diag_noise, ints=True, nb=nb, scale=scale, noise_ints=True)
    rng = np.random.Generator(np.random.PCG64(31 * D + N))
    K = features_as_integers(q, scale)
    N0 = np.zeros((nb, D, D), np.int64)
    for b in range(nb):
        for c in range(D // 2, D):
            N0[b, rng.choice(D // 2, size=3, replace=False), c] = rng.choice([-1, 1], size=3)
    mwi = rng.integers(-3, 4, size=(nb, D))
    q["Lw"] = np.stack([((np.eye(D, dtype=np.int64) + N0[b]) * scale).astype(np.float32).reshape(-1, order="F") for b in range(nb)])
    q["mw"] = (mwi / scale).astype(np.float32)
    assert np.array_equal(q["mw"].astype(np.float64) * scale, mwi)
    eye = np.eye(D, dtype=np.int64)
    z = np.stack([(eye - N0[b]).T @ K[b] for b in range(nb)])
    si = q["s"].astype(np.int64) if diag_noise else q["s"].astype(np.int64)[:, None]
    mean, var = np.einsum("bdn,bd->bn", K, mwi), np.sum(z * z, axis=1) + si
    big = max(int(np.max(np.einsum("bdn,bd->bn", np.abs(K), np.abs(mwi)))), int(np.max(var)),
              max(int(np.max(np.abs(eye - N0[b]).T @ np.abs(K[b]))) for b in range(nb)))
    return q, mean.astype(np.float32), var.astype(np.float32), big


def pure_stream_problem(fmt, xkind, D, B, N=PURE_N):
    """B regressors on ONE shared X (strideX = 0) of integers: mw integers in [-3, 3], a diagonal prior of 1, 2, 4, diagonal noise of
    integers 1 .. 4.  mean = K'mw; var = sum K_d^2 / Lw_d + s_n: a multiple of 1/4 below 2^24 / 4, whatever the order of the sum.
    -> (q, mean, var as float32 (B, N), the largest sum of |terms| in units of 1/4)"""
    q = _marg_problem(fmt, xkind, D, N, "diag", True, ints=True, nb=1)
    rng = np.random.Generator(np.random.PCG64(5 * D + B))
    K = features_as_integers(q)[0]
    mwi, Lwi, si = rng.integers(-3, 4, size=(B, D)), 2 ** rng.integers(0, 3, size=(B, D)), rng.integers(1, 5, size=(B, N))
    q.update(nb=B, strideX=0, mw=mwi.astype(np.float32), Lw=Lwi.astype(np.float32), s=si.astype(np.float32))
    quarters = (4 // Lwi) @ (K * K) + 4 * si
    big = max(int(np.max(np.abs(mwi) @ np.abs(K))), int(np.max(quarters)))
    return q, (mwi @ K).astype(np.float32), (quarters / 4.0).astype(np.float32), big
