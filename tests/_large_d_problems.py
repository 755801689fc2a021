"""Problems of the large-D update (D > 128, posterior_large_group) for the GPU tests: the table of (route, shape, loader, noise, prior,
prior mean, group) rows that reaches every Gram route of plan_large off the clean shape, the rule that says which route a call
takes -- a Python restatement of csrc/blr_large_plan.hpp, it never calls the library --, device images of X whose alignment, padding
rows and slack columns are what the row says (NaN wherever nothing may read), and the oracle checks.  A plain module, not a conftest;
importing it needs no GPU.  The batch itself (data, noise, priors, oracle inputs) is _small_d_problems._batch's."""
import numpy as np

from _small_d_problems import _batch, _oracle_inputs, _outputs, _result, _same_bits, _written  # noqa: F401  (re-exported to the tests)
from _yardsticks import _assert_fp32_within_lapack
from blr_amd import _abi
from oracle import blr_oracle as O

ROUTES = ("gram_tile_kernel<double>", "gram_planes4_kernel", "gram_planes_kernel<2>", "gram_planes_kernel<3>",
          "gram_tile_kernel<float, true>", "gram_tile_kernel<float>")
PLANES_ROUTES = {"gram_planes4_kernel": 2, "gram_planes_kernel<2>": 2, "gram_planes_kernel<3>": 3}  # route -> planes per operand (NP)
TILE_ROUTES_F32 = ("gram_tile_kernel<float, true>", "gram_tile_kernel<float>")
KPB = 128            # blr_marg_image.hpp kPB: edge of a macro tile / row block
PLANES_CHUNK_KB = 64  # blr_planes.hpp kPlanesChunkKb
PLANES_KBS = {2: 2, 3: 1}  # blr_planes.hpp PlanesCfg<NP>::KBS: k-blocks of 16 columns per stage of the Gram launch

# Handles of the lattice: per-handle options only (Handle.set_option), the default handle and the environment stay untouched.
# NO_LDSDMA is not consulted at D > 128 (blr_abi.hip reads it for the fused kernels only): its rows pin that the route and the
# result are those of the handle without it.
OPTION_SETS = {
    "default": {},
    "nospec": {"NO_SPEC_ROWMAX": "1"},
    "planes8": {"PLANES8": "1"},
    "nofp16": {"NO_FP16_PLANES": "1"},
    "noplanes": {"NO_PLANES": "1"},
    "noplanes_noldsdma": {"NO_PLANES": "1", "NO_LDSDMA": "1"},
    "noplanes_noring": {"NO_PLANES": "1", "NO_GRAM_RING": "1"},
    "noplanes_nodiagsplit": {"NO_PLANES": "1", "NO_DIAG_SPLIT": "1"},
    "nobf16x3": {"NO_BF16X3": "1"},
    "nobf16x3_noldsdma": {"NO_BF16X3": "1", "NO_LDSDMA": "1"},
    "nobf16x3_noring": {"NO_BF16X3": "1", "NO_GRAM_RING": "1"},
    "nobf16x3_nodiagsplit": {"NO_BF16X3": "1", "NO_DIAG_SPLIT": "1"},
}

# 129: DP = 256, the second row block holds one row; 200; 256: whole blocks, one off-diagonal tile; 384: NC = 3, strictly lower tiles
DS = (129, 200, 256, 384)
# one column; either side of a k-block of 16 and of the f32 tile kernel's stage of 32; a ragged few hundred; whole stages everywhere
NS = (1, 15, 16, 17, 31, 33, 333, 512)
# A short or empty last column chunk of the planes pass.  plan_large: NKB = ceil(ceil(N / 16) / KBS) KBS and
# nbchunks = max(1, min(NKB, max(ceil(512 / NC), ceil(NKB / 64)))); a chunk holds per = ceil(NKB / nbchunks) k-blocks.  At D <= 384
# (NC <= 3) ceil(512 / NC) >= 171, so up to NKB = 171 -- N = 2736 -- nbchunks = NKB and every chunk is exactly one k-block: the
# smallest shapes with another chunking are D = 384 (NC = 3, nbchunks = 171) with NKB >= 172, per = 2.
#   NP = 2 (KBS = 2): N = 2725 -> ceil(N / 16) = 171, odd: the stage padding adds k-block 171, all zero columns; NKB = 172; chunks
#     0 .. 85 hold two k-blocks (chunk 85: k-block 170 with 5 real columns and the zero k-block), chunks 86 .. 170 are empty.
#   NP = 3 (KBS = 1): N = 2755 -> NKB = 173: chunks 0 .. 85 full, chunk 86 short (one k-block, 3 real columns), chunks 87 .. 170 empty.
# (The stage padding's whole zero k-block alone also shows at NP = 2 with N = 1, 17 and 33: ceil(N / 16) odd.)
N_SHORT_CHUNK = {2: 2725, 3: 2755}
XKINDS = ("col16", "colodd", "colbase1", "row")
NOISES = ("iso", "diag")
PRIORS = ("diag", "dense", "factor")
MEANS = ("zero", "nonzero")


def _on(options, key):
    return str(options.get(key, "0")) == "1"


def expected_plan(dtype, D, N, xkind, options):
    """What plan_large decides for one regressor of this type, width, observation count and loader kind on a handle with these
    options (a mapping of option names to "1"): route, planes / bf3 / x_ring, NP, and the padded dimensions of the planes pass.
    Written from csrc/blr_large_plan.hpp; the CPU test holds it against tools/large_plan_dump."""
    elem = np.dtype(dtype).itemsize
    if not 128 < D <= 8192 or N < 0:
        raise ValueError("the large-D update takes 128 < D <= 8192")
    if xkind not in XKINDS:
        raise ValueError(f"unknown loader kind {xkind!r}")
    colvecs = xkind != "row"
    x_ring = xkind == "col16"  # ColVecs whose base and ldx are multiples of 16 bytes
    bf3 = elem == 4 and not _on(options, "NO_BF16X3") and not _on(options, "NO_GRAM_RING") and x_ring
    planes = elem == 4 and not _on(options, "NO_BF16X3") and not _on(options, "NO_PLANES") and colvecs and N > 0
    NP = 3 if _on(options, "NO_FP16_PLANES") else 2
    if elem == 8:
        route = "gram_tile_kernel<double>"
    elif planes:
        route = "gram_planes_kernel<3>" if NP == 3 else ("gram_planes_kernel<2>" if _on(options, "PLANES8") else "gram_planes4_kernel")
    else:
        route = "gram_tile_kernel<float, true>" if bf3 else "gram_tile_kernel<float>"
    DP = -(-D // KPB) * KPB
    NC = DP // KPB
    kbs = PLANES_KBS[NP]
    NKB = -(-(-(-N // 16)) // kbs) * kbs
    nbchunks = max(1, min(NKB, max(-(-512 // NC), -(-NKB // PLANES_CHUNK_KB)))) if planes else 0
    return dict(route=route, planes=planes, bf3=bf3, x_ring=x_ring, NP=NP, DP=DP, NC=NC, NKB=NKB, nbchunks=nbchunks)


def expected_route(dtype, D, N, xkind, options):
    return expected_plan(dtype, D, N, xkind, options)["route"]


def planes_chunks(plan):
    """k-blocks of every column chunk of the planes pass (planes_kernel: per = ceil(NKB / nchunks), chunk x = [x per, min(NKB, x per + per)))"""
    per = -(-plan["NKB"] // plan["nbchunks"])
    return [max(0, min(plan["NKB"], x * per + per) - x * per) for x in range(plan["nbchunks"])]


def mixes_ring_and_stage_tiles(row):
    """One launch of an fp32 tile kernel holds ring-loop tiles and stage-loop tiles: the ring loop takes a macro tile with
    use_dma == 1 (aligned ColVecs, no NO_GRAM_RING), 128 full rows on both sides and a column range that is a multiple of 16 --
    every range of ANY split plan is one where N is a multiple of 16 (ranges are whole stages of 32 columns but the last) -- so at
    D = 129 / 200 tile (0, 0) is eligible and the tiles of the ragged second row block are not."""
    return (row["route"] in TILE_ROUTES_F32 and row["xkind"] == "col16" and not _on(row["options"], "NO_GRAM_RING")
            and row["N"] % 16 == 0 and row["N"] >= 16 and row["D"] in (129, 200))


# ---- the table ----------------------------------------------------------------------------------------------------------------------
_NB3 = {(129, 17), (200, 33), (200, 333), (256, 512), (384, 16), (384, 31)}  # (D, N) of the main families' groups of 3 regressors
_ALIGNED = {(129, 16), (200, 512)}                                          # ... and of their aligned-ColVecs rows (where served)
# (name, element type, option set, loader kinds the family's route serves)
_FAMILIES = (
    ("f64", np.float64, "default", XKINDS),
    ("planes4", np.float32, "default", ("col16", "colodd", "colbase1")),
    ("planes8", np.float32, "planes8", ("col16", "colodd", "colbase1")),
    ("planes3", np.float32, "nofp16", ("col16", "colodd", "colbase1")),
    ("tilebf3", np.float32, "noplanes", ("col16",)),
    ("tilef32", np.float32, "nobf16x3", XKINDS),
)
# option variants: two widths with a ragged last row block at three N each, the two whole-block widths at two
_VARIANT_SHAPES = ((129, 16), (129, 333), (200, 512), (200, 33), (256, 512), (256, 17), (384, 512), (384, 333))
_VARIANTS = (
    ("planes4_nospec", np.float32, "nospec", ("col16", "colodd", "colbase1")),
    ("tilebf3_noldsdma", np.float32, "noplanes_noldsdma", ("col16",)),
    ("tilebf3_noring", np.float32, "noplanes_noring", ("col16", "col16", "colodd", "row")),      # (NO_GRAM_RING: the plain f32 kernel, stage loop only)
    ("tilebf3_nodiagsplit", np.float32, "noplanes_nodiagsplit", ("col16",)),
    ("tilef32_noldsdma", np.float32, "nobf16x3_noldsdma", ("col16", "col16", "colbase1", "row")),
    ("tilef32_noring", np.float32, "nobf16x3_noring", ("col16", "col16", "colodd", "row")),
    ("tilef32_nodiagsplit", np.float32, "nobf16x3_nodiagsplit", ("col16", "col16", "colbase1", "row")),
    # NO_PLANES without an aligned ColVecs X: the plain f32 kernel on its register-staging loaders
    ("noplanes_generic", np.float32, "noplanes", ("colodd", "colbase1", "row")),
)


def _balanced(rng, values, n):
    """n draws that hold every value ceil(n / len) times or once less, in a fixed pseudo-random order"""
    reps = list(values) * (-(-n // len(values)))
    return [reps[i] for i in rng.permutation(len(reps))[:n]]


def _lattice():
    rows = []

    def add(fam, dtype, optset, D, N, xkind, noise, prior, mean, nb):
        options = OPTION_SETS[optset]
        rows.append(dict(id=f"{fam}-D{D}-N{N}-{xkind}-{noise}-{prior}-{mean}-nb{nb}", family=fam, dtype=dtype, D=D, N=N, xkind=xkind, noise=noise,
                         prior=prior, prior_mean=mean, nb=nb, optset=optset, options=options, seed=len(rows),
                         route=expected_route(dtype, D, N, xkind, options)))

    for f, (fam, dtype, optset, kinds) in enumerate(_FAMILIES):
        rng = np.random.Generator(np.random.PCG64(77 + f))
        shapes = [(D, N) for D in DS for N in NS]
        n = len(shapes)
        xk, no, pr, me = _balanced(rng, kinds, n), _balanced(rng, NOISES, n), _balanced(rng, PRIORS, n), _balanced(rng, MEANS, n)
        for i, (D, N) in enumerate(shapes):
            xkind = "col16" if ((D, N) in _ALIGNED and "col16" in kinds) else xk[i]
            add(fam, dtype, optset, D, N, xkind, no[i], pr[i], me[i], 3 if (D, N) in _NB3 else 1)
    for fam, dtype, optset, kinds in _VARIANTS:
        for i, (D, N) in enumerate(_VARIANT_SHAPES):
            add(fam, dtype, optset, D, N, kinds[i % len(kinds)], NOISES[i % 2], PRIORS[i % 3], MEANS[(i // 2) % 2], 3 if (D, N) == (200, 33) else 1)
    # the short / empty last chunk of the planes pass (N_SHORT_CHUNK), once per planes route and once with exact row maxima
    for fam, optset, NP, xkind, noise, prior, mean in (("planes4", "default", 2, "col16", "diag", "dense", "nonzero"),
                                                       ("planes8", "planes8", 2, "colodd", "iso", "factor", "zero"),
                                                       ("planes3", "nofp16", 3, "colbase1", "diag", "diag", "nonzero"),
                                                       ("planes4_nospec", "nospec", 2, "colodd", "diag", "diag", "zero")):
        add(fam, np.float32, optset, 384, N_SHORT_CHUNK[NP], xkind, noise, prior, mean, 1)
    return rows


LARGE_LATTICE = _lattice()


def ragged_rows():
    """one row with a ragged last row block and a ragged N per (option set, route): the first of the table, D = 200 before D = 129"""
    picked = {}
    for want_D in (200, 129):
        for r in LARGE_LATTICE:
            if r["D"] == want_D and r["N"] > 16 and r["N"] % 16 != 0:
                picked.setdefault((r["optset"], r["route"]), r)
    return list(picked.values())


# ---- problems and device images -------------------------------------------------------------------------------------------------------
def ldx_of(dtype, D, xkind, nb, cols_per):
    per16 = 16 // np.dtype(dtype).itemsize
    if xkind == "row":
        return nb * cols_per + 3
    return (D + 1) | 1 if xkind == "colodd" else -(-D // per16) * per16


def large_problem(row, nb=None):
    """The batch of a lattice row (data, noise, priors: _small_d_problems._batch with equal counts) and the image of X a device
    call reads: regressor b's N observations followed by 1 .. 4 slack observations of NaN (so that the stride between regressors
    is a multiple of 16 bytes whatever ldx: the group shares its launches), padding rows of NaN where ldx > D ("col16" at a D that
    is no multiple of the vector, "colodd"), one element in front of the base for "colbase1"."""
    nb = row["nb"] if nb is None else nb
    D, N, dtype, xkind = row["D"], row["N"], row["dtype"], row["xkind"]
    q = _batch(D, dtype, "col16", row["noise"], row["prior"], False, counts=[N] * nb, seed=row["seed"])
    if row["prior_mean"] == "zero":
        q["mw"][:] = 0
    q.update(N=N, xkind=xkind, X=None, stride_s=N if q["noise_kind"] == _abi.NOISE_DIAGONAL else q["strides"])
    return pack_image(q)


def pack_image(q):
    """(re)builds the image of X from q["Xd"]: a test that changes the data calls it again"""
    D, N, dtype, xkind, nb = q["D"], q["N"], q["dtype"], q["xkind"], q["nb"]
    cols_per = N + 4 - N % 4
    ldx = ldx_of(dtype, D, xkind, nb, cols_per)
    if xkind == "row":
        img = np.full((ldx, D), np.nan, dtype=dtype, order="F")
        for b in range(nb):
            img[b * cols_per:b * cols_per + N, :] = q["Xd"][:, b * N:(b + 1) * N].T
        q.update(layout=_abi.LAYOUT_ROWVECS, strideX=cols_per, xoff=0)
    else:
        img = np.full((ldx, nb * cols_per), np.nan, dtype=dtype, order="F")
        for b in range(nb):
            img[:D, b * cols_per:b * cols_per + N] = q["Xd"][:, b * N:(b + 1) * N]
        q.update(layout=_abi.LAYOUT_COLVECS, strideX=ldx * cols_per, xoff=1 if xkind == "colbase1" else 0)
    q["ximg"] = np.concatenate((np.full(q["xoff"], np.nan, dtype=dtype), img.reshape(-1, order="F")))
    q["ldx"] = ldx
    assert (q["strideX"] * np.dtype(dtype).itemsize) % 16 == 0
    return q


def x_of_image(q, b):
    """regressor b's D x N block as a call reads it from the image (the tests' check that image and oracle see the same numbers)"""
    D, N, ldx = q["D"], q["N"], q["ldx"]
    base = q["xoff"] + b * q["strideX"]
    if q["layout"] == _abi.LAYOUT_ROWVECS:
        idx = base + np.arange(N)[None, :] + np.arange(D)[:, None] * ldx
    else:
        idx = base + np.arange(D)[:, None] + np.arange(N)[None, :] * ldx
    return q["ximg"][idx]


def run_on_device(hd, q, o):
    """blr_posterior_batched_* in device memspace on a problem of large_problem, into device copies of the buffers of _outputs
    (gaps and fills included), which come back into o.  Every pointer is the start of an allocation of its own, but X's under
    "colbase1" (one element on): base and ldx have the alignment the row says."""
    dtype, item = q["dtype"], np.dtype(q["dtype"]).itemsize
    ins = dict(X=q["ximg"], y=q["y"], s=q["s"], mw=q["mw"], Lw=q["Lw"])
    outs = ("mw_post", "T", "A", "lp", "info")
    p = {}
    try:
        for k, a in ins.items():
            p[k] = hd.device_alloc(a.nbytes)
            hd.memcpy_h2d(p[k], a)
        for k in outs:
            p[k] = hd.device_alloc(o[k].nbytes)
            hd.memcpy_h2d(p[k], o[k])
        rc = hd.posterior_batched(dtype, _abi.MEM_DEVICE, q["layout"], q["nb"], q["D"], q["N"], p["X"] + q["xoff"] * item, q["ldx"], q["strideX"],
                                  p["y"], q["N"], q["noise_kind"], p["s"], q["stride_s"], q["prior_kind"], p["mw"], q["stridemw"], p["Lw"], q["ldl"],
                                  q["strideLw"], p["mw_post"], o["stride_mwpost"], p["T"], o["ldt"], o["strideT"], p["A"], o["ldt"], o["strideT"],
                                  p["lp"], p["info"])
        hd.synchronize()
        for k in outs:
            hd.memcpy_d2h(o[k], p[k])
    finally:
        for ptr in p.values():
            hd.device_free(ptr)
    return rc


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
FP32_FLOOR = (2e-6, 5e-7, 2e-7)  # _assert_fp32_within_lapack's default floors


def fp32_bound_used(e, yard):
    """error / (4 x yardstick + the default floor) as (the larger of mean and precision, evidence).  The first is the share of the
    bound that was used; the evidence's real floor is the yardstick's cancellation term where that is larger than the default, so
    its figure can exceed 1 on a passing row: it is an upper limit of the share."""
    r = [e[i] / (4 * yard[i] + FP32_FLOOR[i]) for i in range(3)]
    return max(r[0], r[1]), r[2]


def check_oracle(q, b, res, what=""):
    """regressor b's (mw', T, Lw', logpdf, info) against the fp64 oracle on the same inputs.  fp32: within 4 x fp32 LAPACK
    (tests/_yardsticks.py, T'T and T's zero strict lower triangle included), -> (errors, yardstick).  fp64: the tolerances of
    test_large_d_posterior_logpdf_f64 against the direct form, -> None."""
    mw_p, T, A, lp, info = res
    assert info == 0, (what, b, info)
    mw, Lw, Xb, sb, yb = _oracle_inputs(q, b)
    if q["dtype"] == np.float32:
        return _assert_fp32_within_lapack(mw, Lw, np.asfortranarray(Xb), np.asarray(sb, dtype=np.float32), yb, mw_p, A, lp, got_T=T,
                                          what=f"{what} regressor {b}")
    mw_o, T_o, A_o, lp_o = O.posterior_logpdf_direct(mw, Lw, Xb, sb, yb)
    assert abs(lp - lp_o) <= 1e-10 * abs(lp_o), (what, b, lp, lp_o)
    np.testing.assert_allclose(mw_p, mw_o, rtol=1e-8, atol=1e-10, err_msg=f"{what} mw' of regressor {b}")
    np.testing.assert_allclose(np.triu(T), T_o, rtol=1e-8, atol=1e-9, err_msg=f"{what} T of regressor {b}")
    assert np.all(np.tril(T, -1) == 0)
    np.testing.assert_allclose(A, A_o, rtol=1e-10, atol=1e-10, err_msg=f"{what} Lw' of regressor {b}")
    return None


def reference_alone(q, b):
    """the direct form in fp32 LAPACK on regressor b's fp32 inputs, as (mw', T, Lw', logpdf, info)"""
    mw, Lw, Xb, sb, yb = _oracle_inputs(q, b)
    m, T, A, lp = O.posterior_logpdf_direct(mw, Lw, np.asfortranarray(Xb), np.asarray(sb, dtype=np.float32), yb)
    assert m.dtype == np.float32 and A.dtype == np.float32
    return m, T, A, lp, 0
