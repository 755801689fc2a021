"""The launch rule of marg_blocksub_kernel (marginals_large_group, csrc/blr_abi.hip) restated in Python, and the problems and fp64
references of tests/test_marg_block_gpu.py.  Importing this needs no GPU; tests/test_marg_block_rule_cpu.py checks the arithmetic.

The kernel is the variance of every D > 128 marginal with a factor or a dense prior whose tile of inputs fits LDS.  What a test
has to reach in it is decided by the launch: the tile height RT (32 on eight waves / 16 on four), how many tiles one workgroup
walks (the input prefetch wraps into the next tile), and whether a batch's workgroups are renumbered per XCD."""
import functools

import numpy as np

import _seam_problems as SP

F64, F32 = np.float64, np.float32
KPB = 128                # kPB: columns of a block
KMAX_LDS = 156 * 1024    # MargBlockCfg::kMaxLds
IMG_ELEMS = 4 * 36 * 64  # MargGemmCfg::IMG_ELEMS: one diagonal block's triangular-inverse image
FILL = -7.0              # what the output buffers of section (c) hold before the call

# (rtol of the variance = rtol of the mean; atol of the mean = 10 rtol): tests/test_gpu_parity.py test_large_d_marginals, TOL["marginals"]
# of tests/test_chunk_seams_gpu.py
TOL = {"float64": 1e-10, "float32": 3e-4}


def padded(D):
    return (D + KPB - 1) // KPB * KPB


def lds_bytes(dtype, DP, rt=32):
    """MargBlockCfg<T, RT>::lds_bytes(DP): the tile (rows 32 bytes longer than DP), one double per wave and row, the prior mean"""
    size = np.dtype(dtype).itemsize
    waves = rt // 4
    return rt * (DP + 32 // size) * size + waves * rt * 8 + DP * size


def qualifies(dtype, D, layout="col", prior="factor", aligned=True):
    """marginals_large_group's first test (with var != NULL and N >= 1): everything else goes one regressor at a time through the
    tall-matrix sweep (or, D <= 128 / diagonal prior, through other kernels altogether)"""
    return (D > KPB and prior in ("factor", "dense") and layout == "col" and D % 16 == 0 and aligned and
            lds_bytes(dtype, padded(D)) <= KMAX_LDS)


def small_tiles(dtype, N, B, cus):
    """16-row tiles on four waves, two workgroups per CU: fp32 only, when 32-row tiles would leave CUs idle"""
    return np.dtype(dtype).itemsize == 4 and ((N + 31) // 32) * B < cus


def launch(dtype, N, B, nb, cus):
    """one launch of nb regressors of a call with B -> (rt, grid.x, tiles of a regressor)"""
    if small_tiles(dtype, N, B, cus):
        rt, slots = 16, 2 * cus
    else:
        rt, slots = 32, cus
    ntiles = (N + rt - 1) // rt
    return rt, min(ntiles, max(1, (slots + nb - 1) // nb)), ntiles


def expected_block_route(dtype, D, N, B, cus, layout="col", prior="factor", aligned=True):
    """-> (rt, walk, renumbered) as blr_get_stat reports them after a blr_marginals_batched_* call with mean and var: a factor prior
    without option MAX_CHUNK, where the batch is one launch (nb = B; the images' 256 MiB and grid.y bound it, asserted here).
    A dense prior qualifies alike but goes in chol_large's groups: (rt, None, None) -- read those two from the stat."""
    if not qualifies(dtype, D, layout, prior, aligned):
        return 0, 0, 0
    rt, gx, ntiles = launch(dtype, N, B, B, cus)
    if prior == "dense":
        return rt, None, None
    assert B <= min(65535, (256 << 20) // (padded(D) // KPB * IMG_ELEMS * np.dtype(dtype).itemsize)), "more than one chunk"
    return rt, (ntiles + gx - 1) // gx, int(B > 1 and (gx * B) % 8 == 0)


# ---- problems --------------------------------------------------------------------------------------------------------------------
def spd_factor(D, seed):
    """upper factor (row i, column j) of Bm Bm' / D + I, the prior of test_large_d_marginals"""
    rng = np.random.Generator(np.random.PCG64(seed))
    Bm = rng.standard_normal((D, D)) / np.sqrt(D)
    return np.linalg.cholesky(Bm @ Bm.T + np.eye(D)).T


@functools.lru_cache(maxsize=4)
def shared_problem(dtype, D, N, B, seed=0):
    """One X and one factor for the whole batch (the caller passes them with stride 0), every regressor its own prior mean and
    noise: one fp64 triangular solve is the reference of all B variances.  Every operand is rounded to dtype before the
    reference sees it.  -> dict: X [N, D], Ucm [D, D] (column-major storage of U), mw [B, D], s [B, N] (diagonal noise), s1 [B]
    (isotropic), and the fp64 references mean [B, N], lat [N] (|U^-T x_n|^2: var = lat + noise).  Cached: callers leave it
    unchanged."""
    rng = np.random.Generator(np.random.PCG64(77000 + 13 * D + N + seed))
    r = lambda a: a.astype(dtype).astype(F64)  # noqa: E731
    p = {"D": D, "N": N, "B": B}
    p["X"] = r(rng.standard_normal((N, D)))
    p["Ucm"] = r(np.ascontiguousarray(spd_factor(D, 77000 + D).T))
    p["mw"] = r(rng.standard_normal((B, D)))
    p["s"] = r(np.exp(0.3 * rng.standard_normal((B, N))))
    p["s1"] = p["s"][:, 0].copy()
    mean, lat = SP.marginals_ref(p["X"][None], p["mw"][None], p["Ucm"][None], np.zeros((1, N)))
    p["mean"], p["lat"] = mean[0], lat[0]
    return p


@functools.lru_cache(maxsize=2)
def distinct_problem(dtype, D, N, B, prior, seed=0):
    """Every operand of every regressor its own (tests/_seam_problems.batch), rounded to dtype.  prior "factor": Lw = the factors;
    "dense": Lw = U'U formed in fp64 and rounded -- the reference factors what the device gets.
    -> dict: X [B, N, D], Lw [B, D, D] (column-major per regressor), mw, s [B, N], s1 [B], references mean [B, N], lat [B, N].
    Cached: callers leave it unchanged."""
    q = SP.batch(B, D, N, 1, seed=88000 + D + N + B + seed)
    p = {"D": D, "N": N, "B": B}
    for k in ("X", "mw", "s", "U"):
        p[k] = q[k].astype(dtype).astype(F64)
    p["s1"] = p["s"][:, 0].copy()
    if prior == "factor":
        p["Lw"], Ucm = p["U"], p["U"]
    else:
        Uu = np.swapaxes(p["U"], 1, 2)
        p["Lw"] = (np.swapaxes(Uu, 1, 2) @ Uu).astype(dtype).astype(F64)  # (symmetric: either storage order)
        Ucm = np.linalg.cholesky(p["Lw"])                                  # lower L = U' row-major == U column-major
    mean, p["lat"] = SP.marginals_ref(p["X"], p["mw"][:, None, :], Ucm, np.zeros((B, N)))
    p["mean"] = mean[:, 0, :]
    return p


def pad_ld(a, ld):
    """[..., cols, rows] -> the same with rows padded to ld (zeros; the kernels never read them)"""
    out = np.zeros(a.shape[:-1] + (ld,), dtype=a.dtype)
    out[..., : a.shape[-1]] = a
    return out
