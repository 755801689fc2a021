"""Problems, truth and yardsticks of the evidence gradient for D <= 128 (blr_logpdf_grad_batched_*: logpdf_grad_kernel, the sweep
route, and marg_image_kernel + grad_gemm_kernel, the product route; both end in grad_reduce_kernel), the cases of
tests/test_grad_lattice_gpu.py and a HOST restatement of the route gate and of the launch heuristics (csrc/blr_abi.hip,
logpdf_grad_batched) that says which walk a case takes.  A plain module, not a conftest; importing it needs no GPU.

Truth: the closed form of oracle.blr_oracle.logpdf_grad in np.longdouble with hand-written Cholesky / substitution loops (fp64
cases), or the same closed form in NumPy float64 on the fp32-rounded inputs (fp32 cases).  Yardstick: the same closed form in plain
NumPy at the WORKING precision, every intermediate in that type.  Error of one output of one regressor: max |got - truth| / max |truth|
(logpdf: relative, absolute when |logpdf| < 1).  Bound: err_gpu <= 4 err_yardstick + FLOOR[kind, dtype] eps(dtype)."""
import functools

import numpy as np

import _seam_problems as SP
from blr_amd import _abi

F64, F32, LD = np.float64, np.float32, np.longdouble
OUTPUTS = ("logpdf", "dX", "dy", "ds", "dmw", "mw_post", "Ainv")
OPTIONAL = OUTPUTS[1:]
RB, PB = 64, 128                     # TrsmCfg::RB (inputs per sweep tile), kPB
VEC = {F64: 2, F32: 4}               # elements of a 16-byte vector (Mfma<T>::VEC)
GG_WAVES = {F64: 4, F32: 8}          # GradGemmCfg<T>::WAVES
CUS = 256                            # compute units of an MI355X: the handle does not expose its count (blr_get_stat has no such key).
# The product route's grid is min(tiles / (4 WAVES), ceil(CUS / B)): the B = 3 cases with two workgroups per regressor hold for any
# count >= 4, the B = 256 cases (one workgroup) for any count <= 256; nothing else in the lattice depends on it.
COND_MAX = 1e3

# Floors of the bound in units of eps(dtype) (x max |truth| through the error measure), one per output kind and dtype: the smallest
# power of two that covers the worst case measured over the whole lattice on the MI355X; 0 where 4 x the yardstick sufficed.  The
# measurements stand in the table at the top of tests/test_grad_lattice_gpu.py.
FLOOR = {("logpdf", "f64"): 4.0, ("dX", "f64"): 4.0, ("dy", "f64"): 0.5, ("ds", "f64"): 2.0, ("dmw", "f64"): 2.0, ("mw_post", "f64"): 4.0,
         ("Ainv", "f64"): 8.0,
         ("logpdf", "f32"): 2.0, ("dX", "f32"): 8.0, ("dy", "f32"): 1.0, ("ds", "f32"): 2.0, ("dmw", "f32"): 0.0, ("mw_post", "f32"): 8.0,
         ("Ainv", "f32"): 8.0}
FLOOR_MAX = 16.0


def name(dt):
    return "f64" if np.dtype(dt) == np.float64 else "f32"


# ---- problems ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(dt, B, D, N, prior, noise, seed=0):
    """fp64 arrays that hold values of type `dt` (generated in fp64, rounded ONCE): X [B, N, D], y [B, N], s [B, N] ("diag") or [B, 1]
    ("iso"), mw [B, D] and the prior as the ABI takes it -- "diag": precisions [B, D]; "dense": symmetric [B, D, D]; "factor": upper
    U [B, D, D] (row i, column j) with Lw = U'U.  Every regressor differs in every operand.  cond [B] is cond_2 of A = Lw + X S^-1 X'
    on the rounded inputs; the generator refuses a batch with cond > COND_MAX."""
    rng = np.random.Generator(np.random.PCG64([B, D, N, PRIORS.index(prior), NOISES.index(noise), seed, np.dtype(dt).itemsize]))
    rnd = lambda a: np.asarray(a, dtype=dt).astype(F64)  # noqa: E731
    p = {"dt": dt, "B": B, "D": D, "N": N, "prior": prior, "noise": noise}
    p["X"] = rnd(rng.standard_normal((B, N, D)) * (0.7 / np.sqrt(D)))
    p["y"] = rnd(rng.standard_normal((B, N)))
    p["s"] = rnd(np.exp(0.3 * rng.standard_normal((B, N if noise == "diag" else 1))))
    p["mw"] = rnd(rng.standard_normal((B, D)))
    U = np.triu(rng.standard_normal((B, D, D)), 1) * (0.3 / np.sqrt(D))
    U[:, np.arange(D), np.arange(D)] = 1.0 + rng.random((B, D))
    if prior == "diag":
        p["P"] = rnd(1.0 + rng.random((B, D)))
        Lw = p["P"][:, :, None] * np.eye(D)
    elif prior == "factor":
        p["P"] = rnd(U)
        Lw = np.swapaxes(p["P"], 1, 2) @ p["P"]
    else:
        Lw = rnd(np.swapaxes(U, 1, 2) @ U)
        p["P"] = Lw = np.triu(Lw) + np.swapaxes(np.triu(Lw, 1), 1, 2)  # symmetric to the bit
    A = Lw + np.swapaxes(p["X"] / np.broadcast_to(p["s"], (B, N))[:, :, None], 1, 2) @ p["X"]
    p["cond"] = np.linalg.cond(A)
    if not (p["cond"] <= COND_MAX).all():
        raise ValueError(f"ill-conditioned problem: cond(A) = {p['cond'].max():.3g} > {COND_MAX:g}")
    return p


# ---- the closed form (oracle.blr_oracle.logpdf_grad, stacked over the batch) ----------------------------------------------------------
class _NumpyLin:
    """LAPACK through NumPy: results have the type of the operands (float32 in, float32 out)"""
    chol = staticmethod(np.linalg.cholesky)
    fwd = staticmethod(lambda L, R: np.linalg.solve(L, R))                          # L Z = R
    bwd = staticmethod(lambda L, Z: np.linalg.solve(np.swapaxes(L, 1, 2), Z))       # L'G = Z


class _LoopLin:
    """hand-written loops, vectorised over the batch and the right-hand sides: any element type (np.linalg has no longdouble)"""

    @staticmethod
    def chol(A):
        L = np.zeros_like(A)
        for j in range(A.shape[1]):  # column by column
            v = A[:, j:, j] - (L[:, j:, :j] @ L[:, j, :j, None])[:, :, 0]
            L[:, j:, j] = v / np.sqrt(v[:, :1])
        return L

    @staticmethod
    def fwd(L, R):
        Z = np.zeros_like(R)
        for j in range(L.shape[1]):
            Z[:, j, :] = (R[:, j, :] - (L[:, j:j + 1, :j] @ Z[:, :j, :])[:, 0, :]) / L[:, j, j, None]
        return Z

    @staticmethod
    def bwd(L, Z):
        G = np.zeros_like(Z)
        for j in range(L.shape[1] - 1, -1, -1):
            G[:, j, :] = (Z[:, j, :] - (L[:, j + 1:, j][:, None, :] @ G[:, j + 1:, :])[:, 0, :]) / L[:, j, j, None]
        return G


def closed_form(p, dt, lin, only_logpdf=False):
    """{logpdf [B], dX [B, N, D], dy, ds [B, N], dmw, mw_post [B, D], Ainv [B, D, D]} of a problem, every operation in `dt`.  With
    w = 1 / s, A = Lw + X'W X = L L', m = A^-1 X'W (y - X mw), mw' = mw + m, r = y - X mw', Z = L^-1 [X' | I], G = L^-T Z:
    dX = (r mw'' - (A^-1 X')') W, dy = -w r, ds = -(s - r^2 - |L^-1 x|^2) / (2 s^2), dmw = X'W r, Ainv = the last D columns of G."""
    B, D, N = p["B"], p["D"], p["N"]
    c = lambda a: np.asarray(a).astype(dt)  # noqa: E731
    X, y, mw, P = c(p["X"]), c(p["y"]), c(p["mw"]), c(p["P"])
    s = np.ascontiguousarray(np.broadcast_to(c(p["s"]), (B, N)))
    sumlogdiag = lambda M: np.log(np.diagonal(M, axis1=1, axis2=2)).sum(axis=1)  # noqa: E731
    if p["prior"] == "diag":
        Lw, logdet_Lw = P[:, :, None] * np.eye(D, dtype=dt), np.log(P).sum(axis=1)
    elif p["prior"] == "factor":
        Lw, logdet_Lw = np.swapaxes(P, 1, 2) @ P, dt(2) * sumlogdiag(P)
    else:
        Lw, logdet_Lw = P, dt(2) * sumlogdiag(lin.chol(P))
    w = dt(1) / s
    A = Lw + np.swapaxes(X * w[:, :, None], 1, 2) @ X
    delta = y - (X @ mw[:, :, None])[:, :, 0]
    b = (np.swapaxes(X, 1, 2) @ (w * delta)[:, :, None])
    L = lin.chol(A)
    u = lin.fwd(L, b)
    m = lin.bwd(L, u)[:, :, 0]
    log2pi = np.log(dt(8) * np.arctan(dt(1)))
    lp = -(dt(N) * log2pi + np.log(s).sum(axis=1) + (delta * delta * w).sum(axis=1) + dt(2) * sumlogdiag(L) - logdet_Lw
           - (u[:, :, 0] * u[:, :, 0]).sum(axis=1)) / dt(2)
    for a in (Lw, logdet_Lw, w, A, delta, b, L, u, m, log2pi, lp):
        assert a.dtype == dt, (a.dtype, dt)
    if only_logpdf:
        return {"logpdf": lp}
    mwp = mw + m
    r = y - (X @ mwp[:, :, None])[:, :, 0]
    R = np.concatenate([np.swapaxes(X, 1, 2), np.broadcast_to(np.eye(D, dtype=dt), (B, D, D))], axis=2)  # [B, D, N + D]
    Z = lin.fwd(L, R)
    G = lin.bwd(L, Z)
    v = (Z[:, :, :N] * Z[:, :, :N]).sum(axis=1)
    out = {"logpdf": lp, "dX": (mwp[:, None, :] * r[:, :, None] - np.swapaxes(G[:, :, :N], 1, 2)) * w[:, :, None], "dy": -w * r,
           "ds": -(s - r * r - v) / (dt(2) * s * s), "dmw": (np.swapaxes(X, 1, 2) @ (w * r)[:, :, None])[:, :, 0], "mw_post": mwp,
           "Ainv": np.ascontiguousarray(G[:, :, N:])}
    for a in (mwp, r, R, Z, G, v) + tuple(out.values()):
        assert a.dtype == dt, (a.dtype, dt)
    return out


def _key(p):
    return (p["dt"], p["B"], p["D"], p["N"], p["prior"], p["noise"])


_TRUTH, _YARD = {}, {}


def truth(p):
    """fp64 problems: np.longdouble (x87 extended, 64-bit mantissa); fp32 problems: NumPy float64 on the rounded inputs.  Computed
    once per problem and shared; callers must not change it."""
    if _key(p) not in _TRUTH:
        if p["dt"] == F64:
            assert np.finfo(LD).nmant >= 63, "np.longdouble is not the x87 extended type on this host"
            _TRUTH[_key(p)] = closed_form(p, LD, _LoopLin)
        else:
            _TRUTH[_key(p)] = closed_form(p, F64, _NumpyLin)
    return _TRUTH[_key(p)]


def yardstick(p):
    """the closed form in plain NumPy at the working precision"""
    if _key(p) not in _YARD:
        _YARD[_key(p)] = closed_form(p, p["dt"], _NumpyLin)
        assert all(v.dtype == p["dt"] for v in _YARD[_key(p)].values())
    return _YARD[_key(p)]


# ---- error measure and bound --------------------------------------------------------------------------------------------------------------
def errors(kind, got, ref):
    """per regressor: max |got - ref| / max |ref| over the regressor's payload (logpdf: relative, absolute below 1), as floats"""
    B = ref.shape[0]
    assert np.shape(got) == ref.shape, (kind, np.shape(got), ref.shape)
    d = np.abs(np.asarray(got).astype(ref.dtype) - ref).reshape(B, -1).max(axis=1)
    scale = np.abs(ref).reshape(B, -1).max(axis=1)
    if kind == "logpdf":
        scale = np.maximum(scale, 1)
    return (d / scale).astype(F64)


def judge(p, got, regs=None, what=""):
    """Hold every output in `got` ({kind: [B, ...] payload in the truth's index order}) to the bound; prints one line of figures per
    output before asserting.  -> {kind: (worst err_gpu, its err_yardstick, floor units needed)}"""
    t, yd, eps = truth(p), yardstick(p), float(np.finfo(p["dt"]).eps)
    regs = list(range(p["B"])) if regs is None else list(regs)
    figures, failed = {}, []
    for k, g in got.items():
        eg, ey = errors(k, g, t[k])[regs], errors(k, yd[k], t[k])[regs]
        need = np.maximum(0.0, (eg - 4 * ey) / eps)
        i = int(np.argmax(need)) if need.max() > 0 else int(np.argmax(eg))
        figures[k] = (float(eg[i]), float(ey[i]), float(need.max()))
        floor = FLOOR[(k, name(p["dt"]))]
        print(f"FIG {name(p['dt'])} {k:8s} err_gpu {eg[i]:.3e} err_yard {ey[i]:.3e} ratio {eg[i] / max(ey[i], eps / 64):9.3f} "
              f"floor_needed {need.max():8.3f} eps worst_ratio {(eg / np.maximum(ey, eps / 64)).max():9.3f} [{what}]")
        if not (eg <= 4 * ey + floor * eps).all():
            failed.append((k, figures[k], floor))
    assert not failed, (what, failed)
    return figures


# ---- cases: what a GPU call is, beyond its problem ----------------------------------------------------------------------------------------
def case(dt, layout, B, D, N, prior, noise, ainv=True, no_gemm=False, xpad=3, dxpad=3, xstride_pad=3, base_off=0, bad=None, claim=None,
         seed=0):
    """layout "col" / "row"; xpad: ldx minus the rows of a column; dxpad: the same for dX (and the gap after each regressor);
    xstride_pad: elements between regressors of X; base_off: elements by which X's DEVICE pointer is shifted (device memspace);
    no_gemm: option NO_GRAD_GEMM = 1; bad: the regressor whose dense prior is negated; claim: (route, walk) this case must land on."""
    c = dict(dt=dt, layout=layout, B=B, D=D, N=N, prior=prior, noise=noise, ainv=ainv, no_gemm=no_gemm, xpad=xpad, dxpad=dxpad,
             xstride_pad=xstride_pad, base_off=base_off, bad=bad, claim=claim, seed=seed)
    rows = D if layout == "col" else N
    c["ldx"] = rows + xpad
    c["strideX"] = c["ldx"] * (N if layout == "col" else D) + xstride_pad
    c["id"] = (f"{name(dt)}-{layout}-B{B}-D{D}-N{N}-{prior}-{noise}" + ("" if ainv else "-noAinv") + ("-nogemm" if no_gemm else "")
               + f"-ldx{c['ldx']}-sx{c['strideX']}-lddx{rows + dxpad}" + (f"-off{base_off}" if base_off else "") + (f"-bad{bad}" if bad is not None else ""))
    return c


def case_problem(c):
    return problem(c["dt"], c["B"], c["D"], c["N"], c["prior"], c["noise"], c["seed"])


# ---- host restatement of logpdf_grad_batched's route gate and launch grid (csrc/blr_abi.hip) ------------------------------------------
def takes_products(c):
    """grad_gemm_kernel serves D = 128, N >= 64, B <= 65535, RowVecs or ColVecs whose ldx is a multiple of the vector width with a
    16-byte aligned base and regressor stride (and 2 B images within 1 GiB: far beyond these cases), unless NO_GRAD_GEMM is set.  A
    host-memspace X is staged into an aligned device buffer, so base_off only counts for device pointers (how the cases use it)."""
    size = np.dtype(c["dt"]).itemsize
    aligned = c["ldx"] % VEC[c["dt"]] == 0 and (c["base_off"] * size) % 16 == 0 and (c["strideX"] * size) % 16 == 0
    return not c["no_gemm"] and c["D"] == PB and c["N"] >= 64 and c["B"] <= 65535 and (c["layout"] == "row" or aligned)


def per_reg(c, cus=CUS):
    """workgroups per regressor (= dmw partials grad_reduce_kernel sums)"""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    if takes_products(c):
        return max(1, min(cdiv(cdiv(c["N"], 16), 4 * GG_WAVES[c["dt"]]), cdiv(cus, c["B"])))
    ntiles = cdiv(c["N"], RB) + (cdiv(c["D"], RB) if c["ainv"] else 0)
    return max(1, min(ntiles, cdiv(512, c["B"])))


def sweep_walk(c, cus=CUS):
    """the tiles each workgroup of a regressor takes on the sweep route, in order: "r" a tile of inputs, "p" a pseudo tile of A^-1
    (logpdf_grad_kernel: tile = blockIdx.x; tile < ntiles + npseudo; tile += gridDim.x, with npseudo from D rounded up to 16)"""
    assert not takes_products(c)
    real = -(-c["N"] // RB)
    pseudo = -(-(16 * -(-c["D"] // 16)) // RB) if c["ainv"] else 0
    g = per_reg(c, cus)
    return ["".join("r" if t < real else "p" for t in range(x, real + pseudo, g)) for x in range(g)]


def product_walk(c, cus=CUS):
    """the 16-input tiles per wave of each workgroup on the product route (tile = blockIdx.x WAVES + wave, step gridDim.x WAVES)"""
    assert takes_products(c)
    W, g, nt = GG_WAVES[c["dt"]], per_reg(c, cus), -(-c["N"] // 16)
    return [[len(range(x * W + wv, nt, g * W)) for wv in range(W)] for x in range(g)]


def sweep_vec_paths(c):
    """(vector loads with prefetch, vector stores of dX) of logpdf_grad_kernel: ColVecs, D = 128, ldx a multiple of the vector width
    and aligned regressors; stores also need lddx a multiple and aligned regressors of dX (Out pads its stride by dxpad)"""
    size, V = np.dtype(c["dt"]).itemsize, VEC[c["dt"]]
    vec = (c["layout"] == "col" and c["D"] == PB and c["ldx"] % V == 0 and (c["base_off"] * size) % 16 == 0
           and (c["B"] == 1 or (c["strideX"] * size) % 16 == 0))
    lddx = c["D"] + c["dxpad"]
    stride_dx = lddx * (c["N"] - 1) + c["D"] + c["dxpad"]
    return vec, vec and lddx % V == 0 and (c["B"] == 1 or (stride_dx * size) % 16 == 0)


# ---- the lattice ------------------------------------------------------------------------------------------------------------------------
DTL = [(F64, "col"), (F64, "row"), (F32, "col"), (F32, "row")]
SWEEP_DS = [1, 2, 15, 16, 17, 31, 33, 64, 100, 127, 128]
SWEEP_NS = [1, 63, 64, 65, 130]
NOISES, PRIORS = ["iso", "diag"], ["diag", "dense", "factor"]


def _sweep_blocks():
    """every D with every (dtype, layout); N, noise and prior rotate so that each value meets each dtype and each layout"""
    out = []
    for i, D in enumerate(SWEEP_DS):
        for k, (dt, lay) in enumerate(DTL):
            out.append(case(dt, lay, 3, D, SWEEP_NS[(i + k) % 5], PRIORS[(i + 2 * k) % 3], NOISES[(i + k // 2) % 2], no_gemm=D == PB,
                            claim=("sweep", None)))
    return out


def _sweep_walks():
    out = []
    for dt in (F64, F32):
        # D = 20, N = 130: three tiles of inputs (64, 64, 2) and one pseudo tile
        out.append(case(dt, "col", 256, 20, 130, "dense", "diag", claim=("sweep", ["rr", "rp"])))
        out.append(case(dt, "row", 512, 20, 130, "factor", "iso", claim=("sweep", ["rrrp"])))
        # D = 128 on the vector path: aligned ldx / stride, five tiles taken 3 + 2; vector and scalar stores of dX
        for dxpad in (4, 3):
            out.append(case(dt, "col", 256, 128, 130, "diag", "diag", no_gemm=True, xpad=4, dxpad=dxpad, xstride_pad=4,
                            claim=("sweep-vec" if dxpad == 4 else "sweep-vec-scalar-stores", ["rrp", "rp"])))
    return out


def _products():
    out = []
    for i, N in enumerate([64, 65, 79, 80, 130]):
        for k, (dt, lay) in enumerate(DTL):
            out.append(case(dt, lay, 3, 128, N, PRIORS[(i + k) % 3], NOISES[(i + k // 2) % 2], xpad=4 if lay == "col" else 3,
                            xstride_pad=4 if lay == "col" else 3, claim=("product", None)))
    # one workgroup per regressor takes all seven tiles, B = the CU count: fp64 deals them 2 2 2 1 over four waves, fp32 one each
    out.append(case(F64, "col", CUS, 128, 100, "diag", "diag", xpad=0, xstride_pad=0, claim=("product", [[2, 2, 2, 1]])))
    out.append(case(F32, "row", CUS, 128, 100, "diag", "iso", claim=("product", [[1] * 7 + [0]])))
    # two workgroups per regressor: grad_reduce_kernel sums two partials (fp64: N < 512 keeps the posterior off the int8 route)
    out.append(case(F64, "col", 3, 128, 300, "factor", "diag", xpad=2, xstride_pad=2, claim=("product", [[3, 3, 3, 2], [2] * 4])))
    out.append(case(F32, "col", 3, 128, 530, "dense", "iso", xpad=4, xstride_pad=4, claim=("product", [[3, 3] + [2] * 6, [2] * 8])))
    return out


def _gates():
    """(the case, must its default run equal its NO_GRAD_GEMM run bit for bit?)"""
    out = []
    for dt in (F64, F32):
        V = VEC[dt]
        al = dict(xpad=V, xstride_pad=V * (2 if dt == F64 else 1))  # aligned: ldx and the stride are multiples of 16 bytes
        out += [(case(dt, "col", 3, 128, 63, "diag", "diag", claim=("sweep", None), **al), True),
                (case(dt, "col", 3, 128, 64, "dense", "iso", xpad=1 if dt == F64 else 2, xstride_pad=V, claim=("sweep", None)), True),  # ldx 129 / 130
                (case(dt, "col", 3, 128, 64, "factor", "diag", xpad=V, xstride_pad=1 if dt == F64 else 2, claim=("sweep", None)), True),
                (case(dt, "col", 3, 128, 64, "diag", "iso", base_off=1, claim=("sweep", None), **al), True),
                (case(dt, "col", 3, 128, 64, "diag", "diag", claim=("product", None), **al), False),
                (case(dt, "row", 3, 128, 64, "dense", "diag", xpad=1, xstride_pad=1, claim=("product", None)), False)]
    return out


SWEEP_BLOCKS, SWEEP_WALKS, PRODUCTS, GATES = _sweep_blocks(), _sweep_walks(), _products(), _gates()
BROKEN = [case(dt, "col", 5, 128, 80, "dense", "diag", xpad=4, xstride_pad=4, bad=2, no_gemm=ng, claim=("sweep" if ng else "product", None))
          for dt in (F64, F32) for ng in (False, True)]
OPTIONALS = [case(dt, "col", 3, D, N, "dense", "diag", xpad=4, xstride_pad=4, claim=(route, None))
             for dt in (F64, F32) for route, D, N in (("sweep", 33, 65), ("product", 128, 80))]
ALL_CASES = SWEEP_BLOCKS + SWEEP_WALKS + PRODUCTS + [g for g, _ in GATES] + BROKEN + OPTIONALS


# ---- packing a case for the C ABI -----------------------------------------------------------------------------------------------------
PAD = np.nan  # what the padding elements of the inputs hold: a kernel that reads one poisons its result


IN_PAD = 3  # elements between the regressors of y, s, mw and Lw, and between the columns of a dense prior / upper factor


def in_strides(c):
    """element strides of the batched inputs other than X, every one above its tight value: y, s (diagonal noise: N + 3; isotropic:
    one variance per regressor, 4 apart), mw, and the prior (ldl = D + 3 for a matrix, 1 for a diagonal)"""
    D, N = c["D"], c["N"]
    ldl = 1 if c["prior"] == "diag" else D + IN_PAD
    return {"y": N + IN_PAD, "s": (N if c["noise"] == "diag" else 1) + IN_PAD, "mw": D + IN_PAD, "ldl": ldl,
            "Lw": D + IN_PAD if c["prior"] == "diag" else ldl * D + IN_PAD + 2}


def _padded(pay, ld, stride, dt):
    """[B, cols, rows] -> the flat array with leading dimension ld and regressor stride `stride`, PAD in every gap"""
    B, cols, rows = pay.shape
    a = np.full(B * stride, PAD, dtype=dt)
    idx = np.arange(B)[:, None, None] * stride + np.arange(cols)[None, :, None] * ld + np.arange(rows)[None, None, :]
    a[idx.ravel()] = np.asarray(pay, dtype=dt).ravel()
    return a


def pack(c):
    """-> (ins, outs): flat input arrays {X, y, s, mw, Lw} in the case's element type, NaN in every gap (X with base_off leading
    elements; the others at in_strides) and SP.Out sentinel-filled outputs"""
    p, dt = case_problem(c), c["dt"]
    B, D, N = c["B"], c["D"], c["N"]
    X = np.full(c["base_off"] + B * c["strideX"], PAD, dtype=dt)
    Xp = p["X"] if c["layout"] == "col" else np.swapaxes(p["X"], 1, 2)  # [B, cols, rows]
    idx = (c["base_off"] + np.arange(B)[:, None, None] * c["strideX"] + np.arange(Xp.shape[1])[None, :, None] * c["ldx"]
           + np.arange(Xp.shape[2])[None, None, :])
    X[idx.ravel()] = Xp.astype(dt).ravel()
    P = p["P"].copy()
    if c["bad"] is not None:
        assert c["prior"] == "dense"
        P[c["bad"]] *= -1.0
    if c["prior"] == "factor":
        P = np.swapaxes(P, 1, 2)  # column-major storage of the upper factor
    st = in_strides(c)
    ins = {"X": X, "y": _padded(p["y"][:, None, :], N, st["y"], dt), "s": _padded(p["s"][:, None, :], p["s"].shape[1], st["s"], dt),
           "mw": _padded(p["mw"][:, None, :], D, st["mw"], dt),
           "Lw": _padded(P[:, None, :] if c["prior"] == "diag" else P, st["ldl"], st["Lw"], dt)}
    rows, cols = (D, N) if c["layout"] == "col" else (N, D)
    outs = {"logpdf": SP.Out(F64, B), "dX": SP.Out(dt, rows, cols=cols, nb=B, pad=c["dxpad"]), "dy": SP.Out(dt, N, nb=B),
            "ds": SP.Out(dt, N, nb=B), "dmw": SP.Out(dt, D, nb=B), "mw_post": SP.Out(dt, D, nb=B),
            "Ainv": SP.Out(dt, D, cols=D, nb=B), "info": SP.Out(np.int32, B)}
    return ins, outs


def call(h, c, ins, outs, null=(), memspace=None):
    """One blr_logpdf_grad_batched_* call through _abi.Handle.logpdf_grad_batched.  null: the optional outputs passed as NULL.
    Host memspace unless the case shifts X's device pointer.  -> {name: the filled flat array} of the outputs that were passed"""
    dt, B, D, N = c["dt"], c["B"], c["D"], c["N"]
    null = set(null) | (set() if c["ainv"] else {"Ainv"})
    device = c["base_off"] != 0 if memspace is None else memspace == _abi.MEM_DEVICE
    want = [k for k in outs if k not in null]
    size = np.dtype(dt).itemsize
    ptrs, v = {}, {}
    try:
        if device:
            for k, a in list(ins.items()) + [(k, outs[k].a) for k in want]:
                ptrs[k] = h.device_alloc(a.nbytes)
                h.memcpy_h2d(ptrs[k], a)
            v = dict(ptrs, X=ptrs["X"] + c["base_off"] * size)
        else:
            assert c["base_off"] == 0
            v = dict(ins)
            v.update({k: outs[k].a.copy() for k in want})
        for k in null:
            v[k] = None
        o = outs
        diag_noise, st = c["noise"] == "diag", in_strides(c)
        h.logpdf_grad_batched(dt, _abi.MEM_DEVICE if device else _abi.MEM_HOST, _abi.LAYOUT_COLVECS if c["layout"] == "col" else _abi.LAYOUT_ROWVECS,
                              B, D, N, v["X"], c["ldx"], c["strideX"], v["y"], st["y"], _abi.NOISE_DIAGONAL if diag_noise else _abi.NOISE_ISOTROPIC,
                              v["s"], st["s"],
                              {"diag": _abi.PRIOR_DIAGONAL, "dense": _abi.PRIOR_DENSE, "factor": _abi.PRIOR_UPPER_FACTOR}[c["prior"]],
                              v["mw"], st["mw"], v["Lw"], st["ldl"], st["Lw"], v["logpdf"], v["dX"], o["dX"].ld, o["dX"].stride,
                              v["dy"], o["dy"].stride, v["ds"], o["ds"].stride, v["dmw"], o["dmw"].stride, v["mw_post"], o["mw_post"].stride,
                              v["Ainv"], o["Ainv"].ld, o["Ainv"].stride, v["info"])
        if not device:
            return {k: v[k] for k in want}
        h.synchronize()
        got = {k: np.empty_like(outs[k].a) for k in want}
        for k in want:
            h.memcpy_d2h(got[k], ptrs[k])
        return got
    finally:
        for q in ptrs.values():
            h.device_free(q)


def payloads(c, outs, got):
    """{kind: [B, ...] in the truth's index order} of the outputs a call filled (info apart)"""
    res = {}
    for k, a in got.items():
        if k == "info":
            continue
        pay = a[outs[k].idx]                      # [items, columns, rows] whatever the counts (Out.payload drops a single column)
        if k == "logpdf":
            pay = pay[0, 0]
        elif k == "Ainv" or (k == "dX" and c["layout"] == "row"):
            pay = np.swapaxes(pay, 1, 2)          # column-major [B, col, row] -> [B, row, col]; RowVecs dX [B, D, N] -> [B, N, D]
        elif k != "dX":
            pay = pay[:, 0]
        res[k] = pay
    return res
