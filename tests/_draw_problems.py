"""The lattice of the draw entry points (blr_sample_weights_*, blr_apply_weights_*, blr_rand_*, blr_rand_batched_*): named cases
at the tile seams, routes, strides and dtypes of the eight kernels they reach, the operands of a case as flat buffers with the
caller's own offsets and leading dimensions, and the references.  A plain module (CPU only), shared by
tests/test_draw_problems_cpu.py and tests/test_draw_lattice_gpu.py.

Inputs: fixed PCG64 seeds; priors as _prior of tests/test_downdate_gpu.py (unit-plus diagonal, strict upper part scaled by
0.3 / sqrt(D): the condition number is bounded by construction, test_draw_problems_cpu.py asserts the cap); s = exp(0.3 normal);
every element of an input buffer outside the logical operand (the rows between D and ld, the offset in front, the gaps between
regressors, the tail) is NaN; every output buffer is pre-filled with SENTINEL, gaps and tail included."""
import zlib
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np
import scipy.linalg as sla

from oracle import blr_oracle as O
from blr_amd import _abi

SENTINEL = -777.0
TAIL = 7  # elements behind the last column of every buffer
DT = {"f32": np.float32, "f64": np.float64}
VEC = {"f32": 4, "f64": 2}   # elements of a 16-byte load (Mfma<T>::VEC)
KC = {"f32": 32, "f64": 16}  # contraction rows per chunk of rand_project_mfma_tile (ProjCfg<T>::KC)
# 2-norm condition number of every prior factor U (a dense precision U'U: its square).  U = diag(1 + |g|) + E with E strictly upper,
# entries N(0, 0.09 / D): |E|_2 stays near 0.3 x 1.5 whatever D is, so sigma_max <= 1 + 0.3 |g|_max + |E|_2 < 2.5 and sigma_min > 0.6;
# test_draw_problems_cpu.py prints the largest value over the lattice (1.83) and asserts this cap
COND_CAP_U = 4.0

W_DIAG, W_MFMA, W_UVEC, W_LARGE, W_NS1, W_NS4 = (_abi.DRAW_W_DIAG, _abi.DRAW_W_MFMA, _abi.DRAW_W_UVEC, _abi.DRAW_W_LARGE,
                                                  _abi.DRAW_W_BATCHED_NS1, _abi.DRAW_W_BATCHED_NS4)
P_FUSED, P_SCALAR, P_MFMA = _abi.DRAW_P_FUSED, _abi.DRAW_P_SCALAR, _abi.DRAW_P_MFMA
ROUTE_BITS = dict(diag=W_DIAG, mfma=W_MFMA, uvec=W_UVEC, large=W_LARGE, batched_ns1=W_NS1, batched_ns4=W_NS4, fused=P_FUSED,
                  scalar=P_SCALAR, proj_mfma=P_MFMA)
SCALAR_REASONS = ("rowvecs", "dmod", "xoff", "ldx", "option")


@dataclass(frozen=True)
class Case:
    id: str
    entry: str                  # sample_weights | apply_weights | rand | rand_batched
    dtype: str                  # f32 | f64
    D: int
    N: int = 0
    S: int = 1
    B: int = 1
    layout: str = "col"         # col | row
    prior: str = "diag"         # diag | dense | factor
    noise: Optional[str] = None  # None (noise-free) | iso | diag
    ldx: int = 0
    ldw: int = 0
    ldz1: int = 0
    ldz2: int = 0
    ldy: int = 0
    ldl: int = 0
    off: tuple = ()             # ((operand, elements in front of it), ...)
    strideX: Optional[int] = None  # None: one X per regressor at the natural (16-byte multiple) stride; 0: shared
    options: tuple = ()         # ((key, value), ...) of blr_set_option
    route: int = 0              # the draw_route the call must report
    want_W: bool = True         # rand_batched: pass a W output
    bad: Optional[tuple] = None  # rand_batched: (regressor, 1-based index of its non-positive diagonal entry)
    chunks: Optional[int] = None  # last_chunks the call must report
    seed_key: str = ""          # cases with the same key get the same numbers
    group: str = ""             # cases of one group must agree bit for bit in W

    def offset(self, name):
        return dict(self.off).get(name, 0)

    @property
    def np_dtype(self):
        return DT[self.dtype]

    @property
    def x_shape(self):  # the stored matrix: D x N (ColVecs) or N x D (RowVecs)
        return (self.D, self.N) if self.layout == "col" else (self.N, self.D)


@dataclass(frozen=True)
class Geo:
    rows: int
    cols: int
    ld: int
    off: int
    stride: int
    count: int
    out: bool

    @property
    def extent(self):
        return (self.cols - 1) * self.ld + self.rows if self.rows > 0 and self.cols > 0 else 0

    @property
    def size(self):
        return self.off + (self.count - 1) * self.stride + self.extent + TAIL


def _up(n, m):
    return (n + m - 1) // m * m


def operands(c):
    """name -> Geo of every operand the call of case c takes"""
    D, N, S, B = c.D, c.N, c.S, c.B
    g = {}
    has_x = c.entry != "sample_weights" and N > 0  # (N = 0: weights only, X and Y are NULL)
    if has_x:
        r, k = c.x_shape
        natural = _up(c.ldx * k, 4) + 4
        sx = natural if c.strideX is None else c.strideX
        g["X"] = Geo(r, k, c.ldx, c.offset("X"), sx, 1 if sx == 0 else B, False)
    if c.entry == "apply_weights":
        g["W"] = Geo(D, S, c.ldw, c.offset("W"), 0, 1, False)
        g["Y"] = Geo(N, S, c.ldy, c.offset("Y"), 0, 1, True)
        return g
    g["mw"] = Geo(D, 1, D, c.offset("mw"), D + 1, B, False)
    if c.prior == "diag":
        g["L"] = Geo(D, 1, D, c.offset("L"), D + 1, B, False)
    else:
        g["L"] = Geo(D, D, c.ldl, c.offset("L"), c.ldl * D + 2, B, False)
    g["Z1"] = Geo(D, S, c.ldz1, c.offset("Z1"), c.ldz1 * S + 1, B, False)
    if c.entry == "sample_weights" or (c.entry == "rand_batched" and c.want_W):
        g["W"] = Geo(D, S, c.ldw, c.offset("W"), c.ldw * S + 2, B, True)
    if has_x:
        if c.noise is not None:
            ns = N if c.noise == "diag" else 1
            g["s"] = Geo(ns, 1, ns, c.offset("s"), ns + (1 if c.noise == "diag" else 0), B, False)
            g["Z2"] = Geo(N, S, c.ldz2, c.offset("Z2"), c.ldz2 * S + 1, B, False)
        g["Y"] = Geo(N, S, c.ldy, c.offset("Y"), c.ldy * S + 1, B, True)
    return g


def moved_bytes(c):
    return sum(g.size for g in operands(c).values()) * np.dtype(c.np_dtype).itemsize


def _view(buf, g, b):
    it = buf.itemsize
    base = g.off + b * g.stride
    return np.lib.stride_tricks.as_strided(buf[base:], shape=(g.rows, g.cols), strides=(it, g.ld * it), writeable=True)


def pack(mats, g, dtype):
    """flat buffer of operand g holding mats (one per regressor): NaN (input) or SENTINEL (output) everywhere else"""
    buf = np.full(g.size, SENTINEL if g.out else np.nan, dtype=dtype)
    if not g.out and g.rows > 0 and g.cols > 0:
        for b in range(g.count):
            _view(buf, g, b)[...] = mats[b]
    return buf


def unpack(buf, g, b=0):
    return _view(buf, g, b).copy()


def logical_mask(g, regs=None):
    """True where buffer elements belong to the logical operand (of the regressors regs; default all)"""
    m = np.zeros(g.size, dtype=bool)
    if g.rows > 0 and g.cols > 0:
        for b in (range(g.count) if regs is None else regs):
            _view(m, g, b)[...] = True
    return m


def prior_factor(rng, D):
    """_prior of tests/test_downdate_gpu.py: unit-plus diagonal, strict upper part scaled by 0.3 / sqrt(D)"""
    U = np.triu(rng.standard_normal((D, D))) * (0.3 / np.sqrt(D))
    U[np.diag_indices(D)] = 1.0 + np.abs(U[np.diag_indices(D)])
    return U


def problem(c):
    """The logical operands of case c, rounded to its dtype and returned in fp64 (exactly representable): dict of per-regressor lists
    X (D x N whatever the layout), mw, L (d | precision | U, as the library takes it), Z1, Z2, s, and W for apply_weights."""
    rng = np.random.Generator(np.random.PCG64(zlib.crc32((c.seed_key or c.id).encode())))
    dt = c.np_dtype
    r64 = lambda a: np.asarray(a, dtype=dt).astype(np.float64)
    D, N, S, B = c.D, c.N, c.S, c.B
    p = dict(X=[], mw=[], L=[], Z1=[], Z2=[], s=[], W=[])
    if c.entry == "apply_weights":
        p["X"].append(r64(rng.standard_normal((D, N)) / np.sqrt(D)))
        p["W"].append(r64(rng.standard_normal((D, S))))
        return p
    for b in range(B):
        if c.entry != "sample_weights" and (b == 0 or c.strideX != 0):
            p["X"].append(r64(rng.standard_normal((D, N)) / np.sqrt(D)))
        p["mw"].append(r64(rng.standard_normal(D)))
        if c.prior == "diag":
            L = np.exp(0.3 * rng.standard_normal(D))
        else:
            U = prior_factor(rng, D)
            L = U if c.prior == "factor" else U.T @ U
        L = r64(L)
        if c.bad is not None and c.bad[0] == b:
            k = c.bad[1] - 1
            if c.prior == "diag":
                L[k] = -1.0
            elif c.prior == "factor":
                L[k, k] = 0.0
            else:
                L[k, k] = -50.0
        p["L"].append(L)
        p["Z1"].append(r64(rng.standard_normal((D, S))))
        if c.noise is not None:
            p["Z2"].append(r64(rng.standard_normal((N, S))))
            p["s"].append(r64(np.exp(0.3 * rng.standard_normal(N if c.noise == "diag" else 1))))
    return p


def buffers(c, p):
    """name -> flat numpy buffer of case c's dtype (inputs packed, outputs at SENTINEL), plus info for rand_batched"""
    g = operands(c)
    dt = c.np_dtype
    col = lambda v: np.asarray(v).reshape(-1, 1)
    bufs = {}
    for name, geo in g.items():
        if geo.out:
            mats = None
        elif name == "X":
            mats = [x if c.layout == "col" else x.T for x in p["X"]]
        elif name in ("mw", "s") or (name == "L" and c.prior == "diag"):
            mats = [col(v) for v in p[name]]
        else:
            mats = p[name]
        bufs[name] = pack(mats, geo, dt)
    if c.entry == "rand_batched":
        bufs["info"] = np.full(c.B, -5, dtype=np.int32)
    return bufs


# ---- references ---------------------------------------------------------------------------------------------------------------------
def _chol_upper_ld(P):
    """upper Cholesky factor in np.longdouble (outer-product form)"""
    A = np.array(P, dtype=np.longdouble)
    D = A.shape[0]
    U = np.zeros_like(A)
    for k in range(D):
        U[k, k] = np.sqrt(A[k, k])
        U[k, k + 1:] = A[k, k + 1:] / U[k, k]
        A[k + 1:, k + 1:] -= np.outer(U[k, k + 1:], U[k, k + 1:])
    return U


def _backsub_ld(U, Z):
    """U^-1 Z by column-oriented back substitution in np.longdouble"""
    U = np.asarray(U, dtype=np.longdouble)
    Z = np.array(Z, dtype=np.longdouble)
    for j in range(U.shape[0] - 1, -1, -1):
        Z[j] /= U[j, j]
        if j:
            Z[:j] -= np.outer(U[:j, j], Z[j])
    return Z


def ref_weights(c, p, b, prec="f64"):
    """mw + U^-1 Z1 of regressor b from the rounded inputs: prec = ld (np.longdouble substitution), f64 or f32 (LAPACK: potrf of a
    dense precision, then trtrs; a diagonal prior: sqrt, divide, add in that precision)"""
    dt = dict(ld=np.longdouble, f64=np.float64, f32=np.float32)[prec]
    mw, L, Z = (np.asarray(p[k][b], dtype=dt) for k in ("mw", "L", "Z1"))
    if c.prior == "diag":
        return mw[:, None] + Z / np.sqrt(L)[:, None]
    if prec == "ld":
        U = _chol_upper_ld(L) if c.prior == "dense" else np.triu(L)
        return mw[:, None] + _backsub_ld(U, Z)
    U = sla.cholesky(L, lower=False, check_finite=False) if c.prior == "dense" else np.triu(L)
    V = sla.solve_triangular(U, Z, lower=False, check_finite=False)
    assert V.dtype == dt
    return mw[:, None] + V


def noise_term(c, p, b):
    """sqrt.(s) .* Z2 of regressor b in fp64 (zeros for a noise-free case)"""
    if c.noise is None:
        return np.zeros((c.N, c.S))
    sd = np.sqrt(p["s"][b]) if c.noise == "diag" else np.full(c.N, np.sqrt(p["s"][b][0]))
    return sd[:, None] * p["Z2"][b]


def x_of(c, p, b):
    return p["X"][0 if c.strideX == 0 else b]


def gamma(k, eps):
    return k * eps / (1.0 - k * eps)


def projection_bound(c, X, W, noise):
    """gamma(D + 2) |X|'|W| + 2 eps |sqrt(s) Z2|, eps that of the dtype: D products and D - 1 additions in any order (fused or not,
    on the matrix cores or not) stay within gamma_u(D) |X|'|W| with u = eps / 2, the sqrt, the product with z and the final addition
    within the rest; the fp64 product the result is compared with has its own gamma(D) of fp64, which the factor 2 between eps and
    u absorbs in fp64 and which vanishes in fp32"""
    eps = float(np.finfo(c.np_dtype).eps)
    return gamma(c.D + 2, eps) * (np.abs(X).T @ np.abs(W)) + 2 * eps * np.abs(noise)


def weights_tolerance(c, p, b):
    """(reference, elementwise-or-scalar bound, yardstick) for W of regressor b.  Diagonal prior: 3 eps (|mw| + |ref - mw|) from one
    sqrt, one divide, one add.  Dense / factor: 4 x the max-abs error LAPACK of the case's dtype makes on the same inputs + 4 ulps of
    max |ref|; fp32 is measured against the fp64 reference, fp64 against the np.longdouble substitution."""
    eps = float(np.finfo(c.np_dtype).eps)
    ref = ref_weights(c, p, b, "ld" if c.dtype == "f64" else "f64")
    if c.prior == "diag":
        mw = p["mw"][b][:, None]
        return ref, np.asarray(3 * eps * (np.abs(mw) + np.abs(ref - mw)), dtype=np.float64), None
    yard = float(np.max(np.abs(ref_weights(c, p, b, c.dtype) - ref)))
    return ref, 4 * yard + 4 * eps * float(np.max(np.abs(ref))), yard


# ---- the route the host picks, from the fields of a case (mirror of csrc/blr_abi.hip) -------------------------------------------------
def _aligned16(c, name, ld, stride=0):
    it = np.dtype(c.np_dtype).itemsize
    return (c.offset(name) * it) % 16 == 0 and (ld * it) % 16 == 0 and (stride * it) % 16 == 0


def scalar_reasons(c):
    """why the projection of case c cannot run on the matrix cores (empty: it can)"""
    r = []
    if dict(c.options).get("NO_MFMA_PROJECT"):
        r.append("option")
    if c.layout == "row":
        r.append("rowvecs")
    if c.D % VEC[c.dtype]:
        r.append("dmod")
    it = np.dtype(c.np_dtype).itemsize
    sx = operands(c)["X"].stride if c.entry == "rand_batched" and c.D <= 128 else 0
    if (c.offset("X") * it) % 16 or (sx * it) % 16:
        r.append("xoff")
    if (c.ldx * it) % 16:
        r.append("ldx")
    if c.entry == "apply_weights" and not _aligned16(c, "W", c.ldw):
        r.append("w")
    # (D > 128 batched: the projection reads the caller's W when there is one -- such cases pass none, the side buffer has ld = D)
    assert not (c.entry == "rand_batched" and c.D > 128 and c.want_W)
    return r


def expected_route(c):
    D, N, S = c.D, c.N, c.S
    proj = c.entry != "sample_weights" and N > 0
    pbit = 0
    if proj:
        pbit = P_SCALAR if scalar_reasons(c) else P_MFMA
    if c.entry == "apply_weights":
        return pbit
    if c.entry == "rand_batched" and D <= 128:
        fuse = proj and N * S <= 512
        return (W_NS1 if S == 1 else W_NS4) | (P_FUSED if fuse else pbit)
    if c.prior == "diag":
        return W_DIAG | pbit
    if D > 128:
        return W_LARGE | pbit
    # the factor sample_weights_mfma_kernel reads: the caller's, or the library's own Cholesky factor (ld = D, aligned)
    own = c.prior == "dense"
    uvec = D == 128 and (own or (c.ldl % VEC[c.dtype] == 0 and (c.offset("L") * np.dtype(c.np_dtype).itemsize) % 16 == 0))
    return W_MFMA | (W_UVEC if uvec else 0) | pbit


# ---- the lattice ----------------------------------------------------------------------------------------------------------------------
def _weights_small():
    out = []
    Ss = [1, 63, 64, 65, 129]
    for dt in ("f32", "f64"):
        for i, D in enumerate([1, 15, 16, 17, 33, 112, 113, 127, 128]):  # the edges of nchunks = ceil(D / 16)
            for j, prior in enumerate(("diag", "dense", "factor")):
                S = Ss[(i + 2 * j) % 5]
                ldl = D + 2 * VEC[dt]  # (D = 128, factor: aligned, the vector loader runs; its other two cases are below)
                route = W_DIAG if prior == "diag" else W_MFMA | (W_UVEC if D == 128 else 0)
                out.append(Case(f"w-{dt}-D{D}-{prior}-S{S}", "sample_weights", dt, D, S=S, prior=prior, ldl=ldl, ldz1=D + 3, ldw=D + 5,
                                route=route))
        # the grid-stride loops: more than 512 tiles of 64 draws; more than 1024 x 256 elements
        out.append(Case(f"w-{dt}-D16-factor-S{512 * 64 + 65}", "sample_weights", dt, 16, S=512 * 64 + 65, prior="factor", ldl=17, ldz1=19,
                        ldw=21, route=W_MFMA))
        S = 1024 * 256 // 17 + 1
        out.append(Case(f"w-{dt}-D17-diag-S{S}", "sample_weights", dt, 17, S=S, prior="diag", ldz1=20, ldw=22, route=W_DIAG))
        # the 16-byte loader of U at D = 128 and its two ways out: the same numbers, the same bits
        odd = 129 if dt == "f64" else 130
        for name, ldl, off, route in (("uvec", 128, 0, W_MFMA | W_UVEC), ("ldodd", odd, 0, W_MFMA), ("ptroff", 128, 1, W_MFMA)):
            out.append(Case(f"w-{dt}-D128-factor-S65-{name}", "sample_weights", dt, 128, S=65, prior="factor", ldl=ldl, ldz1=131, ldw=133,
                            off=(("L", off),), route=route, seed_key=f"uvec-{dt}", group=f"uvec-{dt}"))
    return out


def _weights_large():
    out = []
    for dt in ("f32", "f64"):
        for D in (129, 144, 256, 257):
            for prior in ("diag", "dense", "factor"):
                for S in (1, 5) + ((1025,) if D == 129 else ()):  # 1025 crosses the chunk of 1024 draws
                    out.append(Case(f"wl-{dt}-D{D}-{prior}-S{S}", "sample_weights", dt, D, S=S, prior=prior, ldl=D + 1, ldz1=D + 3,
                                    ldw=D + 5, route=W_DIAG if prior == "diag" else W_LARGE))
    return out


def _apply():
    out = []
    Ns, Ss = [1, 127, 128, 129, 257], [1, 15, 16, 17, 63, 64, 65]
    Dm = dict(f64=[16, 18, 32, 34, 48, 64, 66, 80], f32=[32, 36, 64, 68, 96, 128, 132, 160])  # nchunks 1 2 2 3 3 4 5 5
    for dt in ("f32", "f64"):
        v = VEC[dt]
        for i, D in enumerate(Dm[dt]):  # every D (so every nchunks, with and without a partial last chunk) meets every S and every N
            for k, S in enumerate(Ss):
                N = Ns[(i + k) % 5]
                base = Case(f"a-{dt}-D{D}-N{N}-S{S}-mfma", "apply_weights", dt, D, N=N, S=S, ldx=D + 2 * v, ldw=D + v, ldy=N + 3,
                            route=P_MFMA, seed_key=f"a-{dt}-D{D}-N{N}-S{S}")
                out.append(base)
                out.append(replace(base, id=f"a-{dt}-D{D}-N{N}-S{S}-nomfma", options=(("NO_MFMA_PROJECT", "1"),), route=P_SCALAR))
        # the scalar tiles, one reason at a time (D = 32 or 64 is eligible but for the reason named)
        Nc, S4 = [1, 63, 64, 65, 130], [1, 63, 64, 65]
        for i, D in enumerate([1, 31, 32, 33, 65]):
            N, S = Nc[i], S4[i % 4]
            out.append(Case(f"a-{dt}-D{D}-N{N}-S{S}-rowvecs", "apply_weights", dt, D, N=N, S=S, layout="row", ldx=_up(N, v) + v,
                            ldw=_up(D, v) + v, ldy=N + 3, route=P_SCALAR))
        for i, D in enumerate([1, 31, 33, 65] + ([34] if dt == "f32" else [])):
            N, S = Nc[(i + 1) % 5], S4[(i + 2) % 4]
            out.append(Case(f"a-{dt}-D{D}-N{N}-S{S}-dmod", "apply_weights", dt, D, N=N, S=S, ldx=_up(D, v) + v, ldw=_up(D, v) + 2 * v,
                            ldy=N + 3, route=P_SCALAR))
        for i in range(5):
            D, N, S = (32, 64)[i % 2], Nc[(i + 2) % 5], S4[(i + 1) % 4]
            out.append(Case(f"a-{dt}-D{D}-N{N}-S{S}-xoff", "apply_weights", dt, D, N=N, S=S, ldx=D + 2 * v, ldw=D + v, ldy=N + 3,
                            off=(("X", 1),), route=P_SCALAR))
            N, S = Nc[(i + 3) % 5], S4[(i + 3) % 4]
            out.append(Case(f"a-{dt}-D{D}-N{N}-S{S}-ldxodd", "apply_weights", dt, D, N=N, S=S, ldx=D + 1, ldw=D + v, ldy=N + 3,
                            route=P_SCALAR))
        out.append(Case(f"a-{dt}-D32-N65-S17-woff", "apply_weights", dt, 32, N=65, S=17, ldx=32 + 2 * v, ldw=32 + v, ldy=68,
                        off=(("W", 1),), route=P_SCALAR))
    return out


def _rand():
    out = []
    priors = ("diag", "dense", "factor")
    k = 0
    for dt in ("f32", "f64"):
        v = VEC[dt]
        for noise in ("iso", "diag"):
            for D in (16, 128, 130):
                for layout in ("col", "row"):
                    prior = priors[k % 3]
                    N, S = (65, 129)[k % 2], (17, 65)[(k // 2) % 2]
                    k += 1
                    wbit = W_DIAG if prior == "diag" else (W_LARGE if D > 128 else W_MFMA | (W_UVEC if D == 128 else 0))
                    pbit = P_MFMA if layout == "col" and D % v == 0 else P_SCALAR
                    out.append(Case(f"r-{dt}-D{D}-N{N}-S{S}-{layout}-{prior}-{noise}", "rand", dt, D, N=N, S=S, layout=layout,
                                    prior=prior, noise=noise, ldx=(D + 2 * v) if layout == "col" else _up(N, v) + v, ldl=D + v,
                                    ldz1=D + 3, ldz2=N + 2, ldy=N + 3, route=wbit | pbit))
    return out


def _batched():
    out = []
    priors = ("diag", "dense", "factor")
    noises = (None, "iso", "diag")
    for dt in ("f32", "f64"):
        v = VEC[dt]
        k = 0

        def case(tag, B, D, N, S, route, layout="col", ldx=None, **kw):
            nonlocal k
            prior = kw.pop("prior", priors[k % 3])
            noise = kw.pop("noise", noises[(k // 2) % 3])
            k += 1
            if ldx is None:
                ldx = (_up(D, v) + v) if layout == "col" else _up(N, v) + v
            return Case(f"b-{dt}-B{B}-D{D}-N{N}-S{S}-{tag}", "rand_batched", dt, D, N=N, S=S, B=B, layout=layout, prior=prior, noise=noise,
                        ldx=ldx, ldl=D + 1, ldz1=D + 3, ldz2=N + 2, ldw=D + 5, ldy=N + 3, route=route, **kw)

        # fused (N S <= 512): the projection's loop over blocks of 64 inputs makes 2 to 8 trips; NS = 1 | 4 with full / partial last block
        Bs, Ds = (1, 3, 37), (5, 64, 65, 128)
        for i, (N, S) in enumerate([(512, 1), (65, 1), (65, 4), (65, 5), (65, 7), (128, 1), (128, 4), (100, 1), (100, 4), (100, 5)]):
            out.append(case("fused", Bs[i % 3], Ds[i % 4], N, S, (W_NS1 if S == 1 else W_NS4) | P_FUSED, layout=("col", "row")[i % 2]))
        # the first unfused shape, and the weights alone
        out.append(case("unfused", 3, 64, 513, 1, W_NS1 | P_MFMA))
        out.append(case("weights", 37, 33, 0, 7, W_NS4, noise=None))
        # unfused on both projections: Wt's ld is D rounded up to 4
        small = P_MFMA if dt == "f64" else P_SCALAR  # 6 and 30 are multiples of 2, not of 4
        out.append(case("unfused", 37, 6, 130, 5, W_NS4 | small))
        out.append(case("unfused", 3, 30, 257, 4, W_NS4 | small))
        out.append(case("unfused", 37, 100, 129, 5, W_NS4 | P_MFMA))
        out.append(case("unfused", 3, 128, 130, 7, W_NS4 | P_MFMA, want_W=False))
        out.append(case("dmod", 3, 33, 130, 5, W_NS4 | P_SCALAR))
        out.append(case("rowvecs", 3, 64, 130, 5, W_NS4 | P_SCALAR, layout="row"))
        out.append(case("xoff", 3, 64, 130, 5, W_NS4 | P_SCALAR, off=(("X", 1),)))
        out.append(case("ldxodd", 3, 64, 130, 5, W_NS4 | P_SCALAR, ldx=65))
        sx = _up((64 + v) * 130, 4) + 4
        out.append(case("stridex", 3, 64, 130, 5, W_NS4 | P_SCALAR, strideX=sx + 1))
        out.append(case("nomfma", 37, 64, 130, 5, W_NS4 | P_SCALAR, options=(("NO_MFMA_PROJECT", "1"),)))
        # one X for all regressors: the workgroups are enumerated regressor-fastest
        out.append(case("sharedx", 37, 64, 257, 5, W_NS4 | P_MFMA, strideX=0))
        out.append(case("sharedx-rowvecs", 3, 64, 130, 5, W_NS4 | P_SCALAR, layout="row", strideX=0))
        # MAX_CHUNK = 2 with five regressors: three projection launches, the last of one regressor
        for tag, sxv, lay, pb in (("chunk", None, "col", P_MFMA), ("chunk-sharedx", 0, "col", P_MFMA), ("chunk-sharedx-rowvecs", 0, "row", P_SCALAR)):
            out.append(case(tag, 5, 64, 257, 5, W_NS4 | pb, layout=lay, strideX=sxv, options=(("MAX_CHUNK", "2"),), chunks=3))
        # a failed regressor in the middle (status from the second ballot: rows 64 and above)
        out.append(case("bad", 3, 128, 130, 5, W_NS4 | P_MFMA, prior="diag", bad=(1, 66)))
        out.append(case("bad", 3, 100, 513, 1, W_NS1 | P_MFMA, prior="factor", bad=(1, 97)))
        # D > 128: one regressor after the other on the single-regressor kernels
        out.append(case("large", 3, 130, 65, 5, W_LARGE | small, prior="factor", want_W=False))
    return out


LATTICE = _weights_small() + _weights_large() + _apply() + _rand() + _batched()
BY_ENTRY = {e: [c for c in LATTICE if c.entry == e] for e in ("sample_weights", "apply_weights", "rand", "rand_batched")}
