"""Exact fixtures for the int8 Gram route (blr_fused_i8.hpp): a host model of what fused_i8_kernel keeps, and problem
families built on the rows' dyadic grids, for which every number the kernel forms on its way to A = diag(lam) + G / s is exactly
representable in fp64 -- so A must equal the model's integer computation bit for bit (tests/test_i8_edges_gpu.py; the fixtures
themselves are checked on the CPU in tests/test_i8_problems_cpu.py).

The model, per regressor (X is D x N, row r = feature r; under diagonal noise what is sliced is x_rn / sqrt(s_n)):
  * capacity exponent e_r = exponent of the largest |x| among the first min(N32, 96) columns (times the largest 1 / sqrt(s_n) under
    diagonal noise, both with their low words filled with ones as the prologue does) clamped at -400, + 2 (6 groups) or + 3 (7 groups);
  * Q = round-half-even(x 2^(47 - e_r)); the entry FITS iff Q + 0x8080808080 lies in [-2^47, 2^47) -- NOT symmetric: the balancing
    offset rides in the magic constant, so +2^e_r (1 - 2^-8) is out and -2^e_r (1 + 2^-8) is in;
  * balanced digits b_s of Q (top byte signed, the others minus 128, of Q + 0x8080808080); an entry that does not fit has the digits of
    the WRAPPED integer c (the low 48 mantissa bits of x + magic, whatever they are), its 32-column block is marked, and the repair
    adds x x' - c c' for that column in fp64;
  * kept: sum_n sum_{s + t < NG} b_s(i, n) b_t(j, n) 2^(80 - 8 (s + t)) in units of 2^(e_i + e_j - 94), on the diagonal of the 6-group
    plan also the pair (3, 3); the last N % 32 columns as exact products.
For entries that fit, or wrap to a c without dropped digit products, this is the plain Gram with wrapped entries at their true value."""
from fractions import Fraction

import numpy as np

D = 128
BAL = 0x8080808080
KC = 32
RW_OF_S = {0.25: 2.0, 0.0625: 4.0, 1.0: 1.0}  # the noise variances of the fixtures: 1 / sqrt(s_n) is a power of two
S_ISO = 0.125


def cap_of(NG):
    return 2 if NG == 6 else 3


def _words(hi, lo):
    return ((np.asarray(hi, np.int64).astype(np.uint64) << np.uint64(32)) | np.asarray(lo, np.int64).astype(np.uint64)).view(np.float64)


def _hi(x):
    return (np.ascontiguousarray(x, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)


def _lo(x):
    return (np.ascontiguousarray(x, np.float64).view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def _biased_capacity(X, NG, rwmax=1.0, diag=False):
    """(biased exponent field of the rows' capacities, rows whose scale the route accepts) -- the prologue of i8_gram_stream"""
    N32 = KC * (X.shape[1] // KC)
    m = (_hi(X[:, :min(N32, 96)]) & 0x7FFFFFFF).max(axis=1)
    if diag:
        with np.errstate(over="ignore", invalid="ignore"):
            mv = _words(m, np.full_like(m, 0xFFFFFFFF)) * _words(_hi(np.float64(rwmax)), 0xFFFFFFFF)
        m = _hi(mv) & 0x7FFFFFFF
    E1 = m >> 20
    ok = E1 <= 1023 + 400
    return np.maximum(E1, 1023 - 400) + cap_of(NG), ok


def capacity_exponent(X, NG, rwmax=1.0, diag=False):
    """e_r per row (unbiased).  Only the exponent FIELD of the maximum counts, as in the kernel."""
    return _biased_capacity(X, NG, rwmax, diag)[0] - 1023


def fits(x, e_r):
    """the interval rule in Python ints: round-half-even(x 2^(47 - e_r)) + 0x8080808080 in [-2^47, 2^47)"""
    if not np.isfinite(x):
        return False
    q = round(Fraction(float(x)) * Fraction(2) ** (47 - int(e_r)))  # (round() of a Fraction: half to even)
    return -(1 << 47) <= q + BAL < (1 << 47)


def fits_array(xs, e):
    """the same rule for a whole D x n block (rint: half to even; every comparison below 2^53 is exact, above it is false anyway)"""
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint(np.ldexp(xs, (47 - e)[:, None].astype(np.int32))) + float(BAL)
    return (q >= -float(1 << 47)) & (q < float(1 << 47))


def balanced_digits(Q):
    """b_0 .. b_5 of int64 Q (|Q + BAL| within 48 bits): Q = sum_s b_s 2^(8 (5 - s)), b_s in [-128, 127]"""
    Qp = np.asarray(Q, np.int64) + BAL
    out = []
    for s in range(6):
        d = (Qp >> (8 * (5 - s))) & 0xFF
        out.append(np.where(d >= 128, d - 256, d) if s == 0 else d - 128)
    return out


def slice_emulated(xs, eb):
    """the slicing itself in IEEE doubles: t = x + magic (one rounding); -> (fits by the high-word test, the integer the digits stand for)"""
    eb = np.asarray(eb, np.int64)
    Cm = _words(((eb + 5) << 20) | 0x00080080, np.full_like(eb, 0x80808080))
    hlo = ((eb + 5) << 20) | 0x00078000
    with np.errstate(over="ignore", invalid="ignore"):
        t = xs + Cm[:, None]
    hi, lo = _hi(t), _lo(t)
    ok = ((hi - hlo[:, None]) & 0xFFFFFFFF) <= 0xFFFF
    top = hi & 0xFFFF
    q48 = ((np.where(top >= 0x8000, top - 0x10000, top)) << 32) | lo
    return ok, q48 - BAL


def _obj(a):
    return np.asarray(a, np.float64).astype(np.int64).astype(object)


def _v2(n):
    n = abs(int(n))
    return (n & -n).bit_length() - 1 if n else 10 ** 6


class Model:
    """everything the host knows about one regressor on the route: marks, hand-back, the kept and the plain Gram as Python ints in
    units of 2^(e_i + e_j - 94), and the sum of |terms| / the finest unit of any term, entry by entry"""

    def __init__(self, X, NG, rw=None):
        X = np.ascontiguousarray(X, np.float64)
        assert X.shape[0] == D
        self.NG, self.N = NG, X.shape[1]
        self.N32 = KC * (self.N // KC)
        self.nk = self.N32 // KC
        diag = rw is not None
        xs = X * rw[None, :] if diag else X
        self.xs = xs
        eb, in_range = _biased_capacity(X, NG, float(rw.max()) if diag else 1.0, diag)
        self.e = eb - 1023
        self.finite = bool(np.all(np.isfinite(xs)))
        S = xs[:, :self.N32]
        self.fit = fits_array(S, self.e)
        self.fit_emulated, self.cint = slice_emulated(S, eb)
        self.marked = sorted(set((np.nonzero(~self.fit.all(axis=0))[0] // KC).tolist()))
        self.limit = min(32, max(2, self.nk // 16))
        self.handed_back = (not bool(in_range.all())) or (not self.finite) or len(self.marked) > self.limit
        self._gram_done = False

    # exact integer of an on-grid value, in units of its row's grid 2^(e_r - 47)
    def _grid_int(self, x, r):
        q = Fraction(float(x)) * Fraction(2) ** (47 - int(self.e[r]))
        assert q.denominator == 1, "an entry is not on its row's grid"
        return int(q)

    def gram(self):
        if self._gram_done:
            return
        NG = self.NG
        di = balanced_digits(self.cint)
        dg = [np.asarray(d, np.float64) for d in di]
        live = [s for s in range(6) if np.any(di[s])]
        # 2-adic valuation of the finest non-zero digit of every (plane, row): the unit of that row's products
        vrow = [np.where(di[s] != 0, np.log2(np.maximum(di[s] & -di[s], 1)).astype(np.int64), 99).min(axis=1) for s in range(6)]
        kept = np.zeros((D, D), dtype=object) + 0
        plain = np.zeros((D, D), dtype=object) + 0
        absum = np.zeros((D, D), dtype=object) + 0
        unit = np.full((D, D), 10 ** 6, dtype=np.int64)  # log2 of the finest unit of any term of the entry
        for s in live:
            for t in live:
                k = s + t
                P = dg[s] @ dg[t].T  # (|b| <= 128, N <= 16384: exact in fp64)
                Pa = np.abs(dg[s]) @ np.abs(dg[t]).T
                term = _obj(P) * (1 << (80 - 8 * k))
                plain = plain + term
                if k < NG:
                    kept = kept + term
                    absum = absum + _obj(Pa) * (1 << (80 - 8 * k))
                    unit = np.where(Pa != 0, np.minimum(unit, 80 - 8 * k + vrow[s][:, None] + vrow[t][None, :]), unit)
        if NG == 6 and 3 in live:  # TD: the diagonal's pair (3, 3)
            td = _obj((dg[3] ** 2).sum(axis=1)) * (1 << 32)
            for i in range(D):
                if td[i]:
                    kept[i, i] += td[i]
                    absum[i, i] += td[i]
                    unit[i, i] = min(unit[i, i], 32 + 2 * int(vrow[3][i]))
        # the stream's values must be the inputs (on the rows' grids) wherever they fit
        grid = np.ldexp(1.0, (self.e - 47).astype(np.int32))[:, None]
        S = self.xs[:, :self.N32]
        assert np.array_equal(np.where(self.fit, self.cint.astype(np.float64) * grid, S), S), "an entry that fits is not on its row's grid"
        # repair: x x' - c c' for every column with a wrapped entry; |terms| as the kernel forms them (d v, and 2 d v + d d on the diagonal)
        self.wrapped = [(int(r), int(n)) for n in np.nonzero(~self.fit.all(axis=0))[0] for r in np.nonzero(~self.fit[:, n])[0]]
        for n in sorted({n for _, n in self.wrapped}):
            c = np.array([int(v) for v in self.cint[:, n]], dtype=object)
            x = c.copy()
            rows = [int(r) for r in np.nonzero(~self.fit[:, n])[0]]
            for r in rows:
                x[r] = self._grid_int(S[r, n], r)
            upd = np.multiply.outer(x, x) - np.multiply.outer(c, c)
            kept = kept + upd
            plain = plain + upd
            v = c.copy()
            for r in rows:  # the kernel's order: row r's d against the column as it stands
                d = x[r] - c[r]
                for j in range(D):
                    if j != r:
                        if v[j]:
                            for a_, b_ in ((r, j), (j, r)):
                                absum[a_, b_] += abs(d * v[j])
                                unit[a_, b_] = min(unit[a_, b_], _v2(d) + _v2(v[j]))
                    else:
                        absum[r, r] += abs(2 * d * v[r]) + d * d
                        unit[r, r] = min(unit[r, r], 2 * _v2(d), _v2(d) + _v2(v[r]) + 1 if v[r] else 10 ** 6)
                v[r] = x[r]
        # the last N % 32 columns: exact products
        for n in range(self.N32, self.N):
            x = np.array([self._grid_int(self.xs[r, n], r) for r in range(D)], dtype=object)
            o = np.multiply.outer(x, x)
            kept = kept + o
            plain = plain + o
            absum = absum + abs(o)
            v = np.array([_v2(a_) for a_ in x], dtype=np.int64)
            unit = np.minimum(unit, np.where(o != 0, v[:, None] + v[None, :], 10 ** 6))
        self.kept, self.plain, self.absum, self.unit = kept, plain, absum, unit
        self._gram_done = True


def _rw(svec):
    return None if svec is None else np.array([RW_OF_S[float(v)] for v in svec])


def marked_blocks(X, NG, svec=None):
    return Model(X, NG, _rw(svec)).marked


def handed_back(X, NG, svec=None):
    return Model(X, NG, _rw(svec)).handed_back


def kept_gram(X, NG, svec=None, model=None):
    """(K, e): G_kept(i, j) = K[i, j] 2^(e_i + e_j - 94), K a D x D array of Python ints"""
    m = model or Model(X, NG, _rw(svec))
    m.gram()
    return m.kept, m.e


def assert_exact_fixture(X, lam, s, NG, svec=None, model=None, allow=()):
    """A_expected = diag(lam) + G_kept / s as float64, after checking that (1) every entry converts without rounding and (2) for every
    entry the sum of |terms| over the finest unit of any term stays below 2^53, so that ANY order of exact partial sums is exact.
    `allow`: the entries (i, j) known to miss this (the diagonal entry of an entry planted beyond 16 capacities: its repair term
    2 d c + d d needs 94 bits); they must be exactly the entries that fail, and they get the correctly rounded value.  s: the isotropic
    variance (a power of two); under diagonal noise pass s = 1 and the variances as svec."""
    m = model or Model(X, NG, _rw(svec))
    m.gram()
    lg_s = int(round(np.log2(s)))
    assert 2.0 ** lg_s == s
    A = np.zeros((D, D))
    failing = set()
    for i in range(D):
        for j in range(D):
            ex = int(m.e[i] + m.e[j]) - 94 - lg_s
            a, ab, u = int(m.kept[i, j]), int(m.absum[i, j]), int(m.unit[i, j])
            if i == j:
                li = Fraction(float(lam[i])) / Fraction(2) ** ex
                assert li.denominator == 1, "the prior is not on the diagonal entry's grid"
                a, ab, u = a + int(li), ab + abs(int(li)), min(u, _v2(int(li)))
            assert -1000 < ex + abs(a).bit_length() < 1000 and ex + u > -1000
            odd = abs(a) >> _v2(a) if a else 0
            if odd.bit_length() > 53 or (ab and (ab >> u) >= (1 << 53)):
                failing.add((i, j))
            A[i, j] = np.ldexp(float(a), ex)  # (int -> float is correctly rounded; exact unless the entry is in `failing`)
    assert failing == set(allow), f"entries whose partial sums may round: {sorted(failing)[:8]} (allowed: {sorted(allow)})"
    return A


# ==== the families ======================================================================================================================
E_CYCLE = (-12, 0, 9, 5)
PAD_ROWS = (45, 77)    # rows of the two padding entries of a threshold pair (never rows under test)
PAD_BLOCKS = (5, 9)
# planted values in capacities 2^e_r
VALUES = {"fit+": 1 - 2.0 ** -7, "out+": 1 - 2.0 ** -9, "fit-1": -1.0, "fit-": -(1 + 2.0 ** -9), "out-": -(1 + 2.0 ** -7),
          "wrap+": 1.5, "wrap-": -1.5, "far+": 64.0, "far-": -64.0}


def noise_of(noise, N):
    """-> (svec or None, rw or None)"""
    if noise == "iso":
        return None, None
    svec = np.array([0.25, 0.0625, 1.0])[np.arange(N) % 3]
    return svec, _rw(svec)


def lg_rwmax(noise):
    return 2 if noise == "diag" else 0


def dyadic(seed, N, noise, NG, E=None):
    """a regressor record: every row an anchor 2^E_r in one of the first 96 columns, all other entries m 2^(E_r - 13), |m| < 2^13 (digits
    0 and 1 of the row's grid under isotropic noise; 0 .. 2 under diagonal noise, where x / sqrt(s_n) is what is sliced)"""
    rng = np.random.Generator(np.random.PCG64(77000 + seed))
    E = np.array([E_CYCLE[r % len(E_CYCLE)] for r in range(D)]) if E is None else np.asarray(E)
    X = rng.integers(-(2 ** 13) + 1, 2 ** 13, size=(D, N)).astype(np.float64) * np.ldexp(1.0, E - 13)[:, None]
    svec, rw = noise_of(noise, N)
    if rw is not None:  # anchors sit where 1 / sqrt(s_n) is largest, so no scaled entry exceeds the scaled anchor
        acols = 1 + 3 * rng.integers(0, 31, size=D)
    else:
        acols = rng.integers(0, 95, size=D)
    X[np.arange(D), acols] = np.ldexp(1.0, E)
    return {"X": X, "E": E, "N": N, "noise": noise, "NG": NG, "svec": svec, "rw": rw, "seed": seed, "acols": acols,
            "e": E + lg_rwmax(noise) + cap_of(NG), "allow": set(), "unit": E - 13, "mw": np.zeros(D)}


def plant(p, row, col, value):
    """what the kernel slices at (row, col) becomes value x 2^e_row (value: a key of VALUES or a number of capacities)"""
    v = VALUES[value] if isinstance(value, str) else float(value)
    rwn = 1.0 if p["rw"] is None else p["rw"][col]
    p["X"][row, col] = np.ldexp(v, int(p["e"][row])) / rwn
    if abs(v) > 16 and col < KC * (p["N"] // KC):
        p["allow"].add((row, row))
    return p


def far_column(p, col):
    """a column that takes an entry beyond 16 capacities: its other entries are k 2^(E_r - 3), |k| <= 7 (the repair's products d v then fit 53 bits)"""
    rng = np.random.Generator(np.random.PCG64(99000 + p["seed"] + col))
    k = rng.integers(-7, 8, size=D).astype(np.float64)
    for r in range(D):
        if p["acols"][r] != col:
            p["X"][r, col] = k[r] * np.ldexp(1.0, int(p["E"][r]) - 3)
    return p


def pad(p, blocks=PAD_BLOCKS):
    """two other marked blocks: with them the entry under test is the third, and max(2, nk / 16) = 2 at N = 512 / 543"""
    for row, blk in zip(PAD_ROWS, blocks):
        plant(p, row, KC * blk + 4, "wrap+")
    return p


def finish(p):
    """prior on the data grid of every row, y = X'w + noise, the model"""
    rng = np.random.Generator(np.random.PCG64(55000 + p["seed"]))
    p["lam"] = rng.integers(1, 8, size=D).astype(np.float64) * np.ldexp(1.0, 2 * (p["unit"] + lg_rwmax(p["noise"])))
    w = rng.standard_normal(D) / np.ldexp(1.0, p["E"])
    sd = np.sqrt(S_ISO) if p["svec"] is None else np.sqrt(p["svec"])
    p["y"] = p["X"].T @ w + sd * rng.standard_normal(p["N"])
    p["model"] = Model(p["X"], p["NG"], p["rw"])
    return p


def expected_A(p):
    s = S_ISO if p["svec"] is None else 1.0
    return assert_exact_fixture(p["X"], p["lam"], s, p["NG"], model=p["model"], allow=p["allow"])


def plain_mask(p):
    """the entries of A for which the plain Gram (what the fp64 kernel forms) is the kept one and an exact fixture"""
    p["model"].gram()
    mask = p["model"].kept == p["model"].plain
    for i, j in p["allow"]:
        mask[i, j] = False
    return mask.astype(bool)


def _batch_values(noise, NG, N):
    """family (b), values: five neighbours of the interval's ends as THIRD marked block (padded), then wrapped entries on their own"""
    ps = []
    for i, (val, padded) in enumerate([("fit+", 1), ("out+", 1), ("fit-1", 1), ("fit-", 1), ("out-", 1), ("wrap+", 0), ("wrap-", 0), ("out+", 0)]):
        p = dyadic(100 + i, N, noise, NG)
        plant(p, (3, 40, 70, 101, 127, 0, 31, 32)[i], KC * 3 + (0, 7, 8, 23, 31, 8, 23, 0)[i], val)
        ps.append(finish(pad(p) if padded else p))
    return ps


def _batch_far(noise, NG, N=543):
    """family (b): beyond 16 capacities, both signs; column 95 / 96; the last partial block"""
    ps = []
    nk = N // KC
    for i, sign in enumerate(("far+", "far-")):
        p = dyadic(120 + i, N, noise, NG)
        col = KC * (nk - 1) + (7, 22)[i]  # (columns = 1 mod 3: the largest 1 / sqrt(s_n) under diagonal noise)
        ps.append(finish(plant(far_column(p, col), (64, 95)[i], col, sign)))
    p = dyadic(122, N, noise, NG)     # column 95 sets the capacity: 1.5 x the OLD capacity there raises it, nothing is marked but the pads
    ps.append(finish(pad(_raise(p, 10, 95))))
    p = dyadic(123, N, noise, NG)     # column 96 no longer does: the same entry there is the third mark
    ps.append(finish(pad(plant(p, 10, 96, "wrap+"))))
    p = dyadic(124, N, noise, NG)     # over-capacity entries in the last partial block: never a mark (two pads: stays on the route)
    plant(p, 20, KC * nk + 0, "wrap+"); plant(p, 99, N - 1, "out-")
    ps.append(finish(pad(p)))
    p = dyadic(125, N, noise, NG)     # an entry that wraps and is out by one unit in the last place the test sees (third mark)
    ps.append(finish(pad(plant(p, 127, KC * (nk - 1) + 31, "out-"))))
    return ps


def _batch_ends(noise, NG, N=512):
    """family (b), the ends themselves: Q + 0x8080808080 in the last high word the test accepts (2^47 - 2^32 + 0x80808080) and in the first
    (-2^47 + 0x80808080) fit, in the high words next to them (+-2^32 further out) they do not -- as third marked block, and the two that wrap once more on their own.  Their column holds k 2^(E_r - 3)
    elsewhere, so that the products with these 40- to 48-bit entries stay exact."""
    lo = 0x80808080  # (low bytes 0x80: balanced digits 2 .. 5 are zero, and Q itself has 14 bits at most)
    top, bot, above, below = (1 << 47) - (1 << 32) + lo, -(1 << 47) + lo, (1 << 47) + lo, -(1 << 47) - (1 << 32) + lo
    ends = [(top, 1), (bot, 1), (above, 1), (below, 1), (above, 0), (below, 0)]
    ps = []
    for i, (qp, padded) in enumerate(ends):
        p = dyadic(130 + i, N, noise, NG)
        col = KC * (3, N // KC - 1)[i & 1] + (7, 22)[i & 1]
        assert noise == "iso" or p["rw"][col] == 4.0
        plant(far_column(p, col), (31, 32, 64, 96, 0, 127)[i], col, (qp - BAL) / float(1 << 47))
        ps.append(finish(pad(p) if padded else p))
    return ps


def _raise(p, row, col):
    """an entry of 1.5 OLD capacities in a column that still sets the capacity: E_r and e_r go up by CAP + lg(rwmax), and it fits"""
    up = cap_of(p["NG"]) + lg_rwmax(p["noise"])
    rwn = 1.0 if p["rw"] is None else p["rw"][col]
    p["X"][row, col] = np.ldexp(1.5, int(p["e"][row])) / rwn
    assert rwn == 1.0
    p["e"] = p["e"].copy(); p["e"][row] += up
    return p


def _batch_positions(noise, NG, N=512):
    """family (b), positions: rows of all four 32-row tiles, columns 0 / 7 / 8 / 23 / 31 of a block, block 3 and the last one; no pads"""
    nk = N // KC
    spec = [(0, 3, 0, "wrap+"), (31, nk - 1, 7, "wrap-"), (32, 3, 8, "out+"), (127, nk - 1, 23, "out-"), (64, 3, 31, "wrap-"), (96, nk - 1, 31, "wrap+"),
            (63, nk - 1, 8, "wrap-"), (100, 3, 23, "wrap+")]
    return [finish(plant(dyadic(140 + i, N, noise, NG), r, KC * b + c, v)) for i, (r, b, c, v) in enumerate(spec)]


def _batch_words(noise, NG, N=2112):
    """family (b): blocks 63 / 64 / 65 -- bit 63 of the first mask word, bits 0 and 1 of the second -- and the limit nk / 16 = 4"""
    spec = [[(5, 63, 31)], [(37, 64, 0)], [(70, 65, 8)], [(5, 3, 0), (6, 63, 7), (7, 64, 8), (8, 65, 23)],
            [(5, 3, 0), (9, 10, 1), (6, 63, 7), (7, 64, 8), (8, 65, 23)], [(120, 63, 0), (121, 64, 31)]]
    ps = []
    for i, plants in enumerate(spec):
        p = dyadic(160 + i, N, noise, NG)
        for q, (r, b, c) in enumerate(plants):
            plant(p, r, KC * b + c, ("wrap+", "wrap-")[q & 1])
        ps.append(finish(p))
    return ps


def _batch_multi(noise, NG, N):
    """family (c).  N = 512: limit 2; N = 1536: limit 3"""
    nk = N // KC
    lim = max(2, nk // 16)
    spec = [
        [(3, 4, 9, "wrap+"), (17, 4, 9, "wrap-")],                       # one column, rows of one 32-row word
        [(3, 6, 31, "wrap-"), (100, 6, 31, "out+"), (64, 6, 31, "wrap+")],  # one column, rows of three words
        [(50, 7, 2, "wrap+"), (50, 7, 19, "wrap-")],                      # one row, two columns of one block (two column octets)
        [(8, 3, 0, "wrap+"), (90, nk - 1, 31, "wrap-")],                  # two blocks
        [(1 + q, 4 + 2 * q, 3 + q, "wrap+") for q in range(lim)],         # exactly the limit: repaired
        [(1 + q, 4 + 2 * q, 3 + q, "wrap-") for q in range(lim + 1)],     # one more: handed back
        [(1, 4, 5, "wrap+"), (2, 4, 5, "wrap+"), (1, 4, 6, "wrap-"), (33, 8, 5, "out-")],  # a 2 x 2 pattern in one block and another block
    ]
    ps = []
    for i, plants in enumerate(spec):
        p = dyadic(180 + i + N, N, noise, NG)
        for r, b, c, v in plants:
            plant(p, r, KC * b + c, v)
        ps.append(finish(p))
    return ps


def digit_lattice(seed, N, noise, NG):
    """family (d): row r has its anchor in column 0 (which holds nothing else) and elsewhere ONE non-zero balanced digit m at position
    r % 6 of its grid (there are six digits under both plans; every 32-row tile holds every position, so every tile pair holds every
    digit pair).  Digit 0 stays below the anchor (|m| < 2^(6 - CAP)) so that the anchor alone sets the capacity; the other digits are
    multiples of 8 in [-120, 120]: the anchors' product 2^(90 - 2 CAP) and a kept product of the lowest group, in units of
    2^(80 - 8 (NG - 1) + 6), then fit one double, and all digits can be planted at once (no split of the family is needed); the prior
    is a small integer times 2^48 of the grid's square for the same reason.  The rank-one
    anchor column makes A numerically singular (condition ~2^70): this family is held to its matrix, not to the solve."""
    rng = np.random.Generator(np.random.PCG64(66000 + seed))
    cap = cap_of(NG)
    E = np.array([E_CYCLE[r % len(E_CYCLE)] for r in range(D)])
    svec, rw = noise_of(noise, N)
    pos = np.arange(D) % 6
    lim = (1 << (6 - cap)) - 1
    m0 = rng.integers(-lim, lim + 1, size=(D, N))
    m8 = 8 * rng.integers(-15, 16, size=(D, N))
    m = np.where(pos[:, None] == 0, m0, m8)
    e = E + lg_rwmax(noise) + cap
    # what is sliced: m 2^(8 (5 - pos)) on the row's grid 2^(e - 47); the raw entry is that over 1 / sqrt(s_n)
    Xs = m.astype(np.float64) * np.ldexp(1.0, 8 * (5 - pos) + e - 47)[:, None]
    X = Xs / (rw[None, :] if rw is not None else 1.0)
    X[:, 0] = np.ldexp(1.0, E)
    p = {"X": X, "E": E, "N": N, "noise": noise, "NG": NG, "svec": svec, "rw": rw, "seed": seed, "acols": np.zeros(D, int),
         "e": e, "allow": set(), "unit": e - 47 - lg_rwmax(noise) + 24 + 0 * pos, "mw": np.zeros(D), "pos": pos, "singular": True}
    return finish(p)


def _batch_lattice(noise, NG, N=512):
    return [digit_lattice(200 + i, N, noise, NG) for i in range(6)]


def _batch_extreme(noise, NG, N=512):
    """family (e): rows at 2^(+-390) stay on the route; a row at 2^402 sends its regressor back"""
    ps = []
    for i in range(6):
        E = np.array([E_CYCLE[r % len(E_CYCLE)] for r in range(D)])
        if i in (0, 3):
            E[::3] = 390
        if i in (1, 3):
            E[1::3] = -390
        if i == 2:   # (rows at 2^-404: below the clamp of the capacity exponent)
            E[:] -= 392
        if i == 4:
            E[:] += 380
        if i == 5:
            E[::3] = 390; E[7] = 402
        p = dyadic(220 + i, N, noise, NG, E=E)
        if i == 3:
            plant(p, 3, KC * 7 + 8, "wrap-")
        ps.append(finish(p))
    return ps


def _batch_prior_mean(noise, NG, N=543):
    """the one case with a prior mean: dyadic mw (it enters b and the evidence through the finished matrix, never A)"""
    ps = []
    for i in range(6):
        p = dyadic(240 + i, N, noise, NG)
        if i % 2:
            plant(p, 11 * i, KC * (3 + i) + i, "wrap+")
        p = finish(p)
        rng = np.random.Generator(np.random.PCG64(88000 + i))
        p["mw"] = rng.integers(-8, 9, size=D).astype(np.float64) * np.ldexp(1.0, -p["E"] - 6)
        ps.append(p)
    return ps


BATCHES = {
    "values512": lambda noise, NG: _batch_values(noise, NG, 512),
    "values543": lambda noise, NG: _batch_values(noise, NG, 543),
    "far543": _batch_far,
    "ends512": _batch_ends,
    "positions512": _batch_positions,
    "words2112": _batch_words,
    "multi512": lambda noise, NG: _batch_multi(noise, NG, 512),
    "multi1536": lambda noise, NG: _batch_multi(noise, NG, 1536),
    "lattice512": _batch_lattice,
    "extreme512": _batch_extreme,
    "prior_mean543": _batch_prior_mean,
}
_cache = {}


def batch(name, noise, NG):
    """the regressors of a batch (built once per process and left unchanged)"""
    key = (name, noise, NG)
    if key not in _cache:
        _cache[key] = BATCHES[name](noise, NG)
    return _cache[key]
