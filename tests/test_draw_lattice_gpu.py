"""Every draw kernel at its tile seams, routes, strides and dtypes: blr_sample_weights_*, blr_apply_weights_*, blr_rand_* and
blr_rand_batched_* over the lattice of tests/_draw_problems.py, on torch device tensors (the offsets and leading dimensions are
the caller's own).  Each case asserts, in this order: status and blr_get_stat "draw_route"; that nothing outside the logical output
moved and no NaN of the input padding reached a result; the projection within gamma(D + 2) |X|'|W| + 2 eps |sqrt(s) Z2| of the
fp64 product of the same rounded inputs; the weights within 3 eps (|mw| + |ref - mw|) (diagonal prior) or 4 x the error LAPACK of
the same precision makes on the same inputs + 4 ulps of max |ref| (tests/_yardsticks.py's convention); route equivalences bit for bit.
All tests need an MI355X.

Largest (gpu error) / (LAPACK error) of the weights per kernel and dtype over the lattice (max-abs errors; cases where LAPACK is
exact are judged by the floor alone and are not in the ratio), as printed by test_zz_report_ratios:

    kernel                                   f32      f64
    sample_weights_mfma_kernel (scalar)      3.33     3.58
    sample_weights_mfma_kernel (uvec)        3.33     2.52
    D > 128 wave solves                      4.40     2.77
    rand_batched_solve_kernel NS = 1         8.93     5.97
    rand_batched_solve_kernel NS = 4         4.22     5.12

The ratios above 4 (the D > 128 solves in fp32 at D = 256 with a dense prior; rand_batched_solve_kernel, whose column-oriented
substitution multiplies by a rounded reciprocal of the pivot; at NS = 1 the yardstick is the largest error of a single column) are
of cases where LAPACK's own error is about one ulp of max |ref| or less (8.93: gpu 1.34e-6, LAPACK 1.5e-7, max |ref| about 3):
they pass on the floor of 4 ulps, not on the factor, which stays 4.  The explicit 16 x 16 block inverses of the MFMA sweep stay
below 4 x on their own.
"""
import numpy as np
import pytest

import _draw_problems as DP

pytestmark = pytest.mark.gpu

RATIOS = {}  # (kernel, dtype) -> (largest gpu error / LAPACK error, case id)


@pytest.fixture(scope="module")
def B():
    import blr_amd

    blr_amd._abi.default_handle()  # raises if the extension or the GPU is missing: no silent fallback
    return blr_amd


@pytest.fixture
def opt(B):
    """blr_set_option on the process-wide handle, restored to the default after the test."""
    h = B._abi.default_handle()
    touched = []

    def set_(key, value):
        h.set_option(key, value)
        touched.append(key)

    yield set_
    for key in touched:
        h.set_option(key, None)


class Call:
    """One case on the device: the operands as torch tensors, the call, the outputs back on the host."""

    def __init__(self, c, p=None):
        import torch

        self.c, self.g = c, DP.operands(c)
        self.p = DP.problem(c) if p is None else p
        self.host = DP.buffers(c, self.p)
        self.dev = {k: torch.from_numpy(v).cuda() for k, v in self.host.items()}
        for t in self.dev.values():
            assert t.data_ptr() % 16 == 0  # (the lattice's offsets are relative to a 16-byte boundary)
        torch.cuda.synchronize()  # (torch's copies run on its own stream, the library on the handle's)

    def ptr(self, name, b=0):
        if name not in self.dev:
            return None
        t = self.dev[name]
        if name == "info":
            return t.data_ptr() + 4 * b
        g = self.g[name]
        return t.data_ptr() + (g.off + b * g.stride) * t.element_size()

    def run(self, h, b0=0, nb=None):
        """the case's call on regressors b0 .. b0 + nb (default: all of them)"""
        from blr_amd import _abi

        c, g = self.c, self.g
        dt = c.np_dtype
        q = lambda name: self.ptr(name, b0)
        layout = _abi.LAYOUT_COLVECS if c.layout == "col" else _abi.LAYOUT_ROWVECS
        prior = dict(dense=_abi.PRIOR_DENSE, factor=_abi.PRIOR_UPPER_FACTOR, diag=_abi.PRIOR_DIAGONAL)[c.prior]
        noise = _abi.NOISE_DIAGONAL if c.noise == "diag" else _abi.NOISE_ISOTROPIC
        ldl = c.ldl if c.prior != "diag" else 1
        if c.entry == "sample_weights":
            rc = h.sample_weights(dt, _abi.MEM_DEVICE, c.D, c.S, prior, q("mw"), q("L"), ldl, q("Z1"), c.ldz1, q("W"), c.ldw)
        elif c.entry == "apply_weights":
            rc = h.apply_weights(dt, _abi.MEM_DEVICE, layout, c.D, c.N, c.S, q("X"), c.ldx, q("W"), c.ldw, q("Y"), c.ldy)
        elif c.entry == "rand":
            rc = h.rand(dt, _abi.MEM_DEVICE, layout, c.D, c.N, c.S, q("X"), c.ldx, noise, q("s"), prior, q("mw"), q("L"), ldl, q("Z1"),
                        c.ldz1, q("Z2"), c.ldz2, q("Y"), c.ldy)
        else:
            st = lambda name: g[name].stride if name in g else 0
            rc = h.rand_batched(dt, _abi.MEM_DEVICE, layout, c.B if nb is None else nb, c.D, c.N, c.S, q("X"), c.ldx, st("X"), noise,
                                q("s"), st("s"), prior, q("mw"), st("mw"), q("L"), ldl, st("L"), q("Z1"), c.ldz1, st("Z1"), q("Z2"),
                                c.ldz2, st("Z2"), q("W"), c.ldw, st("W"), q("Y"), c.ldy, st("Y"), q("info"))
        h.synchronize()
        return rc

    def fetch(self, name):
        import torch

        torch.cuda.synchronize()
        return self.dev[name].cpu().numpy()


def _execute(B, opt, c):
    h = B._abi.default_handle()
    for key, value in c.options:
        opt(key, value)
    call = Call(c)
    rc = call.run(h)
    # 1. status and route
    assert rc == 0
    good = [b for b in range(c.B) if not (c.bad and c.bad[0] == b)]
    if c.entry == "rand_batched":
        info = call.fetch("info")
        want = np.zeros(c.B, dtype=np.int32)
        if c.bad:
            want[c.bad[0]] = c.bad[1]
        assert np.array_equal(info, want), info
    route = h.get_stat("draw_route")
    assert route == c.route, (bin(route), bin(c.route))
    if c.chunks is not None:
        assert h.get_stat("last_chunks") == c.chunks
    # 2. nothing outside the logical output moved (a failed regressor's outputs are outside it); no NaN inside
    out = {}
    for name, g in call.g.items():
        if not g.out:
            continue
        buf = call.fetch(name)
        m = DP.logical_mask(g, good)
        assert np.all(buf[~m] == DP.SENTINEL), (name, int(np.sum(buf[~m] != DP.SENTINEL)))
        assert not np.any(np.isnan(buf[m])), name
        out[name] = buf
    return call, out, good


def _note_ratio(c, err, yard):
    if yard is None or yard == 0.0:
        return
    kernel = {DP.W_MFMA: "mfma", DP.W_MFMA | DP.W_UVEC: "mfma+uvec", DP.W_LARGE: "large", DP.W_NS1: "batched_ns1",
              DP.W_NS4: "batched_ns4"}[c.route & 63]
    r = err / yard
    print(f"ratio {c.id} {kernel} {c.dtype}: gpu {err:.3e} lapack {yard:.3e} ratio {r:.3f}")
    if r > RATIOS.get((kernel, c.dtype), (0.0, ""))[0]:
        RATIOS[(kernel, c.dtype)] = (r, c.id)


def _check_weights(c, p, b, W):
    """4. W of regressor b against mw + U^-1 Z from the same rounded inputs"""
    ref, bound, yard = DP.weights_tolerance(c, p, b)
    err = np.abs(W.astype(np.longdouble) - ref)
    worst = float(np.max(err))
    print(f"weights {c.id} b={b}: max error {worst:.3e}, bound {float(np.max(bound)):.3e}")
    _note_ratio(c, worst, yard)
    assert np.all(err <= bound), (c.id, b, worst, float(np.max(bound)), yard)


def _weights_slack(c, p, b, X):
    """the weights bound of regressor b propagated through |X|' (entry points that do not return W)"""
    ref, bound, _ = DP.weights_tolerance(c, p, b)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    return np.asarray(ref, dtype=np.float64), np.abs(X).T @ bound


def _check_projection(c, p, b, Y, W, slack=None):
    """3. Y of regressor b against the fp64 product of the same rounded inputs (W: the weights the library used, in fp64)"""
    X = DP.x_of(c, p, b)
    noise = DP.noise_term(c, p, b)
    ref = X.T @ W + noise
    bound = DP.projection_bound(c, X, W, noise) + (0.0 if slack is None else slack)
    err = np.abs(Y.astype(np.float64) - ref)
    print(f"projection {c.id} b={b}: max error {float(np.max(err)):.3e}, max error / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound), (c.id, b, float(np.max(err / np.maximum(bound, 1e-300))))


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("c", DP.BY_ENTRY["sample_weights"], ids=_ids(DP.BY_ENTRY["sample_weights"]))
def test_sample_weights_lattice(B, opt, c):
    call, out, _ = _execute(B, opt, c)
    _check_weights(c, call.p, 0, DP.unpack(out["W"], call.g["W"]))


@pytest.mark.parametrize("c", DP.BY_ENTRY["apply_weights"], ids=_ids(DP.BY_ENTRY["apply_weights"]))
def test_apply_weights_lattice(B, opt, c):
    call, out, _ = _execute(B, opt, c)
    _check_projection(c, call.p, 0, DP.unpack(out["Y"], call.g["Y"]), call.p["W"][0])


@pytest.mark.parametrize("c", DP.BY_ENTRY["rand"], ids=_ids(DP.BY_ENTRY["rand"]))
def test_rand_lattice(B, opt, c):
    call, out, _ = _execute(B, opt, c)
    # (no W output: the reference weights, and the weights bound through |X|')
    W_ref, slack = _weights_slack(c, call.p, 0, DP.x_of(c, call.p, 0))
    _check_projection(c, call.p, 0, DP.unpack(out["Y"], call.g["Y"]), W_ref, slack)


@pytest.mark.parametrize("c", DP.BY_ENTRY["rand_batched"], ids=_ids(DP.BY_ENTRY["rand_batched"]))
def test_rand_batched_lattice(B, opt, c):
    call, out, good = _execute(B, opt, c)
    p = call.p
    for b in good:
        W = DP.unpack(out["W"], call.g["W"], b).astype(np.float64) if c.want_W else None
        if W is not None:
            _check_weights(c, p, b, W)
        if c.N == 0:
            continue
        Y = DP.unpack(out["Y"], call.g["Y"], b)
        if W is not None:
            _check_projection(c, p, b, Y, W)
        else:
            W_ref, slack = _weights_slack(c, p, b, DP.x_of(c, p, b))
            _check_projection(c, p, b, Y, W_ref, slack)
    # 5. regressor b of the batch has the bits of a call on that regressor alone (blr_rand_batched.hpp's header)
    if c.B == 37 and not c.bad:
        h = B._abi.default_handle()
        single = Call(c, p)
        for b in (0, 17, 36):
            assert single.run(h, b0=b, nb=1) == 0
        for name in ("W", "Y"):
            if name not in out:
                continue
            one = single.fetch(name)
            g = call.g[name]
            assert np.all(one[~DP.logical_mask(g, (0, 17, 36))] == DP.SENTINEL)
            for b in (0, 17, 36):
                assert np.array_equal(DP.unpack(one, g, b).view(np.uint8), DP.unpack(out[name], g, b).view(np.uint8)), (name, b)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_uvec_loader_gives_the_bits_of_the_scalar_loader(B, opt, dt):
    """D = 128, factor prior: the 16-byte loader of U (aligned, ld a multiple of the vector), an ld that is not and a pointer one
    element off: the same arithmetic behind three loads, so the same bits"""
    trio = [c for c in DP.BY_ENTRY["sample_weights"] if c.group == f"uvec-{dt}"]
    assert [c.route for c in trio] == [DP.W_MFMA | DP.W_UVEC, DP.W_MFMA, DP.W_MFMA]
    Ws = []
    for c in trio:
        call, out, _ = _execute(B, opt, c)
        Ws.append(DP.unpack(out["W"], call.g["W"]))
    assert np.array_equal(Ws[0].view(np.uint8), Ws[1].view(np.uint8)) and np.array_equal(Ws[0].view(np.uint8), Ws[2].view(np.uint8))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_no_mfma_twins_agree_with_the_matrix_cores(B, opt, dt):
    """each NO_MFMA_PROJECT twin satisfies the projection bound itself (test_apply_weights_lattice); here: the two routes differ by
    no more than the sum of their bounds on the twins of the largest D"""
    D = max(c.D for c in DP.BY_ENTRY["apply_weights"] if c.dtype == dt)
    pairs = {}
    for c in DP.BY_ENTRY["apply_weights"]:
        if c.dtype == dt and c.D == D and c.seed_key:
            pairs.setdefault(c.seed_key, []).append(c)
    assert pairs
    for a, b in pairs.values():
        ya = DP.unpack(_execute(B, opt, a)[1]["Y"], DP.operands(a)["Y"]).astype(np.float64)
        call, out, _ = _execute(B, opt, b)
        B._abi.default_handle().set_option("NO_MFMA_PROJECT", None)  # (the next pair starts on the matrix cores again)
        yb = DP.unpack(out["Y"], call.g["Y"]).astype(np.float64)
        X, W = call.p["X"][0], call.p["W"][0]
        assert np.all(np.abs(ya - yb) <= 2 * DP.projection_bound(b, X, W, np.zeros((b.N, b.S))))


def test_zz_report_ratios(B):
    """prints the table of the module header (run the module with -s); the 4 x bound itself is asserted case by case above"""
    for (kernel, dt), (r, cid) in sorted(RATIOS.items()):
        print(f"largest gpu / lapack error: {kernel:12s} {dt}: {r:.3f} ({cid})")
