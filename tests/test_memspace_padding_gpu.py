"""Host staging against device pointers, with every output padded: for each entry point that takes a memspace and has outputs
with a leading dimension or a batch stride (the posterior itself: tests/test_gpu_parity.py
test_padded_leading_dimensions_and_shared_inputs), the same call is made with host arrays and with device pointers on one
handle.  Every output's ld and stride exceed their minimum and the gaps hold a sentinel byte pattern beforehand.  Afterwards
the payload of every output is bit-identical between the two memspaces and every gap byte still holds the sentinel: a host
call that copies an output back with the wrong extent, or that does not carry the caller's bytes into the staged buffer first,
fails one of the two.  Random draws are passed in (the Z arguments).

Shapes: B = 3 where batched, N = 37, S = 5, D = 5 and 130 (either side of the D > 128 router); blr_posterior_rff_* at D = 130,
D_in = 3 in fp32 (the basis inside the planes pass) and fp64 (materialised features)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N, S, G = 3, 37, 5, 4
SENTINEL = 0xA5


class Out:
    """A flat output array: B items of rows x cols (column-major, leading dimension ld) at `stride`, sentinel everywhere;
    `init` (B x rows x cols) seeds the payload of an array the call updates in place."""

    def __init__(self, dtype, rows, cols=1, ld=None, nb=1, stride=None, init=None):
        ld = rows if ld is None else ld
        one = (cols - 1) * ld + rows
        stride = one if stride is None else stride
        assert ld >= rows and stride >= one
        n = (nb - 1) * stride + one
        self.idx = (np.arange(nb)[:, None, None] * stride + np.arange(cols)[None, :, None] * ld + np.arange(rows)[None, None, :]).ravel()
        self.a = np.frombuffer(bytes([SENTINEL]) * (n * np.dtype(dtype).itemsize), dtype=dtype).copy()
        if init is not None:
            self.a[self.idx] = np.asarray(init, dtype=dtype).transpose(0, 2, 1).ravel() if np.ndim(init) == 3 else np.asarray(init, dtype=dtype).ravel()
        self.ld, self.stride = ld, stride

    def split(self, a):
        """(payload bytes, gap bytes) of a filled copy of the array"""
        item = a.dtype.itemsize
        by = a.view(np.uint8).reshape(-1, item)
        gap = np.ones(a.size, dtype=bool)
        gap[self.idx] = False
        return by[self.idx], by[gap]


def cm(m):
    """column-major flat copy of a matrix (or of a batch of matrices)"""
    m = np.asarray(m)
    return np.ascontiguousarray(np.swapaxes(m, -1, -2)).ravel()


def problem(dt, D, seed):
    rng = np.random.default_rng(seed)
    p = {}
    X = rng.standard_normal((B, D, N))
    p["X"] = cm(X).astype(dt)
    p["y"] = rng.standard_normal((B, N)).astype(dt).ravel()
    p["s"] = (0.5 + rng.random(B)).astype(dt)
    p["mw"] = rng.standard_normal((B, D)).astype(dt).ravel()
    p["Lw"] = (0.5 + rng.random((B, D))).astype(dt).ravel()  # diagonal prior precision
    p["Z1"] = rng.standard_normal((B, D * S)).astype(dt).ravel()
    p["Z2"] = rng.standard_normal((B, N * S)).astype(dt).ravel()
    p["Y"] = rng.standard_normal(N * S).astype(dt)
    p["W"] = rng.standard_normal(D * S).astype(dt)
    R = rng.standard_normal((N, N))
    p["Sy"] = cm(np.eye(N) + R @ R.T / N).astype(dt)
    # resident states that contain the N observations: T'T = I + X X' / s
    A = np.eye(D)[None] + np.einsum("bdn,ben->bde", X, X) / p["s"].astype(np.float64)[:, None, None]
    p["T"] = np.swapaxes(np.linalg.cholesky(A), -1, -2)  # (B, D, D) upper
    p["alpha"] = np.array([0.5, 1.0, 2.0, 4.0], dtype=dt)
    p["tau"] = np.array([2.0, 1.0, 0.5, 1.5], dtype=dt)
    p["Xin"] = rng.standard_normal(3 * N).astype(dt)
    p["Omega"] = rng.standard_normal(3 * D).astype(dt)
    p["phase"] = (2 * np.pi * rng.random(D)).astype(dt)
    return p


# Every case: (inputs by name, outputs by name, call(h, memspace, v) with v[name] = host array or device pointer)
def case_marginals(dt, D, p):
    outs = {"mean": Out(dt, N, nb=B, stride=N + 3), "var": Out(dt, N, nb=B, stride=N + 4), "info": Out(np.int32, B)}
    return ["X", "s", "mw", "Lw"], outs, lambda h, m, v: h.marginals_batched(
        dt, m, 0, B, D, N, v["X"], D, D * N, 0, v["s"], 1, 2, v["mw"], D, v["Lw"], D, D, v["mean"], N + 3, v["var"], N + 4, v["info"])


def case_logpdf_grad(dt, D, p):
    outs = {"logpdf": Out(np.float64, B), "dX": Out(dt, D, N, ld=D + 3, nb=B, stride=(D + 3) * N + 5),
            "dy": Out(dt, N, nb=B, stride=N + 3), "ds": Out(dt, N, nb=B, stride=N + 4), "dmw": Out(dt, D, nb=B, stride=D + 3),
            "mw_post": Out(dt, D, nb=B, stride=D + 2), "Ainv": Out(dt, D, D, ld=D + 3, nb=B, stride=(D + 3) * D + 5), "info": Out(np.int32, B)}
    return ["X", "y", "s", "mw", "Lw"], outs, lambda h, m, v: h.logpdf_grad_batched(
        dt, m, 0, B, D, N, v["X"], D, D * N, v["y"], N, 0, v["s"], 1, 2, v["mw"], D, v["Lw"], D, D, v["logpdf"], v["dX"], D + 3,
        (D + 3) * N + 5, v["dy"], N + 3, v["ds"], N + 4, v["dmw"], D + 3, v["mw_post"], D + 2, v["Ainv"], D + 3, (D + 3) * D + 5, v["info"])


def case_logpdf_multi(dt, D, p):
    outs = {"logpdf": Out(np.float64, S), "mw_post": Out(dt, D, S, ld=D + 3), "info": Out(np.int32, 1)}
    return ["X", "Y", "s", "mw", "Lw"], outs, lambda h, m, v: h.logpdf_multi(
        dt, m, 0, D, N, S, v["X"], D, v["Y"], N, 0, v["s"], 2, v["mw"], v["Lw"], D, v["logpdf"], v["mw_post"], D + 3, v["info"])


def case_sample_weights(dt, D, p):
    outs = {"Wout": Out(dt, D, S, ld=D + 3)}
    return ["mw", "Lw", "Z1"], outs, lambda h, m, v: h.sample_weights(dt, m, D, S, 2, v["mw"], v["Lw"], D, v["Z1"], D, v["Wout"], D + 3)


def case_apply_weights(dt, D, p):
    outs = {"Yout": Out(dt, N, S, ld=N + 3)}
    return ["X", "W"], outs, lambda h, m, v: h.apply_weights(dt, m, 0, D, N, S, v["X"], D, v["W"], D, v["Yout"], N + 3)


def case_rand(dt, D, p):
    outs = {"Yout": Out(dt, N, S, ld=N + 3)}
    return ["X", "s", "mw", "Lw", "Z1", "Z2"], outs, lambda h, m, v: h.rand(
        dt, m, 0, D, N, S, v["X"], D, 0, v["s"], 2, v["mw"], v["Lw"], D, v["Z1"], D, v["Z2"], N, v["Yout"], N + 3)


def case_rand_batched(dt, D, p):
    outs = {"Wout": Out(dt, D, S, ld=D + 3, nb=B, stride=(D + 3) * S + 5), "Yout": Out(dt, N, S, ld=N + 3, nb=B, stride=(N + 3) * S + 5),
            "info": Out(np.int32, B)}
    return ["X", "s", "mw", "Lw", "Z1", "Z2"], outs, lambda h, m, v: h.rand_batched(
        dt, m, 0, B, D, N, S, v["X"], D, D * N, 0, v["s"], 1, 2, v["mw"], D, v["Lw"], D, D, v["Z1"], D, D * S, v["Z2"], N, N * S,
        v["Wout"], D + 3, (D + 3) * S + 5, v["Yout"], N + 3, (N + 3) * S + 5, v["info"])


def case_mean_and_cov(dt, D, p):
    outs = {"mean": Out(dt, N), "C": Out(dt, N, N, ld=N + 3), "info": Out(np.int32, 1)}
    return ["X", "s", "mw", "Lw"], outs, lambda h, m, v: h.mean_and_cov(
        dt, m, 0, D, N, v["X"], D, 0, v["s"], 1, 2, v["mw"], v["Lw"], D, v["mean"], v["C"], N + 3, v["info"])


def case_posterior_dense_noise(dt, D, p):
    outs = {"mw_post": Out(dt, D), "T_post": Out(dt, D, D, ld=D + 3), "Lw_post": Out(dt, D, D, ld=D + 4), "logpdf": Out(np.float64, 1),
            "info": Out(np.int32, 1)}
    return ["X", "y", "Sy", "mw", "Lw"], outs, lambda h, m, v: h.posterior_dense_noise(
        dt, m, 0, D, N, v["X"], D, v["y"], v["Sy"], N, 2, v["mw"], v["Lw"], D, v["mw_post"], v["T_post"], D + 3, v["Lw_post"], D + 4,
        v["logpdf"], v["info"])


def case_rand_dense_noise(dt, D, p):
    outs = {"Yout": Out(dt, N, S, ld=N + 3)}
    return ["X", "Sy", "mw", "Lw", "Z1", "Z2"], outs, lambda h, m, v: h.rand_dense_noise(
        dt, m, 0, D, N, S, v["X"], D, v["Sy"], N, 2, v["mw"], v["Lw"], D, v["Z1"], D, v["Z2"], N, v["Yout"], N + 3)


def _factor_case(name, k):
    def case(dt, D, p):  # the state is updated in place: its payload goes in, the gaps hold the sentinel
        outs = {"mw_io": Out(dt, D, nb=B, stride=D + 3, init=p["mw"].reshape(B, D)),
                "T_io": Out(dt, D, D, ld=D + 3, nb=B, stride=(D + 3) * D + 5, init=p["T"]),
                "logpdf": Out(np.float64, B), "info": Out(np.int32, B)}
        return ["X", "y", "s"], outs, lambda h, m, v: getattr(h, name)(
            dt, m, 0, B, D, k, v["X"], D, D * N, v["y"], N, 0, v["s"], 1, v["mw_io"], D + 3, v["T_io"], D + 3, (D + 3) * D + 5, v["logpdf"],
            v["info"])
    return case


def case_loo(dt, D, p):
    outs = {"lm": Out(dt, N, nb=B, stride=N + 3), "lv": Out(dt, N, nb=B, stride=N + 4), "ll": Out(np.float64, N, nb=B, stride=N + 5),
            "total": Out(np.float64, B), "info": Out(np.int32, B)}
    return ["X", "y", "s", "mw", "Tin"], outs, lambda h, m, v: h.loo(
        dt, m, 0, B, D, N, v["X"], D, D * N, v["y"], N, 0, v["s"], 1, v["mw"], D, v["Tin"], D, D * D, v["lm"], N + 3, v["lv"], N + 4,
        v["ll"], N + 5, v["total"], v["info"])


def case_logpdf_grid(dt, D, p):
    outs = {"logpdf": Out(np.float64, G, nb=B, stride=G + 3), "best": Out(np.int64, B), "mw_best": Out(dt, D, nb=B, stride=D + 3),
            "T_best": Out(dt, D, D, ld=D + 3, nb=B, stride=(D + 3) * D + 5), "info": Out(np.int32, G, nb=B, stride=G + 2)}
    return ["X", "y", "s", "mw", "Lw", "alpha", "tau"], outs, lambda h, m, v: h.logpdf_grid(
        dt, m, 0, B, D, N, v["X"], D, D * N, v["y"], N, 0, v["s"], 1, 2, v["mw"], D, v["Lw"], D, D, G, v["alpha"], 0, v["tau"], 0,
        v["logpdf"], G + 3, v["best"], v["mw_best"], D + 3, v["T_best"], D + 3, (D + 3) * D + 5, v["info"], G + 2)


def case_rff_features(dt, D, p):
    outs = {"Phi": Out(dt, D, N, ld=D + 3)}
    return ["Xin", "Omega", "phase"], outs, lambda h, m, v: h.rff_features(
        dt, m, 3, D, N, v["Xin"], 3, v["Omega"], 3, v["phase"], 0.125, v["Phi"], D + 3)


def case_posterior_rff(dt, D, p):
    outs = {"mw_post": Out(dt, D), "T_post": Out(dt, D, D, ld=D + 3), "Lw_post": Out(dt, D, D, ld=D + 4), "logpdf": Out(np.float64, 1),
            "info": Out(np.int32, 1)}
    return ["Xin", "Omega", "phase", "y", "s", "mw", "Lw"], outs, lambda h, m, v: h.posterior_rff(
        dt, m, 3, D, N, v["Xin"], 3, v["Omega"], 3, v["phase"], 0.125, v["y"], 0, v["s"], 2, v["mw"], v["Lw"], D, v["mw_post"], v["T_post"],
        D + 3, v["Lw_post"], D + 4, v["logpdf"], v["info"])


CASES = {"marginals": case_marginals, "logpdf_grad": case_logpdf_grad, "logpdf_multi": case_logpdf_multi,
         "sample_weights": case_sample_weights, "apply_weights": case_apply_weights, "rand": case_rand, "rand_batched": case_rand_batched,
         "mean_and_cov": case_mean_and_cov, "posterior_dense_noise": case_posterior_dense_noise, "rand_dense_noise": case_rand_dense_noise,
         "update_factor": _factor_case("update_factor", 1), "downdate_factor": _factor_case("downdate_factor", 2), "loo": case_loo,
         "logpdf_grid": case_logpdf_grid, "rff_features": case_rff_features, "posterior_rff": case_posterior_rff}
# fp64 everywhere; fp32 as well where the code forks on the element type (logpdf_multi's planes route, the fused basis)
PARAMS = [(n, np.float64, D) for n in CASES if n != "posterior_rff" for D in (5, 130)]
PARAMS += [("logpdf_multi", np.float32, 130), ("posterior_rff", np.float32, 130), ("posterior_rff", np.float64, 130)]


@pytest.fixture(scope="module")
def handle():
    from blr_amd import _abi
    h = _abi.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(dt, D):
        key = (np.dtype(dt).name, D)
        if key not in cache:
            p = problem(dt, D, 20240 + D)
            p["Tin"] = cm(p["T"]).astype(dt)
            for a in p.values():
                a.setflags(write=False)
            cache[key] = p
        return cache[key]
    return get


@pytest.mark.parametrize("name,dt,D", PARAMS, ids=[f"{n}-{np.dtype(t).name}-D{D}" for n, t, D in PARAMS])
def test_host_and_device_memspace_agree_and_keep_the_gaps(handle, problems, name, dt, D):
    from blr_amd import _abi
    h = handle
    p = problems(dt, D)
    ins, outs, call = CASES[name](dt, D, p)
    # host pointers
    host = {k: o.a.copy() for k, o in outs.items()}
    call(h, _abi.MEM_HOST, {**{k: p[k] for k in ins}, **host})
    # device pointers, same handle
    ptrs = {}
    try:
        for k in ins:
            ptrs[k] = h.device_alloc(p[k].nbytes)
            h.memcpy_h2d(ptrs[k], p[k])
        for k, o in outs.items():
            ptrs[k] = h.device_alloc(o.a.nbytes)
            h.memcpy_h2d(ptrs[k], o.a)
        call(h, _abi.MEM_DEVICE, ptrs)
        h.synchronize()
        dev = {k: np.empty_like(o.a) for k, o in outs.items()}
        for k in outs:
            h.memcpy_d2h(dev[k], ptrs[k])
    finally:
        for q in ptrs.values():
            h.device_free(q)
    for k, o in outs.items():
        pay_h, gap_h = o.split(host[k])
        pay_d, gap_d = o.split(dev[k])
        assert (gap_h == SENTINEL).all(), f"{k}: the host-memspace call changed {int((gap_h != SENTINEL).sum())} gap bytes"
        assert (gap_d == SENTINEL).all(), f"{k}: the device-memspace call changed {int((gap_d != SENTINEL).sum())} gap bytes"
        assert np.array_equal(pay_h, pay_d), f"{k}: {int((pay_h != pay_d).any(axis=1).sum())} of {len(pay_h)} payload elements differ between the memspaces"
    if "info" in outs:  # the calls themselves succeeded: a status of the inputs, not of the staging
        assert not outs["info"].split(host["info"])[0].view(np.int32).any(), host["info"]
