"""The Python front of the equal-count held-out predictives (loo, kfold, kfold_large, cross_validate, loo_columns, kfold_columns,
their ``_map`` forms and the five resident methods) says to the library exactly what it said before it was folded into one
fit-then-score pipeline: every public function runs under the shared recorder (tests/_recorder.py), and its normalised transcript
-- entry points, arguments, pointer tokens with sizes and content hashes, copies back -- and its result (hash, shape, dtype and
memory order of every field, or the exception's type, message and ``index``) must equal tests/heldout_front_transcript.json.

That file was recorded with ``record(parent module)``: `run_cases` of this module, unchanged, against the regressor.py of the
commit named in its header, loaded beside the current one.  The code under test never produces its own expectation."""
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from blr_amd import _abi
from blr_amd import regressor as R

from _recorder import Recorder, digest

RECORDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "heldout_front_transcript.json")
D, N, S, NB = 6, 5, 3, 4   # four equal problems; fold size 2: three folds, the last one short; fold size 3 on the large route


def _prior(M, rng, d, kind, dt):
    A = rng.standard_normal((d, d))
    if kind == "diag":
        return M.Diagonal(np.exp(0.1 * rng.standard_normal(d)).astype(dt))
    if kind == "dense":
        return (A @ A.T + d * np.eye(d)).astype(dt)
    return M.PDMat((np.triu(A, 1) + np.diag(1.0 + np.abs(np.diag(A)))).astype(dt))


def _problem(M, seed, d=D, n=N, s=S, layout="col", noise="scalar", prior="diag", dt=np.float64, ydt=None, rff=False, ylen=None):
    """One finite regressor with a vector target y and a matrix target Y, everything drawn from ``seed``."""
    rng = np.random.default_rng(seed)
    f = M.BayesianLinearRegressor(rng.standard_normal(d).astype(dt), _prior(M, rng, d, prior, dt))
    din = 2 if rff else d
    if rff:
        f = M.BasisFunctionRegressor(f, M.RandomFourierFeatures(rng.standard_normal((din, d)).astype(dt), rng.standard_normal(d).astype(dt)))
    X = rng.standard_normal((din, n)).astype(dt)
    x = M.ColVecs(np.asfortranarray(X)) if layout == "col" else M.RowVecs(np.ascontiguousarray(X.T))
    Sy = {"scalar": 0.5, "diag": M.Diagonal(np.exp(rng.standard_normal(n)).astype(dt)), "dense": np.eye(n) + 0.1}[noise]
    rows = n if ylen is None else ylen
    y = rng.standard_normal(rows).astype(ydt or dt)
    Y = rng.standard_normal((rows, s)).astype(ydt or dt)
    return SimpleNamespace(f=f, x=x, Sy=Sy, fx=f(x, Sy), y=y, Y=Y, n=n)


def _perm(p):
    return np.random.default_rng(99).permutation(p.n)


def _resident(M, p):
    return M.ResidentPosterior(p.f)


def _resident_columns(M, p):
    return M.ResidentColumnsPosterior(p.f, S=p.Y.shape[1] if p.Y.ndim == 2 and p.Y.shape[1] else S)


def _targets(ps, o, name):
    return [getattr(p, name) for p in ps[:len(ps) - o.drop]]


# entry point -> (set-up or None, call(M, problems, state, o)); o: F (fold size), FL (large fold size), K (n_folds), perm, drop (targets left out),
# digests (False: compare a result's shapes, dtypes and memory order only)
ENTRIES = {
    "loo": (None, lambda M, ps, st, o: M.loo(ps[0].fx, ps[0].y)),
    "loo_map": (None, lambda M, ps, st, o: M.loo_map([p.fx for p in ps], _targets(ps, o, "y"))),
    "kfold": (None, lambda M, ps, st, o: M.kfold(ps[0].fx, ps[0].y, o.F, o.perm)),
    "kfold_map": (None, lambda M, ps, st, o: M.kfold_map([p.fx for p in ps], _targets(ps, o, "y"), o.F)),
    "kfold_large": (None, lambda M, ps, st, o: M.kfold_large(ps[0].fx, ps[0].y, o.FL, o.perm)),
    "kfold_large_map": (None, lambda M, ps, st, o: M.kfold_large_map([p.fx for p in ps], _targets(ps, o, "y"), o.FL)),
    "cross_validate": (None, lambda M, ps, st, o: M.cross_validate(ps[0].fx, ps[0].y, o.K, o.perm)),
    "loo_columns": (None, lambda M, ps, st, o: M.loo_columns(ps[0].fx, ps[0].Y)),
    "loo_columns_map": (None, lambda M, ps, st, o: M.loo_columns_map([p.fx for p in ps], _targets(ps, o, "Y"))),
    "kfold_columns": (None, lambda M, ps, st, o: M.kfold_columns(ps[0].fx, ps[0].Y, o.F, o.perm)),
    "kfold_columns_map": (None, lambda M, ps, st, o: M.kfold_columns_map([p.fx for p in ps], _targets(ps, o, "Y"), o.F)),
    "resident.loo": (_resident, lambda M, ps, st, o: st.loo(ps[0].x, ps[0].Sy, ps[0].y)),
    "resident.kfold": (_resident, lambda M, ps, st, o: st.kfold(ps[0].x, ps[0].Sy, ps[0].y, o.F)),
    "resident.kfold_large": (_resident, lambda M, ps, st, o: st.kfold_large(ps[0].x, ps[0].Sy, ps[0].y, o.FL)),
    "resident_columns.loo": (_resident_columns, lambda M, ps, st, o: st.loo(ps[0].x, ps[0].Sy, ps[0].Y)),
    "resident_columns.kfold": (_resident_columns, lambda M, ps, st, o: st.kfold(ps[0].x, ps[0].Sy, ps[0].Y, o.F)),
}
MAPS = [e for e in ENTRIES if e.endswith("_map")]
PERM = ["kfold", "kfold_large", "cross_validate", "kfold_columns"]
SMALL_FOLDS = ["kfold", "kfold_map", "kfold_columns", "kfold_columns_map", "resident.kfold", "resident_columns.kfold"]
LARGE = ["kfold_large", "kfold_large_map", "resident.kfold_large"]
FIT = {"loo_columns_map": "fit", "kfold_columns_map": "fit"}                       # name of the fit in Recorder.calls, else "posterior"
SCORE = {"loo_map": "loo", "kfold_map": "kfold", "kfold_large_map": "kfold_large", "loo_columns_map": "loo_multi",
         "kfold_columns_map": "kfold_multi", "resident.loo": "loo", "resident.kfold": "kfold", "resident.kfold_large": "kfold_large",
         "resident_columns.loo": "loo_multi", "resident_columns.kfold": "kfold_multi"}


def cases():
    """-> [(id, entry point, problems(M) -> list, options, fail)]; ids starting with "refuse/" must leave the transcript empty"""
    out = []

    def add(cid, entries, problems, fail=None, **o):
        opts = SimpleNamespace(**dict(dict(F=2, FL=3, K=3, perm=None, drop=0, digests=True), **o))
        for e in entries:
            out.append((f"{cid}/{e}", e, problems, opts, fail(e) if callable(fail) else fail))

    def same(**kw):
        return lambda M: [_problem(M, 10 + b, **kw) for b in range(NB)]

    for layout in ("col", "row"):
        for noise in ("scalar", "diag"):
            for prior in ("diag", "dense", "pdmat"):
                add(f"{layout}-{noise}-{prior}", ENTRIES, same(layout=layout, noise=noise, prior=prior))
        add(f"perm-{layout}", PERM, same(layout=layout, noise="diag"), perm=_perm)
    add("cv-large", ["cross_validate"], same(n=70), K=1)                          # F = 70 > 64: kfold_large
    add("cv-large-perm", ["cross_validate"], same(n=70, noise="diag"), K=1, perm=_perm)
    add("f32", ENTRIES, same(dt=np.float32))
    add("one-f64", ENTRIES, lambda M: [_problem(M, 10 + b, dt=np.float32, ydt=np.float64 if b in (0, 2) else None) for b in range(NB)])
    add("map-f64-later", MAPS, lambda M: [_problem(M, 10 + b, dt=np.float32, ydt=np.float64 if b == 2 else None) for b in range(NB)])
    add("pdmat-with-dense", MAPS, lambda M: [_problem(M, 10 + b, prior=("pdmat", "dense")[b % 2]) for b in range(NB)])
    add("mixed-shapes", MAPS, lambda M: [_problem(M, 20 + b, n=n, s=s) for b, (n, s) in enumerate(((5, 3), (4, 3), (5, 2)))])
    add("mixed-layouts", MAPS, lambda M: [_problem(M, 20 + b, layout=("col", "row")[b % 2]) for b in range(NB)])
    add("mixed-noise", MAPS, lambda M: [_problem(M, 20 + b, noise=("scalar", "diag")[b % 2]) for b in range(NB)])
    add("rff-in-map", MAPS, lambda M: [_problem(M, 30 + b, rff=(b == 1)) for b in range(NB)])
    add("rff", ENTRIES, same(rff=True))
    add("fold-past-n", ["kfold", "kfold_large", "kfold_columns", "resident.kfold", "resident.kfold_large", "resident_columns.kfold"],
        same(), F=64, FL=1000)
    add("n0", ENTRIES, same(n=0))
    uncalled = ["loo_columns", "loo_columns_map", "kfold_columns", "kfold_columns_map"]
    add("d0", [e for e in ENTRIES if e not in uncalled], same(d=0))
    add("d0", uncalled, same(d=0), digests=False)     # the empty record without a call: N x S entries that nobody wrote
    add("s0", ["loo_columns", "loo_columns_map", "kfold_columns", "kfold_columns_map", "resident_columns.loo", "resident_columns.kfold"],
        same(s=0))
    add("empty-map", MAPS, lambda M: [])
    # failures: PosDefException(3) with index 2 from the fit (then no scoring call), from the scoring call, and one by one
    add("fail-fit", MAPS, same(), fail=lambda e: (FIT.get(e, "posterior"), 0, 2, 3))
    add("fail-score", MAPS, same(), fail=lambda e: (SCORE[e], 0, 2, 3))
    mixed = lambda M: [_problem(M, 20 + b, n=n, s=s) for b, (n, s) in enumerate(((5, 3), (4, 3), (5, 2), (5, 3)))]  # noqa: E731
    add("fail-fit-one-by-one", MAPS, mixed, fail=lambda e: (FIT.get(e, "posterior"), 2, 0, 3))
    add("fail-score-one-by-one", MAPS, mixed, fail=lambda e: (SCORE[e], 2, 0, 3))
    add("fail-score", [e for e in ENTRIES if e.startswith("resident")], same(), fail=lambda e: (SCORE[e], 0, 0, 3))
    # refusals: nothing reaches the library
    add("refuse/dense-noise", ENTRIES, same(noise="dense"))
    add("refuse/dense-noise-later", MAPS, lambda M: [_problem(M, 10 + b, noise="dense" if b == 3 else "scalar") for b in range(NB)])
    add("refuse/length", ENTRIES, same(ylen=N + 1))
    add("refuse/length-later", MAPS, lambda M: [_problem(M, 10 + b, ylen=N - 1 if b == 3 else None) for b in range(NB)])
    add("refuse/perm-short", PERM, same(), perm=lambda p: np.arange(p.n - 1))
    add("refuse/perm-repeats", PERM, same(), perm=lambda p: np.zeros(p.n, dtype=int))
    for F in (0, 65, 2.5):
        add(f"refuse/fold-size-{F}", SMALL_FOLDS, same(), F=F)
    for F in (0, 2.5):
        add(f"refuse/fold-size-{F}", LARGE, same(), FL=F)
        add(f"refuse/n-folds-{F}", ["cross_validate"], same(), K=F)
    add("refuse/d129", LARGE + ["kfold_columns", "kfold_columns_map", "resident_columns.kfold"], same(d=129, prior="pdmat"))
    add("refuse/folds-1025", LARGE, same(d=2, n=1025), FL=1)
    add("refuse/unequal-lists", MAPS, same(), drop=1)
    return out


def _field(v, digests):
    if isinstance(v, np.ndarray):
        return [digest(v) if digests else None, list(v.shape), v.dtype.name, bool(v.flags.c_contiguous), bool(v.flags.f_contiguous)]
    return [type(v).__name__, repr(v)]


def _result(r, digests):
    if isinstance(r, list):
        return [_result(k, digests) for k in r]
    return [type(r).__name__, [_field(v, digests) for v in r]]


def run_cases(M):
    """Every case against the regressor module ``M`` -> {id: {"calls", "transcript" (hash), "result", "leaked", "handle_lookups"}}, and the full
    transcripts beside it for reading.  The handle is replaced the way the routing tests replace it."""
    saved = (M._handle, _abi.default_handle)
    out, full = {}, {}
    try:
        for cid, entry, problems, o, fail in cases():
            rec = Recorder()
            lookups = []
            M._handle = _abi.default_handle = lambda rec=rec, lookups=lookups: lookups.append(1) or rec
            setup, call = ENTRIES[entry]
            ps = problems(M)
            opts = SimpleNamespace(**vars(o))
            if callable(opts.perm):
                opts.perm = opts.perm(ps[0])
            try:
                state = setup(M, ps[0]) if setup else None
            except Exception as e:  # noqa: BLE001 -- a state that cannot be built is a result too
                out[cid] = {"setup": [type(e).__name__, str(e)]}
                continue
            rec.events.clear()
            rec.calls.clear()
            lookups.clear()
            before = set(rec.bufs)
            rec.fail = fail
            try:
                result = _result(call(M, ps, state, opts), o.digests)
            except Exception as e:  # noqa: BLE001
                result = ["raise", type(e).__name__, str(e), getattr(e, "index", None)]
            text = json.dumps(rec.transcript(), sort_keys=True)
            out[cid] = {"calls": [k for k, _ in rec.calls], "transcript": hashlib.sha1(text.encode()).hexdigest()[:16], "result": result,
                        "leaked": len(set(rec.bufs) - before), "handle_lookups": len(lookups)}
            full[cid] = rec.transcript()
    finally:
        M._handle, _abi.default_handle = saved
    return out, full


def record(M, commit, path=RECORDING):
    """Write the recording; ``M`` is the parent commit's regressor.py loaded as a module of this package."""
    out, _ = run_cases(M)
    with open(path, "w") as fh:
        json.dump({"recorded_at": commit, "what": "tests/test_heldout_front_cpu.py run_cases() against that commit's regressor.py",
                   "cases": out}, fh, indent=0, sort_keys=True)
        fh.write("\n")


@pytest.fixture(scope="module")
def runs():
    return run_cases(R)


@pytest.fixture(scope="module")
def recording():
    with open(RECORDING) as fh:
        return json.load(fh)


def test_the_recording_covers_every_case(recording):
    assert len(recording["recorded_at"]) == 40
    assert sorted(recording["cases"]) == sorted(cid for cid, *_ in cases())


@pytest.mark.parametrize("cid", [c[0] for c in cases()])
def test_transcript_and_result_equal_the_recording(runs, recording, cid):
    got, want = runs[0][cid], recording["cases"][cid]
    assert got == want, (got, want, runs[1].get(cid))
    if "setup" not in got:
        assert got["leaked"] == 0          # no temporary outlives the call; the resident state is from before it
    if cid.startswith("refuse/"):
        assert got["calls"] == [] and runs[1][cid] == [] and got["result"][0] == "raise" and got["handle_lookups"] == 0


def test_failures_name_the_problem_and_skip_the_scoring_call(runs):
    for cid, entry, _, _, fail in cases():
        if not cid.startswith("fail-") or not entry.endswith("_map"):
            continue
        got = runs[0][cid]
        assert got["result"][:2] == ["raise", "PosDefException"] and got["result"][3] == 2, (cid, got)
        if cid.startswith("fail-fit/"):
            assert got["calls"] == [fail[0]], (cid, got)
