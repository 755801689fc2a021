"""The table of tests/test_large_d_lattice_gpu.py without a device: the table reaches what it says it reaches (a shrunken table
would still "pass" on the GPU), its route rule is the real planner's (tools/large_plan_dump --stdin on every row), and its inputs
are well-posed -- fp32 LAPACK's direct form alone, fed to the yardstick the kernels are held to, passes on every fp32 row."""
import json
import os
import subprocess

import numpy as np
import pytest

from _large_d_problems import (DS, LARGE_LATTICE, MEANS, N_SHORT_CHUNK, NOISES, NS, OPTION_SETS, PLANES_ROUTES, PRIORS, ROUTES, TILE_ROUTES_F32,
                               XKINDS, check_oracle, expected_plan, expected_route, large_problem, mixes_ring_and_stage_tiles, planes_chunks,
                               ragged_rows, reference_alone, x_of_image)
from blr_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KEYS = {"id", "dtype", "D", "N", "xkind", "noise", "prior", "prior_mean", "nb", "options", "route"}


def _by_route(route):
    return [r for r in LARGE_LATTICE if r["route"] == route]


def test_rows_are_well_formed():
    ids = [r["id"] for r in LARGE_LATTICE]
    assert len(set(ids)) == len(ids)
    assert len(LARGE_LATTICE) <= 400
    for r in LARGE_LATTICE:
        assert KEYS <= set(r)
        assert r["D"] in DS and (r["N"] in NS or r["N"] in N_SHORT_CHUNK.values()) and r["N"] <= 2800
        assert r["xkind"] in XKINDS and r["noise"] in NOISES and r["prior"] in PRIORS and r["prior_mean"] in MEANS and r["nb"] in (1, 3)
        assert r["options"] is OPTION_SETS[r["optset"]]
        assert r["route"] == expected_route(r["dtype"], r["D"], r["N"], r["xkind"], r["options"])
    assert {r["optset"] for r in LARGE_LATTICE} == set(OPTION_SETS)


@pytest.mark.parametrize("route", ROUTES)
def test_every_route_meets_every_axis(route):
    rows = _by_route(route)
    assert rows
    # the loaders the route can serve: the planes kernels ColVecs of any alignment, <float, true> aligned ColVecs only
    serves = {"gram_tile_kernel<float, true>": {"col16"}}.get(route, {"col16", "colodd", "colbase1"} if route in PLANES_ROUTES else set(XKINDS))
    assert {r["xkind"] for r in rows} == serves
    assert {r["noise"] for r in rows} == set(NOISES)
    assert {r["prior"] for r in rows} == set(PRIORS)
    assert {r["prior_mean"] for r in rows} == set(MEANS)
    assert {r["D"] for r in rows} == set(DS) and set(NS) <= {r["N"] for r in rows}
    assert {(r["D"], r["N"]) for r in rows} >= {(D, N) for D in DS for N in NS}  # every (route, shape edge) pair
    assert any(r["nb"] == 3 and r["D"] in (129, 200) for r in rows)            # a group at a ragged D
    assert any(r["route"] == route for r in ragged_rows())


@pytest.mark.parametrize("route", sorted(PLANES_ROUTES))
def test_planes_routes_have_a_short_or_empty_last_chunk_and_a_zero_k_block(route):
    NP = PLANES_ROUTES[route]
    plans = [(r, expected_plan(r["dtype"], r["D"], r["N"], r["xkind"], r["options"])) for r in _by_route(route)]
    assert all(p["NP"] == NP and p["planes"] for _, p in plans)
    ragged = [(r, planes_chunks(p)) for r, p in plans if p["NKB"] % p["nbchunks"] != 0]
    assert ragged and all(r["N"] == N_SHORT_CHUNK[NP] for r, _ in ragged)
    for _, chunks in ragged:
        assert sum(chunks) == max(1, -(-N_SHORT_CHUNK[NP] // 16) + (NP == 2)) and chunks[-1] == 0 and max(chunks) == 2
        assert (1 in chunks) == (NP == 3)  # NP = 3: a short chunk in front of the empty ones
    if NP == 2:  # the stage padding adds a whole zero k-block: 16 NKB - N >= 16
        assert any(16 * p["NKB"] - r["N"] >= 16 for r, p in plans if r["N"] == N_SHORT_CHUNK[2])
        assert any(16 * p["NKB"] - r["N"] >= 16 for r, p in plans if r["N"] < 64)
    # below N_SHORT_CHUNK every chunk is one k-block: the derivation next to the number
    assert all(set(planes_chunks(p)) == {1} for r, p in plans if r["N"] <= 512)


@pytest.mark.parametrize("route", TILE_ROUTES_F32)
def test_tile_routes_mix_ring_and_stage_tiles_in_one_launch(route):
    rows = [r for r in _by_route(route) if mixes_ring_and_stage_tiles(r)]
    assert {r["D"] for r in rows} == {129, 200}
    # ... and runs without the ring loop on the same shapes: register staging, NO_GRAM_RING
    assert any(r["xkind"] != "col16" for r in _by_route("gram_tile_kernel<float>"))
    assert any(r["options"].get("NO_GRAM_RING") == "1" and r["xkind"] == "col16" for r in _by_route("gram_tile_kernel<float>"))


def test_fp64_rows_stage_full_and_partial_tiles_through_every_loader():
    """gram_tile_kernel<double> has no ring loop; its forks are the staging (LDS-DMA full / bounded pieces / registers) and the ragged block"""
    rows = _by_route("gram_tile_kernel<double>")
    assert any(r["xkind"] == "col16" and r["D"] in (129, 200) and r["N"] >= 16 for r in rows)
    assert all(r["dtype"] == np.float64 for r in rows)


# ---- the route rule against the planner ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc in this image")
    exe = str(tmp_path_factory.mktemp("large_plan_lattice") / "large_plan_dump")
    r = subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-o", exe,
                        os.path.join(ROOT, "tools", "large_plan_dump.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = []
    for i, row in enumerate(LARGE_LATTICE):
        q_layout = "row" if row["xkind"] == "row" else "col"
        aligned = 1 if row["xkind"] in ("col16", "row") else 0
        opts = " ".join(f"{k}={v}" for k, v in row["options"].items())
        lines.append(f"r{i} {np.dtype(row['dtype']).itemsize} {row['D']} {row['N']} {q_layout} {row['noise']} {row['prior']} {aligned} {row['nb']} {opts}")
    r = subprocess.run([exe, "--stdin"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plans = [json.loads(line) for line in r.stdout.splitlines()]
    assert [p["case"] for p in plans] == [f"r{i}" for i in range(len(LARGE_LATTICE))]
    return plans


def test_expected_route_is_the_planners(planner):
    for row, got in zip(LARGE_LATTICE, planner):
        assert "error" not in got, (row["id"], got)
        want = expected_plan(row["dtype"], row["D"], row["N"], row["xkind"], row["options"])
        assert got["route"] == want["route"] == row["route"], (row["id"], got["route"], want["route"])
        for k in ("planes", "bf3", "x_ring"):
            assert bool(got[k]) == want[k], (row["id"], k, got[k], want[k])
        for k in ("DP", "NC", "NKB", "nbchunks"):
            assert got[k] == want[k], (row["id"], k, got[k], want[k])
        if want["planes"]:
            assert got["NP"] == want["NP"] and bool(got["planes4"]) == (row["route"] == "gram_planes4_kernel")
        assert got["G"] == row["nb"]  # the group shares the launches (the workspace bound is far away)


# ---- the inputs are well-posed ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", LARGE_LATTICE, ids=[r["id"] for r in LARGE_LATTICE])
def test_the_image_holds_the_oracles_numbers_and_the_reference_alone_passes_the_yardstick(row):
    q = large_problem(row)
    item = np.dtype(row["dtype"]).itemsize
    aligned = (q["xoff"] * item) % 16 == 0 and (q["ldx"] * item) % 16 == 0
    assert (aligned == (row["xkind"] == "col16") or row["xkind"] == "row") and (q["strideX"] * item) % 16 == 0
    assert (q["layout"] == _abi.LAYOUT_ROWVECS) == (row["xkind"] == "row")
    if row["xkind"] == "colodd":
        assert q["ldx"] > row["D"]
    for b in range(q["nb"]):
        assert np.array_equal(x_of_image(q, b), q["Xd"][:, b * row["N"]:(b + 1) * row["N"]])
    assert np.count_nonzero(~np.isnan(q["ximg"])) == q["nb"] * row["D"] * row["N"]  # everything else is poison
    assert np.all(q["mw"] == 0) == (row["prior_mean"] == "zero")
    if row["dtype"] == np.float32:
        for b in range(q["nb"]):
            check_oracle(q, b, reference_alone(q, b), what=row["id"])
