"""The plan of the large-D update (csrc/blr_large_plan.hpp: route, split factors, workspace layout, group size) needs no device:
tools/large_plan_dump.cpp prints it for a fixed table of shapes on a 256-CU part, and every field must equal
tests/golden/large_plan.json.  That table was recorded from the driver as it was BEFORE the planner was split out of it (its
planning prologue lifted verbatim into a program with a stand-in handle), so it pins the plans themselves, not the new code's
opinion of them.  Layout invariants are checked on top: ascending 256-aligned offsets, `per` = end of the last buffer, and a
group never beyond the workspace bound."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "large_plan.json")))
BUFFERS = ["abar", "w", "xp", "gp", "bp", "mu", "qs", "r", "wv", "q", "l", "m", "sc"]  # in workspace order


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc in this image")
    exe = str(tmp_path_factory.mktemp("large_plan") / "large_plan_dump")
    r = subprocess.run([HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-o", exe,
                        os.path.join(ROOT, "tools", "large_plan_dump.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines()]
    assert [row["case"] for row in rows] == [g["case"] for g in GOLDEN]
    return {row["case"]: row for row in rows}


@pytest.mark.parametrize("want", GOLDEN, ids=[g["case"] for g in GOLDEN])
def test_plan_is_the_recorded_one(plans, want):
    got = plans[want["case"]]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (want["case"], k, got[k], want[k])


@pytest.mark.parametrize("case", [g["case"] for g in GOLDEN if "error" not in g])
def test_layout_invariants(plans, case):
    p = plans[case]
    offs = [p["offsets"][b] for b in BUFFERS]
    assert sorted(p["offsets"]) == sorted(BUFFERS)
    assert offs[0] == 0 and offs == sorted(offs), offs
    assert all(o % 256 == 0 for o in offs) and p["per"] % 256 == 0
    assert p["per"] == p["offsets"]["sc"] + 256  # the 64 scratch bytes, rounded up, are the last buffer
    assert p["G"] >= 1
    if p["G"] > 1:
        assert p["G"] * p["per"] <= p["cap"]


def test_table_reaches_the_branches():
    """the golden table itself: the cases the planner's branches need are there (a table that lost one would still 'pass')"""
    by = {g["case"]: g for g in GOLDEN}
    assert by["f32_nobf16x3_D1024_N16384"]["nsplit_diag"] > 0 and by["f32_nobf16x3_D1024_N16384"]["nlong"] == 0  # single-round diagonal split
    assert by["f32_noplanes_D2048_N16384"]["nlong"] > 0  # plan_gram_rounds
    assert by["f32_noplanes_D2048_N16384_again"] == dict(by["f32_noplanes_D2048_N16384"], case="f32_noplanes_D2048_N16384_again")  # the cache
    for c in ("f32_noplanes_D1024_N16384_unaligned", "f32_noplanes_D1024_N16384_rowvecs"):
        assert by[c]["nsplit_diag"] == 0 and not by[c]["bf3"] and by[c]["route"] == "gram_tile_kernel<float>"
    assert by["f32_default_D1024_N16384"]["planes4"] and by["f32_default_D1024_N16384"]["route"] == "gram_planes4_kernel"
    assert by["f32_planes8_D1024_N16384"]["route"] == "gram_planes_kernel<2>"
    assert by["f32_nofp16planes_D1024_N16385"]["NP"] == 3
    assert by["f32_rff_Din4_D512_N4096"]["rff"] and by["f32_rff_Din16_D512_N4096"]["rff"]
    assert by["f32_multi_S3_D1024_N16384"]["NCA"] == by["f32_multi_S3_D1024_N16384"]["NC"] + 1
    assert by["f32_noplanes_splits_15_11"]["nsplit_diag"] == 11 and by["f32_noplanes_splits_8_4_64"]["nlong"] == 64
    assert by["f32_dense_prior_D384_N200"]["offsets"]["xp"] > by["f32_dense_prior_D384_N200"]["offsets"]["w"]
    assert by["f32_diag_noise_D384_N200"]["offsets"]["q"] > by["f32_diag_noise_D384_N200"]["offsets"]["wv"]
    assert by["f32_factor_prior_D384_N200"]["bslots"] == by["f32_factor_prior_D384_N200"]["nsplit"] + 1
    assert by["f32_D200_N300"]["DP"] == 256
    assert not by["f32_D256_N0"]["planes"]
    assert by["f32_G128_D256_N512"]["G"] == 128
    clamped = by["f32_G128_D256_N512_ws12"]
    assert 1 < clamped["G"] < 128 and clamped["nsplit"] != by["f32_G128_D256_N512"]["nsplit"]  # clamp and re-plan
    assert sum("error" in g for g in GOLDEN) == 4
