"""The launch rule of marg_blocksub_kernel as tests/_marg_block_problems.py restates it: its arithmetic, checked without a GPU
before tests/test_marg_block_gpu.py asserts the stats of real calls against it."""
import os
import re

import numpy as np
import pytest

import _marg_block_problems as MB

F64, F32 = np.float64, np.float32


def test_the_constants_are_the_sources(repo_root):
    csrc = os.path.join(repo_root, "bayesianlinearregressors.jl_amd", "csrc")
    marg = open(os.path.join(csrc, "blr_marginals.hpp")).read()
    img = open(os.path.join(csrc, "blr_marg_image.hpp")).read()
    assert re.search(r"kMaxLds = 156 \* 1024;", marg) and MB.KMAX_LDS == 159744
    assert re.search(r"constexpr int kPB = 128;", img) and MB.KPB == 128
    assert re.search(r"NFRAG = 4 \* 36;", img) and re.search(r"IMG_ELEMS = NFRAG \* 64;", img) and MB.IMG_ELEMS == 9216
    assert "PAD = 32 / (int)sizeof(T)" in marg and "off_red(DP) + WAVES * RT * (int)sizeof(double)" in marg


def test_the_largest_tile_per_type():
    """fp32: D = 1152 takes 155 136 bytes; fp64: D = 512 (138 240); 640 columns of fp64 are 172 032 > 159 744 -- so 528 .. 640,
    the (float64, 576) row of test_large_d_marginals among them, run the tall sweep"""
    assert MB.lds_bytes(F32, 1152) == 155136 and MB.lds_bytes(F64, 512) == 138240 and MB.lds_bytes(F64, 640) == 172032
    assert MB.lds_bytes(F32, 1280) > MB.KMAX_LDS
    assert max(D for D in range(144, 4097, 16) if MB.qualifies(F32, D)) == 1152
    assert max(D for D in range(144, 4097, 16) if MB.qualifies(F64, D)) == 512
    assert not MB.qualifies(F64, 576) and not MB.qualifies(F64, 528) and not MB.qualifies(F32, 1168)
    # the 16-row tile of fp32 is never what decides: it is smaller than the 32-row tile at every width
    assert all(MB.lds_bytes(F32, DP, 16) < MB.lds_bytes(F32, DP, 32) for DP in range(256, 1153, 128))


def test_what_else_the_rule_asks_for():
    assert MB.expected_block_route(F32, 256, 100, 3, 256) == (16, 1, 0)
    for kw in (dict(layout="row"), dict(prior="diag"), dict(aligned=False)):
        assert MB.expected_block_route(F32, 256, 100, 3, 256, **kw) == (0, 0, 0)
    for D in (128, 130, 264):  # D <= 128, and widths that are no multiple of 16
        assert MB.expected_block_route(F64, D, 100, 3, 256) == (0, 0, 0)
    assert MB.expected_block_route(F64, 272, 70, 256, 256, prior="dense") == (32, None, None)


@pytest.mark.parametrize("cus", [256, 64, 304])
def test_small_tiles_boundary(cus):
    """fp32 takes 16-row tiles exactly while ceil(N / 32) B < cus; fp64 never"""
    for B in (1, 3, cus - 1):
        n_last = 32 * ((cus - 1) // B)  # the largest N with ceil(N / 32) B < cus
        assert MB.small_tiles(F32, n_last, B, cus) and not MB.small_tiles(F32, n_last + 1, B, cus)
        assert MB.expected_block_route(F32, 256, n_last, B, cus)[0] == 16
        assert MB.expected_block_route(F32, 256, n_last + 1, B, cus)[0] == 32
        assert MB.expected_block_route(F64, 256, n_last, B, cus)[0] == 32
    assert not MB.small_tiles(F32, 1, cus, cus) and MB.small_tiles(F32, 32, cus - 1, cus)


def test_the_cases_of_the_gpu_tests_at_256_cus():
    """what tests/test_marg_block_gpu.py expects on a whole MI355X (it asks the rule again with the device's own count)"""
    cus = 256
    assert MB.expected_block_route(F32, 256, 8200, 1, cus) == (32, 2, 0)  # the one second trip of the suite before this file
    for dt in (F32, F64):
        assert MB.expected_block_route(dt, 144, 72, cus, cus) == (32, 3, 1)
        assert MB.expected_block_route(dt, 144, 72, cus + 1, cus) == (32, 3, 0)
        assert [MB.expected_block_route(dt, 272, N, cus, cus)[1] for N in (32, 33, 64, 65, 97)] == [1, 2, 2, 3, 4]
    assert MB.expected_block_route(F32, 1152, 72, 1, cus) == (16, 1, 0)
    assert MB.expected_block_route(F64, 512, 72, 1, cus) == (32, 1, 0)
    # the batched cases of the older tests: none is renumbered
    for dt, D, N, B in ((F64, 256, 200, 5), (F32, 1024, 100, 9), (F64, 144, 70, 7), (F32, 144, 70, 7)):
        assert MB.expected_block_route(dt, D, N, B, cus)[2] == 0


def test_16_row_tiles_never_take_a_second_trip():
    """small_tiles needs ceil(N / 32) B < cus, and then ceil(N / 16) <= 2 ceil(N / 32) <= ceil(2 cus / B): grid.x = the tiles.  So the
    tile loop of marg_blocksub_kernel<float, 16> is single-trip by construction (a sweep, not the proof)."""
    seen = 0
    for cus in (8, 60, 64, 104, 256, 304):
        for B in list(range(1, 40)) + [cus // 2, cus - 1, cus, cus + 1]:
            for N in list(range(1, 200)) + [32 * k + e for k in range(7, 2 * cus, 5) for e in (-1, 0, 1)]:
                rt, walk, _ = MB.expected_block_route(F32, 256, N, B, cus)
                if rt == 16:
                    assert walk == 1, (cus, B, N)
                    seen += 1
                else:
                    assert rt == 32 and walk >= 1
    assert seen > 10000
