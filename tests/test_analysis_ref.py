"""CPU: tests/analysis_ref.py -- the numpy restatement of the reference's downsample and SAD scan that the GPU tests
compare with -- gives what the reference's compiled kernels give: on the stored results of tests/golden/analysis_ref.npz
everywhere, and on the kernels themselves (oracle/_ref/libschroorc_ref.so, driven in the reference's row schedule) where
they are built.  The minimum search and the window set-up are checked for the properties their C text states."""
import os

import numpy as np
import pytest

import analysis_ref as A
import oracle_lib as O

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analysis_ref.npz"))
needs_ref = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref is not built on this box")


@pytest.mark.parametrize("w,h", A.GOLDEN_SIZES)
def test_downsample_matches_the_stored_reference_results(w, h):
    assert np.array_equal(A.downsample(A.picture(w, h, 100 + w + 7 * h)), GOLDEN["down_random_%dx%d" % (w, h)])
    assert np.array_equal(A.downsample(A.checkerboard(w, h)), GOLDEN["down_checker_%dx%d" % (w, h)])


def test_scan_tables_match_the_stored_reference_results():
    cases = A.golden_scans()
    assert len(cases) == 3 * len(A.GOLDEN_BLOCKS)
    for n, (frame, ref, s, ext) in enumerate(cases):
        assert np.array_equal(A.do_scan(frame, ref, s), GOLDEN["scan_%02d" % n]), (n, s)


@needs_ref
@pytest.mark.parametrize("w,h", A.GOLDEN_SIZES + [(130, 70), (321, 241)])
def test_downsample_matches_the_compiled_reference_kernels(w, h):
    for src in (A.picture(w, h, 7 + w), A.checkerboard(w, h), np.full((h, w), 255, np.uint8)):
        assert np.array_equal(A.downsample(src), A.downsample_orc(src))


@needs_ref
def test_scan_tables_match_the_compiled_reference_kernels():
    for n, (frame, ref, s, ext) in enumerate(A.golden_scans()):
        assert np.array_equal(A.do_scan(frame, ref, s), A.do_scan_orc(frame, ref, s, ext)), (n, s)
    # the largest block and the widest window
    frame, ref = A.picture(96, 80, 1), A.picture(96, 80, 2)
    s = dict(x=16, y=8, block_width=64, block_height=64, dx=0, dy=0)
    s["ref_x"], s["ref_y"], s["scan_width"], s["scan_height"] = A.scan_setup(16, 8, 64, 64, 96, 80, 32, 0, 0, 6)
    assert np.array_equal(A.do_scan(frame, ref, s), A.do_scan_orc(frame, ref, s, 32))


def test_two_stage_rounding_differs_from_a_single_rounding():
    """The u8 intermediate row is part of the contract: a 2-D filter rounded once gives other values on a random picture."""
    src = A.picture(16, 16, 9).astype(np.int64)
    k = np.array([6, 26, 26, 6])
    p = np.pad(src, ((1, 2), (1, 2)), mode="edge")
    once = np.array([[(np.outer(k, k) * p[2 * i:2 * i + 4, 2 * j:2 * j + 4]).sum() + 2048 >> 12 for j in range(8)] for i in range(8)])
    assert not np.array_equal(once, A.downsample(src.astype(np.uint8)))


def test_edgeextend_is_a_coordinate_clamp():
    src = A.picture(5, 4, 3)
    e = A.edgeextend(src, 3)
    assert e.shape == (10, 11)
    for y in range(-3, 7):
        for x in range(-3, 8):
            assert e[y + 3, x + 3] == src[min(max(y, 0), 3), min(max(x, 0), 4)]
    assert np.array_equal(A.edgeextend(src, 0), src)


def test_empty_blocks_have_metric_zero():
    frame, ref = A.picture(16, 16, 1), A.picture(16, 16, 2)
    for bw, bh in ((0, 8), (8, 0), (-3, 8)):
        s = dict(x=4, y=4, block_width=bw, block_height=bh, ref_x=2, ref_y=2, scan_width=5, scan_height=4)
        assert not A.do_scan(frame, ref, s).any()


def test_get_min_keeps_the_callers_vector_on_ties_and_takes_the_first_strict_minimum():
    s = dict(x=10, y=10, ref_x=8, ref_y=7, scan_width=4, scan_height=5, gravity_x=-2, gravity_y=-3, dx=77, dy=-55)
    flat = np.full(20, 9, np.uint32)
    assert A.get_min(flat, s) == (77, -55, 9)
    m = flat.copy()
    m[[7, 13]] = 3              # i = 1, j = 2 and i = 2, j = 3: the first in i-outer order wins
    assert A.get_min(m, s) == (8 + 1 - 10, 7 + 2 - 10, 3)
    s2 = dict(s, gravity_x=8 + 2 - 10, gravity_y=7 + 3 - 10)       # the gravity position on the later minimum
    assert A.get_min(m, s2) == (77, -55, 3)


def test_rough_scan_marks_degenerate_scans_invalid():
    frame = A.picture(40, 24, 5)
    P = dict(x_num_blocks=8, y_num_blocks=8, xbsep_luma=8, ybsep_luma=8)
    mvs = A.rough_scan_nohint(frame, frame, P, 0, 4, 1)
    grid = mvs.reshape(8, 8)
    assert (mvs["flags"] == 1).all()
    assert grid["metric"][0, 0] == 0 and tuple(grid["v"][0, 0]) == (0, 0, 0, 0)
    # block column 7 starts at x = 56: 16 samples right of the picture, no position is left
    assert grid["metric"][0, 7] == A.METRIC_INVALID and grid["metric"][7, 0] == A.METRIC_INVALID
    # skipped blocks of a coarser level stay as schro_motion_field_set left them
    mvs2 = A.rough_scan_nohint(frame, frame, P, 1, 4, 0).reshape(8, 8)
    assert mvs2["metric"][1, 1] == 0 and mvs2["flags"][1, 1] == 1
