"""CPU: tests/picture_stats_ref.py -- the numpy restatement the GPU picture-statistics tests compare with -- against what
pins it: the reference's compiled orc_sum_u8 / orc_sum_s16 / orc_sum_square_diff_u8 (oracle/_ref/libschroorc_ref.so) where
that library is built, hand-derived values everywhere, and the plain scalar transcription of the low-pass's C loops."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import picture_stats_cases as K
import picture_stats_ref as R

needs_ref = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref is not built on this box")


def rows_for_sums():
    rng = np.random.default_rng(7)
    rows = [np.zeros(1, np.uint8), np.full(33025, 255, np.uint8)]
    rows += [rng.integers(0, 256, n, dtype=np.uint8) for n in (1, 3, 63, 64, 65, 257, 4099)]
    return rows


@needs_ref
def test_row_sums_match_the_compiled_reference_kernels():
    L = O.reforc()
    rng = np.random.default_rng(8)
    out = C.c_int32()
    for a in rows_for_sums():
        L.orc_sum_u8(C.byref(out), a.ctypes.data_as(C.c_void_p), C.c_int(a.size))
        assert out.value == R.orc_sum_u8(a)
        b = rng.integers(0, 256, a.size, dtype=np.uint8)
        for other in (b, np.zeros_like(a), 255 - a):
            other = np.ascontiguousarray(other)
            L.orc_sum_square_diff_u8(C.byref(out), a.ctypes.data_as(C.c_void_p), other.ctypes.data_as(C.c_void_p), C.c_int(a.size))
            assert out.value == R.orc_sum_square_diff_u8(a, other)
        s = rng.integers(-32768, 32768, a.size).astype(np.int16)
        for t in (s, np.full(a.size, -32768, np.int16), np.full(a.size, 32767, np.int16)):
            L.orc_sum_s16(C.byref(out), t.ctypes.data_as(C.c_void_p), C.c_int(t.size))
            assert out.value == R.orc_sum_s16(t)


def test_sums_match_hand_derived_values():
    assert R.orc_sum_u8([1, 2, 3, 250]) == 256
    assert R.orc_sum_s16([-32768, -32768, 5]) == -65531
    # (0 - 255)^2 + (255 - 0)^2 + (10 - 7)^2 = 65025 + 65025 + 9: the 16-bit mullw keeps 65025 whole
    assert R.orc_sum_square_diff_u8([0, 255, 10], [255, 0, 7]) == 130059
    a = np.full((3, 5), 255, np.uint8)
    assert R.plane_sums(a) == (3825, 0)
    assert R.plane_sums(a, np.zeros_like(a)) == (3825, 15 * 65025)
    assert R.plane_sums(np.array([[-3, 4]], np.int16)) == (1, 0)
    assert R.average_luma(a) == 255.0
    assert R.mean_squared_error([a], [np.zeros_like(a)]) == [65025.0]
    # a row at the largest width whose int32 row sum cannot wrap: 33025 * 65025 < 2^31 <= 33026 * 65025
    assert 33025 * 65025 < 2 ** 31 <= 33026 * 65025
    row = np.full(33025, 255, np.uint8)
    assert R.orc_sum_square_diff_u8(row, np.zeros_like(row)) == 33025 * 65025


def test_the_int_accumulator_of_the_average_wraps_on_a_bright_4k_plane():
    w, h = 4096, 2057
    plane = np.full((h, w), 255, np.uint8)
    exact, _ = R.plane_sums(plane)
    assert exact == 2148495360 and exact >= 2 ** 31
    got = R.average_luma(plane)
    assert got < 0
    assert got == (2148495360 - 2 ** 32) / (w * h)
    assert R.average_luma_of_sum(exact, w, h) == got
    # one row fewer still fits
    assert R.average_luma(plane[:-1]) == 255.0 and 4096 * 2056 * 255 < 2 ** 31


def ulp_distance(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


@pytest.mark.parametrize("sigma", K.SIGMAS)
def test_coefficients_sum_to_one(sigma):
    c = R.generate_coeff(sigma)
    assert all(np.isfinite(c))
    assert ulp_distance(((c[0] + c[1]) + c[2]) + c[3], 1.0) <= 4


def test_lowpass_vectorised_matches_the_scalar_transcription_on_every_geometry_of_the_gpu_test():
    for (w, h, dtype, kind, hs, vs, seed) in K.lowpass_cases():
        a = K.lowpass_input(kind, w, h, dtype, seed)
        hc, vc = R.generate_coeff(hs), R.generate_coeff(vs)
        got, bad = R.lowpass2(a, hc, vc)
        want, bad_want = R.lowpass2_scalar(a, hc, vc)
        assert got.dtype == a.dtype and np.array_equal(got, want), (w, h, dtype, kind, hs, vs)
        assert bad == bad_want, (w, h, dtype, kind, hs, vs)


def step_row(n=64):
    a = np.zeros((1, n), np.uint8)
    a[:, n // 2:] = 255
    return a


def row_extremes(row, c):
    """The smallest and largest unrounded x of the two row passes over one u8 row."""
    x = row.astype(np.float64)
    lo, hi = 0.0, 0.0
    for order in (range(x.size), range(x.size - 1, -1, -1)):
        s = [x[order[0]]] * 3
        for i in order:
            v = c[0] * x[i] + c[1] * s[0] + c[2] * s[1] + c[3] * s[2]
            s = [v, s[0], s[1]]
            lo, hi = min(lo, v), max(hi, v)
            x[i] = R.to_sample(np.array([v]), np.uint8)[0][0]
    return round(lo), round(hi)


def test_a_step_at_sigma_0_375_leaves_the_range():
    """The filter sharpens below sigma 0.7 (q < 0): a 0 -> 255 step leaves the u8 range.

    The restatement, which agrees with the scalar transcription of the C loops, gives for ONE step 6 samples per row (x
    from -100 to 361 for 0 -> 255, from -106 to 355 for 255 -> 0) at every width from 8 to 256 and every position but the
    two columns next to a border (5, 3), and 6 per step for steps 16 columns apart (18 for 0, 255, 0, 255 in blocks of 16:
    x from -106 to 361).  A figure of 17 per row has been quoted for this step; no row of one step gives it, nor does
    rounding, clamping or not rounding between the two row passes.  The counts below are asserted exactly."""
    c = R.generate_coeff(0.375)
    assert c[1] < 0 and c[0] > 1         # the sharpening regime
    ident = [1.0, 0.0, 0.0, 0.0]
    up = step_row()
    assert R.lowpass2(up, c, ident)[1] == 6 and R.lowpass2_scalar(up, c, ident)[1] == 6
    assert row_extremes(up[0], c) == (-100, 361)
    down = 255 - up
    assert R.lowpass2(down, c, ident)[1] == 6
    assert row_extremes(down[0], c) == (-106, 355)
    blocks = np.repeat(np.array([[0, 255, 0, 255]], np.uint8), 16, axis=1)
    assert R.lowpass2(blocks, c, ident)[1] == 18 and R.lowpass2_scalar(blocks, c, ident)[1] == 18
    assert row_extremes(blocks[0], c) == (-106, 361)
    # four identical rows: the column passes see constant columns and add nothing
    rows = np.repeat(up, 4, axis=0)
    assert R.lowpass2(rows, c, c)[1] == 4 * 6


@pytest.mark.parametrize("sigma", [s for s in K.SIGMAS if s >= 0.75])
def test_a_step_at_sigma_0_75_and_up_stays_in_range(sigma):
    c = R.generate_coeff(sigma)
    a = K.steps(64, 8, np.uint8)
    assert R.lowpass2(a, c, c)[1] == 0


def test_to_sample_keeps_the_low_bits_of_the_int32_value():
    x = np.array([-106.4, 362.0, 255.5, 254.5, -0.5, 1e12, -1e12, np.nan, np.inf])
    d, bad = R.to_sample(x, np.uint8)
    assert list(d) == [(-106) & 255, 362 & 255, 0, 254, 0, 0, 0, 0, 0] and bad == 7
    d, bad = R.to_sample(np.array([32768.0, -32769.0, 40000.2, -32768.0, 1e12]), np.int16)
    assert list(d) == [-32768, 32767, 40000 - 65536, -32768, 0] and bad == 4
    assert R._rint_store(362.0, np.uint8) == (362 & 255, 1) and R._rint_store(2.5, np.uint8) == (2, 0)
    assert R._rint_store(float("nan"), np.int16) == (0, 1)


@pytest.mark.parametrize("w,h", K.SSIM_SIZES)
def test_ssim_of_a_picture_with_itself_is_exactly_one(w, h):
    a, b = K.ssim_pair("same", w, h, 3)
    values, _ = R.ssim_map(a, b)
    assert np.all(values == 1.0)
    assert R.mssim(values) == 1.0


def test_ssim_falls_with_noise_and_the_score_takes_both_branches():
    a, b = K.ssim_pair("noisy", 130, 67, 3)
    _, c = K.ssim_pair("unrelated", 130, 67, 3)
    near, far = R.mssim(R.ssim_map(a, b)[0]), R.mssim(R.ssim_map(a, c)[0])
    assert far < near < 1.0
    assert R.mssim_bound(R.ssim_map(a, b)[0]) < 1e-11
    assert R.scene_change_score(16.005, a, b) == 1.0 and R.scene_change_score(3.0, a, b) == 1.0
    luma = 100.0 - 16.0
    assert R.scene_change_score(100.0, a, b) == R.mean_squared_error([a], [b])[0] / (luma * luma)


def test_the_hipass_carries_the_offset_of_the_s16_conversion_by_hand():
    """schro_frame_dup16 converts u8 to s16 with orc_offsetconvert_s16_u8 (u8 - 128) before the low-pass is subtracted:
    a_hipass = (a - 128) - a_lowpass lies in -383 .. 127, and the products leave the s16 range, so the clamp bites."""
    a, low = np.array([[0, 255, 200, 128, 130]], np.uint8), np.array([[255, 0, 200, 0, 1]], np.uint8)
    ah = R.hipass(a, low)
    assert ah.tolist() == [[-383, 127, -128, 0, 1]]
    bh = R.hipass(low, a)               # 255 - 128 - 0, 0 - 128 - 255, ...
    assert bh.tolist() == [[127, -383, -128, -256, -257]]
    # -383 * 127 = -48641 -> -32768; 383^2 = 146689 -> 32767; 128^2 = 16384 stays; 0; 1 * -257
    assert R.multiply_s16(ah, bh).tolist() == [[-32768, -32768, 16384, 0, -257]]
    assert R.multiply_s16(ah, ah).tolist() == [[32767, 16129, 16384, 0, 1]]
    # a flat picture: the low-pass is the picture, every hipass sample is -128 and every product 16384 -- the value of a flat
    # 200 against a flat 100 is (2 * 200 * 100 + c1) (2 * 16384 + c2) / ((200^2 + 100^2 + c1) (2 * 16384 + c2))
    c1, c2 = (0.01 * 255) * (0.01 * 255), (0.03 * 255) * (0.03 * 255)
    values, counts = R.ssim_map(np.full((4, 300), 200, np.uint8), np.full((4, 300), 100, np.uint8))
    assert counts == [0] * 5
    assert np.all(values == (40000 + c1) * (32768 + c2) / ((50000 + c1) * (32768 + c2)))


@needs_ref
def test_the_hipass_matches_the_compiled_conversion_and_subtraction():
    L = O.reforc()
    rng = np.random.default_rng(11)
    a, low = rng.integers(0, 256, 777, dtype=np.uint8), rng.integers(0, 256, 777, dtype=np.uint8)
    a[:4], low[:4] = (0, 255, 0, 255), (255, 0, 0, 255)
    d = np.zeros(777, np.int16)
    L.orc_offsetconvert_s16_u8(d.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), C.c_int(777))
    assert np.array_equal(d, a.astype(np.int16) - 128)
    L.orc_subtract_s16_u8(d.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), low.ctypes.data_as(C.c_void_p), C.c_int(777))
    assert np.array_equal(d, R.hipass(a[None], low[None])[0])
