"""CPU: tests/hist_ref.py -- the restatement of schrohistogram.c the device histograms are compared with -- says what the
C text says: ilogx over every s16 value, the DC form's four prediction cases worked by hand, schro_divide3 beside a floor
division over everything the DC form can hand it, and the vectorised forms beside a scalar loop transcribed line by line."""
import numpy as np
import pytest

import hist_ref as H


def test_ilogx_over_every_s16_value():
    v = np.arange(-32768, 32768, dtype=np.int64)
    idx = H.ilogx(v)
    assert np.array_equal(idx[v >= 0], idx[(v <= 0) & (v > -32768)][::-1])      # a function of |v|
    mag = np.arange(0, 32769, dtype=np.int64)
    im = H.ilogx(mag)
    assert np.all(np.diff(im) >= 0) and im[0] == 0                              # monotone in |v|
    sizes = np.bincount(im[:32768])
    assert len(sizes) == H.BINS == 104
    assert sizes.tolist() == [1] * 16 + [1 << ((i >> 3) - 1) for i in range(16, 104)]
    assert sizes.tolist() == [H.ilogx_size(i) for i in range(104)]
    over = v[idx >= H.BINS]
    assert over.tolist() == [-32768] and idx[0] == 104                           # the only overflow, on index 104
    # the first value of each bin from 16 up: 8 + (i & 7) shifted by the octave (iexpx, schrohistogram.c:24-32)
    firsts = [int(np.flatnonzero(im == i)[0]) for i in range(104)]
    assert firsts == [i if i < 8 else (8 | (i & 7)) << ((i >> 3) - 1) for i in range(104)]


def test_dc_prediction_cases_by_hand():
    band = np.array([[10, 13, 7],
                     [4, -20, 100],
                     [-5, 6, 9]], np.int16)
    # (0,0): pred 0.  row 0: the left neighbour.  column 0: the upper neighbour.
    # (1,1): (4 + 13 + 10 + 1) = 28 -> 9; (1,2): (-20 + 7 + 13 + 1) = 1 -> 0; (2,1): (-5 + -20 + 4 + 1) = -20 -> -7 (floor);
    # (2,2): (6 + 100 + -20 + 1) = 87 -> 29
    want = np.array([[10 - 0, 13 - 10, 7 - 13],
                     [4 - 10, -20 - 9, 100 - 0],
                     [-5 - 4, 6 - -7, 9 - 29]])
    assert np.array_equal(H.dc_differences(band), want)
    assert H.divide3(np.array([28, 1, -20, 87])).tolist() == [9, 0, -7, 29]
    # skip 2 counts rows 0 and 2, and row 2's prediction comes from row 1 (row j - 1), not from row 0
    c = H.counts(band, skip=2, dc=True)
    assert c.sum() == 6 and sorted(np.repeat(np.arange(105), c).tolist()) == sorted(H.ilogx(want[[0, 2]].reshape(-1)).tolist())
    n, bins, ovf = H.histogram(band, skip=2, dc=True)
    assert n == 12 and bins.sum() == 12.0 and ovf == 0


def test_divide3_beside_floor_division():
    """The sum of three s16 neighbours + 1 lies in [-98303, 98302].  (a * 21845 + 10922) >> 16 with a = 3 k + r is
    k + ((21845 r + 10922 - k) >> 16): the floor wherever 0 <= 21845 r + 10922 - k < 65536 for the r at hand, i.e. on all
    of [-32769, 32768] (r = 0 binds above: k <= 10922; r = 2 below: k >= -10923); beyond it the reference's form is at
    most one off -- one low above, one high below -- and the checker and the device keep the reference's form."""
    a = np.arange(-98303, 98303, dtype=np.int64)
    got, floor = H.divide3(a), a // 3
    exact = got == floor
    assert exact[(a >= -32769) & (a <= 32768)].all()
    assert not exact[a == 32769][0] and not exact[a == -32770][0]
    assert np.all(np.abs(got - floor) <= 1)
    assert np.all(got[a > 32768] <= floor[a > 32768]) and np.all(got[a < -32769] >= floor[a < -32769])
    # the same numbers from the closed form above
    k, r = a // 3, a % 3
    assert np.array_equal(got, k + ((21845 * r + 10922 - k) >> 16))


def scalar_ilogx(x):
    # schrohistogram.c:11-22
    i = 0
    if x < 0:
        x = -x
    while x >= 2 << 3:
        x >>= 1
        i += 1
    return x + (i << 3)


def c_int(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def scalar_histogram(band, skip, dc):
    """schro_frame_data_generate_histogram / _dc_predict (x = y = 0) line by line, the bound on the index added"""
    h, w = band.shape
    bins, over, n = [0.0] * 104, 0, 0
    j = 0
    while j < h:
        line = band[j]
        prev_line = band[j - 1] if j > 0 else None
        for i in range(w):
            if dc:
                if j > 0:
                    if i > 0:
                        a = c_int(int(line[i - 1]) + int(prev_line[i]) + int(prev_line[i - 1]) + 1)
                        pred_value = c_int(a * 21845 + 10922) >> 16
                    else:
                        pred_value = int(prev_line[i])
                else:
                    pred_value = int(line[i - 1]) if i > 0 else 0
                value = c_int(int(line[i]) - pred_value)
            else:
                value = int(line[i])
            k = scalar_ilogx(value)
            if k < 104:
                bins[k] += 1
            else:
                over += 1
            n += 1
        j += skip
    return int(n * skip), [b * skip for b in bins], over * skip


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_vectorised_forms_equal_the_scalar_loop(dtype):
    rng = np.random.default_rng(31)
    for (h, w) in ((1, 1), (1, 7), (6, 1), (9, 17), (12, 5)):
        for skip in (1, 2, 4):
            for dc in (False, True):
                for spread in (20, 40000, 1 << 31):
                    lim = min(spread, 1 << (8 * np.dtype(dtype).itemsize - 1))
                    band = rng.integers(-lim, lim, (h, w)).astype(dtype)
                    n, bins, ovf = H.histogram(band, skip, dc)
                    wn, wbins, wovf = scalar_histogram(band, skip, dc)
                    assert (n, bins.tolist(), ovf) == (wn, wbins, wovf), (h, w, skip, dc, spread)
                    assert n == bins.sum() + ovf


def test_band_layout_and_skip():
    # positions and skips of a depth-3 transform (schro_subband_get_position; SCHRO_SUBBAND_SHIFT = position >> 2)
    assert [H.position(i) for i in range(10)] == [0, 1, 2, 3, 5, 6, 7, 9, 10, 11]
    assert [H.band_skip(i) for i in range(13)] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 4, 4, 4]
    # a 16 x 8 plane at depth 2: every sample belongs to exactly one sub-band
    plane = np.arange(128).reshape(8, 16)
    seen = np.concatenate([H.band_view(plane, 2, i).reshape(-1) for i in range(7)])
    assert sorted(seen.tolist()) == list(range(128))
    assert H.band_view(plane, 2, 0).tolist() == [[0, 1, 2, 3], [64, 65, 66, 67]]          # rows 0 and 4, the first 4 columns
    assert H.band_rect(16, 8, 2, 6, 32, 2) == (32 + 16, 64, 8, 4)      # HH of the finest level: row 1, column 8
    ns, bins, ovf = H.frame_histograms([plane.astype(np.int16)] * 3, 2, 1)
    assert ns.shape == (21,) and bins.shape == (21, 104) and ovf.shape == (21,)
    assert ns[:7].tolist() == [8, 8, 8, 8, 32, 32, 32]
