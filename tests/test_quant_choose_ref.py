"""CPU: tests/quant_choose_ref.py -- the restatement of the reference's estimate and choice code the device stage is
compared with -- says what the C text says: histograms small enough to work on paper, identities of get_range, the sign of
the lambda sweep read from the code, and a second formulation of the engines' sums."""
import math

import numpy as np
import pytest

import quant_choose_draws as D
import quant_choose_ref as R
import quant_ref as Q


def hist(**bins):
    b = np.zeros(R.BINS, np.float64)
    for k, v in bins.items():
        b[int(k[1:])] = v
    return b


def test_bin_geometry():
    assert [R.iexpx(i) for i in (0, 7, 8, 15, 16, 17, 24, 103, 104)] == [0, 7, 8, 15, 16, 18, 32, 30720, 32768]
    assert all(R.ilogx(R.iexpx(i)) == i and R.ilogx(R.iexpx(i + 1) - 1) == i for i in range(R.BINS))
    assert [R.ilogx_size(i) for i in range(R.BINS)] == [R.iexpx(i + 1) - R.iexpx(i) for i in range(R.BINS)]
    assert R.ilogx(R.RANGE_END) == 103


def test_get_range_by_hand():
    # one sample of |v| = 5: inside every range that starts at or below 5
    b = hist(b5=1.0)
    assert [R.get_range(b, s, 32000) for s in (0, 5, 6, 31999, 32000, 40000)] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    # two bins straddling a start: bin 16 holds |v| 16, 17 and bin 17 holds 18, 19.  From 17 on: half of bin 16, all of
    # bin 17; from 19 on: half of bin 17
    b = hist(b16=6.0, b17=10.0)
    assert R.get_range(b, 17, 32000) == 0.5 * 6.0 + 10.0
    assert R.get_range(b, 19, 32000) == 0.5 * 10.0
    assert R.get_range(b, 16, 32000) == 16.0 and R.get_range(b, 20, 32000) == 0.0
    # start and end in one bin (bin 103: 30720 .. 32767, 2048 values): (32768 - 31000 - 768) / 2048 of it
    b = hist(b103=2048.0)
    assert R.get_range(b, 31000, 32000) == 1000.0
    # the range ends INSIDE bin 103: 768 / 2048 of it is outside
    assert R.get_range(b, 0, 32000) == 2048.0 - 768.0


def test_get_range_of_everything_is_the_sum_but_for_bin_103():
    rng = np.random.default_rng(1)
    for skip in (1, 4, 32):
        c = rng.integers(0, 1 << 20, R.BINS).astype(np.uint32)
        b = R.scaled_bins(c, skip)
        assert R.get_range(b, 0, 32000) == b.sum() - 0.375 * b[103]
        b[103] = 0
        assert R.get_range(b, 0, 32000) == b.sum()


@pytest.mark.parametrize("name", ["d3", "d1_edges"])
def test_ranges_are_monotone_and_exact(name):
    """bin[i] never rises with i (the starts rise), and every partial sum is exact: exact rational arithmetic agrees"""
    from fractions import Fraction
    pic = D.get(name)
    for c in range(3):
        for i, b in enumerate(D.bins_of(pic)[c]):
            for j in (0, 1, 7, 22, 41, 59):
                starts = [R.range_start(j, k) for k in range(R.N_RANGES)]
                assert starts == sorted(starts)
                r = [R.get_range(b, s, 32000) for s in starts]
                assert all(x >= y for x, y in zip(r, r[1:])), (c, i, j, r)
                for s, got in zip(starts, r):
                    if s >= 32000:
                        assert got == 0.0
                        continue
                    k = R.ilogx(s)
                    want = Fraction(R.iexpx(k + 1) - s, R.ilogx_size(k)) * Fraction(float(b[k]))
                    want += sum(Fraction(float(v)) for v in b[k + 1:]) - Fraction(768, 2048) * Fraction(float(b[103]))
                    assert Fraction(got) == want


def test_noarith_estimate_by_hand():
    # one sample of |v| = 5 at index 0 (factor 4: starts (4 (2^i - 1) + 3) / 4 = 0, 1, 3, 7, 15, ...): bins 1, 1, 1, 0 ...
    b = hist(b5=1.0)
    x = 1.0 - math.exp(-12.5)
    want = (x * 1.0 + (1 - x) * 1.0) + 1.0 + 2 * 1.0 + 2 * 1.0
    assert R.estimate_entropy(b, 0, True) == want
    # all mass in bin 0: bin[1 ..] = 0, the proportion is 0, exp (-0) = 1: nothing to code
    assert R.estimate_entropy(hist(b0=1234.0), 0, True) == 0.0
    assert R.estimate_entropy(hist(b0=1234.0), 30, True) == 0.0
    # nothing sampled: 0 / 0
    assert math.isnan(R.estimate_entropy(hist(), 0, True))
    # high indices: the starts from i = 2 on lie past 32000 (start >= end: an empty range), only bin[0] and bin[1] are left
    hi = [j for j in range(60) if R.range_start(j, 2) >= 32000]
    assert hi and hi[-1] == 59 and R.range_start(59, 1) < 32000
    b = hist(b90=100.0, b103=2048.0)    # bin 90 (|v| from 10240) lies below index 59's first start
    b0, b1 = 1380.0, R.get_range(b, R.range_start(59, 1), 32000)
    assert 0 < b1 < b0
    x = 1.0 - math.exp(-0.5 * 25 * (b1 / b0))
    assert R.estimate_entropy(b, 59, True) == x * b0 + (1 - x) * b1 + b1 + 2 * b1


def test_arith_estimate_by_hand():
    one = np.full(R.BINS, 2.0)
    zero = np.full(R.BINS, 6.0)
    b = hist(b0=3.0, b5=1.0)            # bins: 4, 1, 1, 0 ...
    h = lambda p: -(p * math.log(p) + (1 - p) * math.log(1 - p)) * R.INV_LOG_2
    want = 0.0
    want += 1.0                         # the sign bits
    want += h(1.0 / 4.0) * 4.0          # entropy (bin[1], bin[0])
    want += 0.0                         # entropy (1, 1): x >= 1
    want += 0.0                         # entropy (0, 1): x <= 0
    want += 0.0 + 0.0                   # totals of 0
    want += 0.0                         # post5 = 0 over a total of 0
    want += h(8.0 / 32.0) * 32.0        # ones = 4 * 2, zeros = 4 * 6
    assert R.estimate_entropy(b, 0, False, one, zero) == want
    assert R.estimate_entropy(hist(), 0, False, one, zero) == 0.0      # no NaN on this branch
    assert R.utils_entropy(1.0, 0.0) == 0.0 and R.probability_to_entropy(0.5) == pytest.approx(1.0, abs=1e-15)


def test_apply_table_order():
    rng = np.random.default_rng(2)
    b = R.scaled_bins(rng.integers(0, 1 << 30, R.BINS), 2)
    t = rng.uniform(0, 1e9, (5, R.BINS))
    assert [R.apply_table(b, t[k]) for k in range(5)] == R.apply_tables(b, t).tolist()
    # the order matters: the sum from the other end differs somewhere
    assert any(R.apply_table(b, t[k]) != R.apply_table(b[::-1], t[k][::-1]) for k in range(5))


def test_error_table_is_table_generate_over_the_quantiser():
    t = D.error_table()
    assert t.shape == (60, 104) and np.all(t >= 0) and np.all(t[0] == 0)          # index 0 is the identity
    for j, i in ((9, 3), (23, 40), (59, 103)):
        f, o = Q.quant_factor(j), Q.quant_offset(j, True)
        want = R.table_generate(lambda x: float(abs(Q.schro_dequantise(Q.schro_quantise(x, f, o), f, o) - x)) ** 4.0)[i] \
            if i < 41 else None
        if want is not None:
            assert t[j, i] == want
    # an index that quantises everything to zero: the error is x ** 4 itself
    assert t[59, 8] == 8.0 ** 4


def test_pick_quant_first_minimum_and_nan():
    ent, err = np.zeros(60), np.zeros(60)
    assert R.pick_quant(ent, err, 1.0) == 0                     # all equal: the first
    ent[:] = 5.0
    ent[7] = ent[9] = 1.0
    assert R.pick_quant(ent, err, 1.0) == 7
    ent[3] = float("nan")
    assert R.pick_quant(ent, err, 1.0) == 7                     # a NaN at j > 0 never wins
    ent[0] = float("nan")
    assert R.pick_quant(ent, err, 1.0) == 0                     # a NaN at j = 0 is never displaced
    ent[0], ent[1] = float("inf"), float("inf")
    ent[2:] = float("inf")
    assert R.pick_quant(ent, err, 1.0) == 0


def test_subband_lambda_order():
    w = np.full(19, 3.0)
    s = (10.0, 0.1, 0.5)
    assert R.subband_lambda(7.0, 0, 0, w, s, True) == 7.0 * 10.0 / 9.0
    assert R.subband_lambda(7.0, 1, 0, w, s, True) == 7.0 * 10.0 * 0.1 / 9.0
    assert R.subband_lambda(7.0, 2, 3, w, s, True) == 7.0 * 0.1 * 0.5 / 9.0    # sub-band 3 is HH
    assert R.subband_lambda(7.0, 2, 3, w, s, False) == 7.0 * 0.1 / 9.0         # no diagonal scale on the error path
    assert R.subband_lambda(7.0, 0, 2, w, s, True) == 7.0 / 9.0
    assert [R.position(i) & 3 for i in range(7)] == [0, 1, 2, 3, 1, 2, 3]


@pytest.mark.parametrize("name", ["d3", "d3_arith"])
def test_lambda_sweep(name):
    """x = entropy + lambda * error: a larger lambda weighs the error more, so the chosen error never rises and the chosen
    entropy never falls as lambda rises -- per sub-band (an exchange argument on two minimisers), hence for the sums."""
    pic = D.get(name)
    ent, err = D.estimates(name)
    ev = R.Evaluator(ent, err, pic["depth"], pic["weight"], pic["scales"])
    lams = [10.0 ** e for e in range(-10, 11)]
    es = [ev.lambda_to_entropy(l) for l in lams]
    rs = [ev.lambda_to_error(l) for l in lams]
    tol = 1e-12
    assert all(b >= a * (1 - tol) for a, b in zip(es, es[1:])) and es[-1] > es[0]
    assert all(b <= a * (1 + tol) for a, b in zip(rs, rs[1:])) and rs[-1] < rs[0]


def test_raster_and_per_subband_sums_agree():
    """lambda_to_entropy as the C loops run it, beside a formulation per sub-band: a matrix of x, numpy's argmin (first
    minimum) and the chosen entries added in (component, sub-band) order"""
    pic = D.get("d3")
    ent, err = D.estimates("d3")
    nb = R.n_bands(3)
    for lam in (1e-3, 1.0, 250.0):
        for on_error in (False, True):
            ev = R.Evaluator(ent, err, 3, pic["weight"], pic["scales"])
            got = ev.lambda_to_error(lam) if on_error else ev.lambda_to_entropy(lam)
            total, idx = 0.0, np.zeros((3, nb), np.int32)
            for c in range(3):
                for i in range(nb):
                    sl = R.subband_lambda(lam, c, i, pic["weight"], pic["scales"], not on_error)
                    x = ent[c, i] + sl * err[c, i]
                    idx[c, i] = int(np.argmin(x))
                    total += float((err if on_error else ent)[c, i, idx[c, i]])
            assert got == total and np.array_equal(ev.indices, idx)


def test_estimated_residual_bits_truncates_every_addition():
    ce = np.array([[0.9, 0.9, 0.9], [1.5, 1.6, 0.0], [0.0, 0.0, 2.99]])
    assert R.estimated_residual_bits(ce) == 4   # 0, 0, 0, 1, 2, 2, 2, 2, 4: the three 0.9 never add up
    assert R.estimated_residual_bits(np.array([[10.7], [0.7], [0.7]])) == 10
