"""Without a device: every draw of tests/arith_dec_draws.py hits the trap it is meant to hit, the test writer's bytes decode
to the drawn values, and the counters a draw is meant to leave at 0 are 0."""
import numpy as np
import pytest

import arith_dec_draws as AD


@pytest.mark.parametrize("case", AD.draws(), ids=lambda c: c.name)
def test_draw_round_trip_and_witness(case):
    coeffs, quant, result = case.expected()
    for k in range(3):
        assert np.array_equal(quant[k], np.asarray(case.planes[k]).astype(case.dtype)), (case.name, k)
        assert np.array_equal(coeffs[k], case.stored[k]), (case.name, k)
    assert result["compat_quant_offset"] == case.compat_after and result["bytes_read"] == len(case.data)
    clean = dict(AD.CLEAN)
    if case.witness in (AD.witness_offsets,):
        del clean["clamped_quant"]
    assert all(result[k] == v for k, v in clean.items()), (case.name, result)
    case.witness(case)


def test_the_draws_cover_the_ground():
    draws = AD.draws()
    assert {c.dtype for c in draws} == {np.dtype(np.int16), np.dtype(np.int32)} and {c.is_intra for c in draws} == {0, 1}
    assert {tuple(c.sizes[1]) == tuple(c.sizes[0]) for c in draws} == {True, False}
    formats = {(c.sizes[0][0] // c.sizes[1][0], c.sizes[0][1] // c.sizes[1][1]) for c in draws}
    assert formats == {(1, 1), (2, 1), (2, 2)}                  # 4:4:4, 4:2:2, 4:2:0
    assert {c.depth for c in draws} >= {0, 1, 2, 6} and {c.mode for c in draws} == {0, 1} and {c.compat for c in draws} == {0, 1}


@pytest.mark.parametrize("case", AD.hostile(), ids=lambda c: c.name)
def test_hostile_cases_are_defined_and_short(case):
    coeffs, quant, result = case.expected()
    assert result["bins"] < 1 << 20
    if coeffs is not None:
        assert all((p != 0x5b).any() or p.size == 0 or not p.any() for p in coeffs)
