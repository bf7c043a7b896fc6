"""CPU: the restatement of the sub-pel refinement (tests/subpel_ref.py) reads the planes the oracle builds, and the named
cases of tests/subpel_cases.py exercise what they are there for."""
import numpy as np
import pytest

import oracle_lib as O
import rough_hint_cases as RH
import subpel_cases as K
import subpel_ref as R


@pytest.mark.parametrize("w,h,ext", [(20, 18, 8), (17, 21, 32), (33, 12, 4)])
def test_planes_with_aprons_are_the_oracles(w, h, ext):
    pic = RH.texture(w, h, 5)
    planes = R.up_planes(pic, ext)
    up = O.UpComp(pic, ext=ext)
    for i in range(4):
        want = np.array([[up.get(i, x, y) for x in range(-ext, w + ext)] for y in range(-ext, h + ext)], np.uint8)
        assert np.array_equal(planes[i], want), i


def test_a_raw_read_in_the_aprons_is_the_clamped_half_pel_sample():
    """What the tiled image of the device holds in its apron columns, and what the kernel's row clamp gives."""
    w, h, ext = 24, 19, 16
    pic = RH.texture(w, h, 6)
    planes = R.up_planes(pic, ext)
    for Y in range(-2 * ext, 2 * (h + ext)):
        for X in range(-2 * ext, 2 * (w + ext)):
            Xc, Yc = min(max(X, 0), 2 * w - 2), min(max(Y, 0), 2 * h - 2)
            got = planes[(X & 1) | ((Y & 1) << 1)][(Y >> 1) + ext, (X >> 1) + ext]
            assert got == planes[(Xc & 1) | ((Yc & 1) << 1)][(Yc >> 1) + ext, (Xc >> 1) + ext], (X, Y)


def test_a_read_outside_the_aprons_asserts():
    up = R.UpFrame(RH.texture(24, 19, 6), 8)
    up.raw(-16, -16, 8, 8)
    with pytest.raises(AssertionError, match="leaves the aprons"):
        up.raw(-18, 0, 8, 8)
    with pytest.raises(AssertionError, match="leaves the aprons"):
        up.raw(2 * 24, 0, 9, 8)


def test_estimate_sint():
    assert [R.estimate_sint(v) for v in (0, 1, -1, 2, 3, -3, 4, 7, 8, -100)] == [1, 4, 4, 4, 6, 6, 6, 8, 8, 14]


def test_the_issue_s_pair_separates_the_two_roundings():
    assert R._score(27, 0.1, 2557, False) > R._score(25, 0.1, 2577, False)
    assert R._score(27, 0.1, 2557, True) == R._score(25, 0.1, 2577, True)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case_exercises_its_point(name):
    K.expected(name)                    # (asserts the case's `want`)


def test_every_direction_wins_somewhere_and_so_does_none():
    wins = np.sum([K.expected(n)[2]["wins"] for n in K.DIRECTION_CASES], axis=0)
    assert (wins > 0).all(), wins


def test_all_positions_occur():
    p3 = set().union(*[K.expected(n)[2].get("positions3", set()) for n in K.CASES if K.CASES[n]["prec"] == 3])
    assert p3 == K.POSITIONS[3] and len(p3) == 12       # (every position a candidate can have: tests/subpel_cases.py says why not 16)
    p2 = set().union(*[K.expected(n)[2].get("positions2", set()) for n in K.CASES if K.CASES[n]["prec"] == 2])
    assert p2 == K.POSITIONS[2] and len(p2) == 3


def test_lambda_0_and_10_start_from_the_same_pictures():
    assert K.CASES["lambda_0"]["seed"] == K.CASES["lambda_10"]["seed"]
    assert K.inputs("lambda_0")[2].tobytes() == K.inputs("lambda_10")[2].tobytes()
    a, b = K.expected("lambda_0")[0], K.expected("lambda_10")[0]
    assert (a["v"] != b["v"]).any()


def test_rounding_case_separates_fused_from_unfused():
    src, start, table, plain, fused = K.rounding()
    differ = (plain["v"] != fused["v"]).any(axis=1) | (plain["metric"] != fused["metric"])
    assert differ.sum() >= 1


def test_three_unlike_are_unlike():
    cs = [K.CASES[n] for n in K.THREE_UNLIKE]
    assert len({c["prec"] for c in cs}) == 3 and 0 in {c["prec"] for c in cs}
    assert len({(c["xb"], c["yb"], c["w"], c["h"]) for c in cs}) == 3


def test_draws_cover_every_separation_and_lambda():
    cs = [K.draw_case(n) for n in range(K.N_DRAWS)]
    assert {c["xb"] for c in cs} == set(K.SEPARATIONS) and {c["yb"] for c in cs} == set(K.SEPARATIONS)
    assert {c["lam"] for c in cs} == set(K.LAMBDAS)
    assert all(17 <= c["w"] <= 120 and 17 <= c["h"] <= 120 and max(c["xb"], c["yb"]) <= c["ext"] <= 32 for c in cs)


def test_in_place_tables_equal_a_choice_from_them():
    """The error tables the restatement returns, fed back as `tables`, give the same field: the split into two launches."""
    for name in ("precision_3", "bounds", "padded_grid"):
        c = K.CASES[name]
        src, ref, start = K.inputs(name)
        field, tables, _ = K.expected(name)
        again, _ = R.subpel_deep(src, None, K.params_of(c), c["prec"], c["ref_index"], c["lam"], start, c["ext"], tables=tables)
        assert again.tobytes() == field.tobytes(), name
