"""CPU: the walk over tests/quant_choose_draws.py.  The device's exp and log are not the host's (each within 1 ulp, so
the entropy estimates agree to parts in 10^16, compared at a relative 1e-9), while indices and the searches' branches are
discrete: a draw may not sit on a tie.  For every case and every evaluation the restatement makes:
  - the runner-up of every argmin is a relative 1e-6 above the winner, or equal to it as bits;
  - both sides of every comparison of a sum (with the target, or of lo with hi) are a relative 1e-6 apart, or equal as
    bits, or one of them is NaN (the device has NaN where the restatement has it, and every comparison with it is false).
A draw that fails is replaced in the list.  The walk also holds the lists to the branches they are there for."""
import math

import numpy as np
import pytest

import quant_choose_draws as D
import quant_choose_ref as R

check_trace = D.check_trace


@pytest.mark.parametrize("k", range(len(D.ENGINE_CASES)))
def test_margins(k):
    out, trace = D.expected(k)
    assert trace and math.isfinite(out["target"])       # (a non-finite target is refused)
    check_trace(trace, D.ENGINE_CASES[k])
    assert 0 <= out["quant_index"].min() and out["quant_index"].max() < 60
    # the reference's control flow leaves a target outside [lo, hi] only through the five-step exhaustion, which ends in
    # lo == hi and the early return (or in NaN sums, where no comparison is true): its "not bracketed" message is dead
    assert out["not_bracketed"] == 0


def paths(engine):
    return [(D.ENGINE_CASES[k], D.expected(k)[0]) for k in range(len(D.ENGINE_CASES)) if D.ENGINE_CASES[k][1] == engine]


@pytest.mark.parametrize("engine,halvings,most", [(D.B, 7, 14), (D.E, 14, 20)])
def test_branches_reached(engine, halvings, most):
    got = paths(engine)
    p = [o["path"] for _, o in got]
    for direction in ("up", "down"):
        mine = [q for q in p if q["direction"] == direction]
        assert {q["steps"] for q in mine if q["broke"]} >= {1, 2 if direction == "down" else 3, 5}, direction
        assert any(q["steps"] == 5 and not q["broke"] and q["early"] for q in mine), direction      # exhausted, lo == hi
    assert any(q["halvings"] == halvings for q in p)
    assert all(q["halvings"] in (0, halvings) for q in p)       # lo <= target < hi is kept: the loop never ends early
    assert max(o["evaluations"] for _, o in got) == most
    assert all(o["evaluations"] == 1 + o["path"]["steps"] + o["path"]["halvings"] + (engine == D.B) for _, o in got)
    # NaN sums: five steps without a break and NO early return (NaN != NaN), then every halving
    if engine == D.B:
        nan = [o for c, o in got if c[0] == "d2_nan"]
        assert nan and all(math.isnan(o["sum"]) and o["path"]["steps"] == 5 and not o["path"]["early"]
                           and o["path"]["halvings"] == 7 and o["evaluations"] == 14 for o in nan)


def test_lambda_engine_cases():
    lams = sorted(c[2][1] for c in D.ENGINE_CASES if c[1] == D.L)
    assert lams[0] == 1e-10 and lams[-1] == 1e10
    for k, c in enumerate(D.ENGINE_CASES):
        if c[1] == D.L:
            o, _ = D.expected(k)
            assert o["evaluations"] == 1 and o["frame_lambda"] == c[2][1]


def test_constant_error_leaves_stale_indices():
    """the indices constant_error leaves are its last evaluation's, and at the lambda it returns the choice differs"""
    differ = 0
    for k, c in enumerate(D.ENGINE_CASES):
        if c[1] != D.E:
            continue
        o, _ = D.expected(k)
        pic = D.get(c[0])
        ent, err = D.estimates(c[0])
        ev = R.Evaluator(ent, err, pic["depth"], pic["weight"], pic["scales"])
        ev.lambda_to_error(o["frame_lambda"])
        differ += not np.array_equal(ev.indices, o["quant_index"])
    assert differ >= 1


def test_special_sub_bands():
    ent, err = D.estimates("d1_edges")
    assert np.isnan(ent[1, 1]).all() and np.all(err[1, 1] == 0)                 # every sampled value in `overflow`
    assert np.all(ent[1, 2] == 0) and np.all(err[1, 2] == 0)                    # every coefficient zero: bin[1] == 0
    assert np.all(ent[0, 1] == 0)
    assert np.isfinite(ent[0, 0]).all() and ent[0, 0, 0] > 0                    # a single sample
    assert np.isfinite(ent[0, 2]).all() and err[0, 2, 59] > 1e20                # 2^32 - 1 counts under skip 32
    # start >= end at high indices: the ranges from the third on are empty there, and bin 103's mass is still seen
    hi = [j for j in range(60) if R.range_start(j, 2) >= 32000]
    assert hi and np.all(ent[0, 2, hi] > 0)
    assert np.isnan(D.estimates("d2_nan")[0][2, 4]).all()
    assert np.all(D.estimates("d2_nan_arith")[0][0, 3] == 0)                    # the arith branch has no NaN
    for name in D.ESTIMATE_CASES:
        pic = D.get(name)
        # what schro_hip_histogram_batch can leave: fewer than 2^32 sampled values per sub-band, overflow included
        assert int(pic["counts"].astype(np.uint64).sum(axis=2).max()) < 1 << 32
    assert {s for n in D.ESTIMATE_CASES for s in D.get(n)["skip"]} >= {1, 2, 4, 8, 16, 32}
    assert {D.get(n)["depth"] for n in D.ESTIMATE_CASES} >= {0, 3, 6}


def test_mixed_batch_names_cases():
    got = [D.ENGINE_CASES[D.case_index(n, e)] for n, e in D.MIXED_BATCH]
    assert len(got) == 8 and len({D.get(c[0])["depth"] for c in got}) >= 4
    assert {c[1] for c in got} == {D.L, D.B, D.E} and {D.get(c[0])["is_noarith"] for c in got} == {0, 1}
