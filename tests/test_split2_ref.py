"""CPU: tests/split2_ref.py, the restatement of the split-2 level of schro_mode_decision, and the cases of
tests/split2_cases.py: the raster order of the C text and the anti-diagonal order of the device give one result, every
case exercises what it is there for, and the parts are checked against brute force."""
import numpy as np
import pytest

import split2_cases as K
import split2_ref as R


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_raster_and_diagonal_order_agree_and_the_wants_hold(name):
    c = K.CASES[name]
    motion, sb, table, stats = K.expected(name)        # (asserts the case's wants)
    src, refs, fields = K.inputs(name)
    m2, sb2 = R.choose(table, K.params_of(c), c["w"], c["h"], c["lam"], fields, order="diagonal")
    assert m2.tobytes() == motion.tobytes() and sb2.tobytes() == sb.tobytes()
    # every record is split 2 and not global; a block outside the picture is the constant record
    flags = motion["flags"]
    assert ((flags >> 3) & 3 == 2).all() and ((flags >> 2) & 1 == 0).all()
    for j in range(c["nby"]):
        for i in range(c["nbx"]):
            if i * c["xb"] >= c["w"] or j * c["yb"] >= c["h"]:
                assert motion[j * c["nbx"] + i].tobytes() == R.BEST_MV
    assert len(sb) == c["nbx"] * c["nby"] // 16


@pytest.mark.parametrize("n", range(K.N_DRAWS))
def test_raster_and_diagonal_order_agree_on_the_draws(n):
    c, src, refs, fields, motion, sb, table = K.draw(n)
    stats = {}
    m2, sb2 = R.choose(table, K.params_of(c), c["w"], c["h"], c["lam"], fields, order="diagonal", stats=stats)
    assert m2.tobytes() == motion.tobytes() and sb2.tobytes() == sb.tobytes()


def test_the_wants_across_the_set():
    stats = [K.expected(name)[3] for name in K.CASES]
    for mode in range(4):
        assert sum(s["modes"][mode] for s in stats) > 0, mode
    assert sum(s["dc_leftover"] for s in stats) > 0
    assert sum(s["dc_considered_one_ref"] for s in stats) > 0
    assert sum(s["outside_mode1"] for s in stats) > 0 and sum(s["outside_mode2"] for s in stats) > 0
    assert sum(s["same_sb_outside_neighbour"] for s in stats) > 0 and sum(s["other_sb_outside_neighbour"] for s in stats) > 0
    # no inside block has an outside neighbour: the issue's want is replaced (tests/split2_cases.py says why)
    assert sum(s["inside_with_outside_neighbour"] for s in stats) == 0
    assert {K.CASES[n]["lam"] for n in K.CASES} >= set(K.LAMBDAS)
    assert {K.CASES[n]["prec"] for n in K.CASES} == {0, 1, 2, 3} and {K.CASES[n]["fmt"] for n in K.CASES} == set(K.FORMATS)
    assert {(K.CASES[n]["xb"], K.CASES[n]["yb"]) for n in K.CASES} >= {(4, 4), (8, 8), (12, 12), (16, 8), (32, 32)}
    assert len({(K.CASES[n]["refs"], K.CASES[n]["fmt"], K.CASES[n]["xb"]) for n in K.THREE_UNLIKE}) == 3


def test_a_dc_record_keeps_what_the_last_trial_left():
    """Rule 5: dy[1] and chroma_metric of a DC record are the last trial's; the flags keep the field's upper bits."""
    name = "precision_1"
    c = K.CASES[name]
    motion, _, table, _ = K.expected(name)
    _, _, fields = K.inputs(name)
    seen = 0
    for n in np.nonzero(motion["flags"] & 3 == 0)[0]:
        rec = motion[n]
        assert int(rec["v"][3]) == int(fields[1]["v"][n][3])
        assert int(rec["flags"]) & ~0x1f == int(fields[1]["flags"][n]) & ~0x1f
        assert int(rec["metric"]) == int(table[n][R.T_DC_ERROR])
        assert [int(x) for x in rec["v"][:3]] == [int(x) for x in table[n][R.T_DC:R.T_DC + 3]]
        want = int(table[n][R.T_BI_CHROMA]) if table[n][R.T_BI_OK] else int(table[n][R.T_CHROMA + 1])
        assert int(rec["chroma_metric"]) == want
        seen += int(rec["v"][3]) != 0
    assert seen > 0


def test_the_two_forms_of_a_block_outside_the_picture():
    """Rule 1: inside its superblock an outside block is seen with the predicted mode and vector, everywhere else as the
    constant record -- and the final field holds the constant."""
    name = "padded_x"
    c = K.CASES[name]
    motion, _, table, stats = K.expected(name)
    _, _, fields = K.inputs(name)
    assert stats["outside_mode2"] > 0
    nbx = c["nbx"]
    final = [bytearray(motion[n].tobytes()) for n in range(motion.size)]
    x = -(-c["w"] // c["xb"])                           # the first outside column
    assert x % 4 != 0 and x < nbx
    differs = 0
    for y in range(c["nby"]):
        st = R.new_stats()
        work, fin, error, entropy = R.choose_block(lambda nx, ny: final[ny * nbx + nx], x, y, False, 2, c["lam"], fields, table[y * nbx + x],
                                                   y * nbx + x, False, st)
        assert bytes(fin) == R.BEST_MV == motion[y * nbx + x].tobytes() and (error, entropy) == (0, 2)
        mode = R.pred_mode(work)
        assert mode in (1, 2) and (R.vec(work, 2 - mode), R.vec(work, 4 - mode)) == (0, 0)
        differs += bytes(work) != R.BEST_MV
    assert differs > 0


def test_block_average_against_brute_force():
    rng = np.random.default_rng(5)
    comp = rng.integers(0, 256, (23, 37)).astype(np.uint8)
    for (x, y, w, h) in ((0, 0, 8, 8), (32, 16, 8, 8), (36, 22, 4, 4), (35, 0, 2, 2), (0, 20, 32, 32)):
        block = comp[y:y + h, x:x + w].astype(np.int64)
        ave = (int(block.sum()) + block.size // 2) // block.size
        assert R.block_average(comp, x, y, w, h) == (ave - 128, int(np.abs(block - ave).sum()))
    assert R.block_average(comp, 37, 0, 8, 8) is None and R.block_average(comp, 0, 23, 8, 8) is None
    assert R.block_average(comp, 0, 0, 0, 8) is None


def test_biref_metric_against_brute_force():
    rng = np.random.default_rng(6)
    o, a, b = (rng.integers(0, 256, (7, 9)).astype(np.int32) for _ in range(3))
    want = sum(abs(int(o[j, i]) - ((int(a[j, i]) + int(b[j, i]) + 1) >> 1)) for j in range(7) for i in range(9))
    assert R.metric_biref(o, a, b) == want


@pytest.mark.parametrize("prec", [1, 2])
def test_the_shared_fetch_buffers_of_precision_2_and_3(prec):
    """At mv_precision > 1 the bi-reference trial measures luma against V's prediction in the corner V covers and U against
    V's prediction; at 0 and 1 every component against its own."""
    name = "precision_%d" % prec
    c = K.CASES[name]
    src, refs, fields = K.inputs(name)
    P = K.params_of(c)
    _, _, table, _ = K.expected(name)
    ups = [[R.UpFrame(r[k], c["ext"]) for k in range(3)] for r in refs]
    hs, vs = P["h_shift"], P["v_shift"]
    n = 1 * c["nbx"] + 1
    assert table[n][R.T_BI_OK]
    pred = []
    for k in range(3):
        bw, bh = (c["xb"] >> (hs if k else 0)), (c["yb"] >> (vs if k else 0))
        both = []
        for r in (0, 1):
            vx, vy = int(fields[r]["v"][n][r]) >> (hs if k else 0), int(fields[r]["v"][n][2 + r]) >> (vs if k else 0)
            both.append(ups[r][k].block((bw << prec) + vx, (bh << prec) + vy, prec, bw, bh))
        pred.append((both[0] + both[1] + 1) >> 1)
    orig = [src[k][pred[k].shape[0]:2 * pred[k].shape[0], pred[k].shape[1]:2 * pred[k].shape[1]].astype(np.int32) for k in range(3)]
    own = [int(np.abs(orig[k] - pred[k]).sum()) for k in range(3)]
    if prec < 2:
        assert (int(table[n][R.T_BI_LUMA]), int(table[n][R.T_BI_CHROMA])) == (own[0], own[1] + own[2])
    else:
        luma = pred[0].copy()
        luma[:pred[2].shape[0], :pred[2].shape[1]] = pred[2]
        assert int(table[n][R.T_BI_LUMA]) == int(np.abs(orig[0] - luma).sum()) != own[0]
        assert int(table[n][R.T_BI_CHROMA]) == int(np.abs(orig[1] - pred[2]).sum()) + own[2]


def test_the_prediction_skips_neighbours_that_lack_the_reference():
    """Rule 7: a DC neighbour gives no vector, a reference-2 neighbour none for reference 1."""
    def rec(mode, dx0, dy0, dx1, dy1):
        r = bytearray(R.BEST_MV)
        R.set_mode(r, mode)
        for k, v in enumerate((dx0, dx1, dy0, dy1)):
            R.set_vec(r, k, v)
        return r
    grid = {(0, 1): rec(0, 50, 60, 70, 80), (1, 0): rec(2, 9, 9, 4, -6), (0, 0): rec(3, 2, -2, 8, 10)}
    get = lambda x, y: grid[x, y]
    assert R.vector_prediction(get, 1, 1, 1) == (2, -2)                 # only the above-left one has reference 1
    assert R.vector_prediction(get, 1, 1, 2) == (6, 2)                  # two: the rounded mean
    grid[0, 1] = rec(1, 5, 7, 0, 0)
    assert R.vector_prediction(get, 1, 1, 1) == (4, 3)
    grid[0, 1][0] |= 4                                                  # using_global
    assert R.vector_prediction(get, 1, 1, 1) == (2, -2)
    assert R.mode_prediction(get, 1, 1) == (1 & 2) | (2 & 3) | (3 & 1)


def test_int_max_metrics():
    """Rule 6: the block's error for that reference is INT_MAX and chroma_metric keeps the copied value.  A DC trial always
    follows (its trigger compares with best_error = INT_MAX at the most) and wins, so where the record shows it is in what
    the DC record keeps: with one reference, the field's chroma_metric and not the table's."""
    name = "int_max_one_reference"
    c = K.CASES[name]
    motion, sb, table, stats = K.expected(name)
    _, _, fields = K.inputs(name)
    assert stats["int_max"] > 0
    seen = 0
    for j in range(-(-c["h"] // c["yb"])):
        for i in range(-(-c["w"] // c["xb"])):
            n = j * c["nbx"] + i
            if int(fields[0]["metric"][n]) == R.INT_MAX:
                assert int(motion["flags"][n]) & 3 == 0
                assert int(motion["chroma_metric"][n]) == int(fields[0]["chroma_metric"][n]) != int(table[n][R.T_CHROMA])
                seen += 1
            elif int(motion["flags"][n]) & 3 == 0:
                assert int(motion["chroma_metric"][n]) == int(table[n][R.T_CHROMA])
    assert seen == stats["int_max"]
    # two references: the trial of the other reference, the bi-reference trial or DC takes the block
    name = "int_max"
    motion, _, _, stats = K.expected(name)
    fields = K.inputs(name)[2]
    assert stats["int_max"] > 0
    for n in range(motion.size):
        mode = int(motion["flags"][n]) & 3
        if mode in (1, 2) and K.CASES[name]["w"] > (n % K.CASES[name]["nbx"]) * 8 and K.CASES[name]["h"] > (n // K.CASES[name]["nbx"]) * 8:
            assert int(fields[mode - 1]["metric"][n]) != R.INT_MAX


def test_fused_scoring_gives_another_field():
    fields, table, plain, sb, fused = K.rounding()
    assert plain.tobytes() != fused.tobytes()
    c = K.ROUNDING
    again, sb2 = R.choose(table, K.params_of(c), c["w"], c["h"], c["lam"], fields, order="diagonal")
    assert again.tobytes() == plain.tobytes() and sb2.tobytes() == sb.tobytes()
