"""CPU: tests/mode_ref.py, the restatement of schro_mode_decision entire, and the cases of tests/mode_cases.py: the raster
order of the C text and the anti-diagonal order of the device give one result, every case exercises what it is there
for, the rules the restatement names are each shown by a test that fails when the rule is dropped, and the parts are
checked against direct computation."""
import numpy as np
import pytest

import mode_cases as C
import mode_ref as M
import split2_ref as R


def walk(name, **kw):
    c = C.CASES[name]
    src, refs, fields, level1, level2 = C.inputs(name)
    out = C.expected(name)
    P = C.params_of(c)
    return M.choose(out[4], out[5], P, c["w"], c["h"], c["lam"], fields, level1, level2, M.picture_reader(src, refs, P, c["ext"]), **kw)


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4]))


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_raster_and_diagonal_order_agree_and_the_wants_hold(name):
    c = C.CASES[name]
    out = C.expected(name)                              # (asserts the case's wants)
    assert same(out, walk(name, order="diagonal"))
    motion, sb, trials = out[:3]
    assert len(sb) == len(trials) == c["nbx"] * c["nby"] // 16
    # a trial that is not valid is written as zeros; the winner's sums are one of the valid trials'
    for n in range(len(sb)):
        for t in trials[n]:
            assert t["state"] in (-1, 0, 1) and (t["state"] == 1 or (t["error"], t["entropy"], t["score"]) == (0, 0, 0.0))
        assert any(t["state"] == 1 and (t["error"], t["entropy"]) == (sb["error"][n], sb["entropy"][n]) and t["score"].tobytes() == sb["score"][n].tobytes()
                   for t in trials[n])
        assert trials[n][0]["state"] == 1 and trials[n][3]["state"] == (-1 if c["refs"] == 1 else trials[n][3]["state"])
    # the records of a superblock say its split, and split 1 / split 0 records come in fours and sixteens
    nbx = c["nbx"]
    for j in range(0, c["nby"], 4):
        for i in range(0, nbx, 4):
            split = (int(motion["flags"][j * nbx + i]) >> 3) & 3
            for jj in range(4):
                for ii in range(4):
                    rec = motion[(j + jj) * nbx + i + ii]
                    assert (int(rec["flags"]) >> 3) & 3 == split
                    head = motion[(j + (jj & ~((4 >> split) - 1))) * nbx + i + (ii & ~((4 >> split) - 1))]
                    assert rec.tobytes() == head.tobytes()


@pytest.mark.parametrize("n", range(C.N_DRAWS))
def test_raster_and_diagonal_order_agree_on_the_draws(n):
    c, (src, refs, fields, level1, level2), out = C.draw(n)
    P = C.params_of(c)
    again = M.choose(out[4], out[5], P, c["w"], c["h"], c["lam"], fields, level1, level2, M.picture_reader(src, refs, P, c["ext"]), order="diagonal")
    assert same(out, again)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_what_an_invalid_trial_leaves_behind_reaches_nothing(name):
    """Rule 4: the reference goes on after an invalid quadrant and `motion` keeps what was written; stopping at the first
    invalid quadrant gives the same field, sums, trials and statistics."""
    assert same(C.expected(name), walk(name, stop_at_invalid=True))


def test_the_wants_across_the_set():
    stats = [C.expected(name)[6] for name in C.CASES] + [C.crafted()[6]]

    def total(key, k=None):
        return sum(s[key] if k is None else s[key][k] for s in stats)
    for split in range(3):
        assert total("final_split", split) > 0                          # every final split occurs
    assert total("zero_wins") > 0                                       # ... and the zero-vector trial wins somewhere
    for s in range(5):
        assert total("singles", s) > 0, s                               # rule 1: every number of single-reference quadrants
    assert total("honest_loss", 2) + total("honest_loss", 4) > 0        # ... and an even one that loses honestly to split 2
    assert total("invalid_quadrant", 0) > 0 and sum(total("invalid_quadrant", q) for q in (1, 2, 3)) > 0                # rule 4
    named = [C.expected(name)[6] for name in C.CASES]
    assert sum(s["split0_not_tried"] for s in named) > 0 and sum(s["split0_lost"] for s in named) > 0
    assert (C.crafted()[5][2]["state"][:, 2] == 0).sum() > 0           # split 0 tried and invalid (crafted tables)
    assert total("dropped_by_the_shift") > 0 and total("kept_by_the_shift") > 0                                         # rule 2
    assert total("hint_int_max") > 0 and total("out_of_bounds") > 0 and total("out_of_bounds0") > 0
    assert total("outside_quadrant_mode", 2) > 0 and total("outside_quadrant_mode", 1) > 0                              # rule 3
    assert total("rule7") > 0
    assert total("split1_bi", 1) > 0 and total("split0_bi", 1) > 0
    assert {C.CASES[n]["lam"] for n in C.CASES} >= set(C.LAMBDAS)
    assert {C.CASES[n]["prec"] for n in C.CASES} == {0, 1, 2, 3} and {C.CASES[n]["fmt"] for n in C.CASES} == {"420", "422", "444"}
    assert {C.CASES[n]["refs"] for n in C.CASES} == {1, 2}
    assert len({(C.CASES[n]["refs"], C.CASES[n]["fmt"], C.CASES[n]["xb"]) for n in C.THREE_UNLIKE}) == 3


def test_a_single_reference_quadrant_adds_int_max():
    """Rule 1: the split-1 trial's error is the honest sum plus s * INT_MAX, wrapped to int32."""
    seen = set()
    for name in ("precision_1", "format_444", "one_reference"):
        c = C.CASES[name]
        out = C.expected(name)
        src, refs, fields, level1, level2 = C.inputs(name)
        P = C.params_of(c)
        nbx = c["nbx"]
        for n in range(len(out[1])):
            t = out[2][n][1]
            if t["state"] != 1:
                continue
            # the trial once more, counting its single-reference quadrants
            st = M.new_stats()
            w = M._Walk(out[4], out[5], P, c["w"], c["h"], c["lam"], fields, level1, level2, M.picture_reader(src, refs, P, c["ext"]), False, False, st)
            i, j = 4 * (n % (nbx // 4)), 4 * (n // (nbx // 4))
            final = [bytearray(r.tobytes()) for r in out[0]]
            own = {}

            def get(x, y):
                return own[x, y] if (x >> 2, y >> 2) == (i >> 2, j >> 2) else final[y * nbx + x]
            w.split2(get, lambda x, y, rec: own.__setitem__((x, y), rec), i, j)
            block = M._Block()
            _, singles = w.split1(get, lambda x, y, rec: own.__setitem__((x, y), rec), i, j, block)
            assert block.error == int(t["error"])
            # an odd s: hugely negative or positive by about 2^31; an even one: within 4 of a plausible SAD sum
            if singles % 2:
                assert abs(block.error) > 1 << 29
            else:
                assert 0 <= block.error + singles < 16 * 255 * c["xb"] * c["yb"] * 3
            seen.add(singles)
    assert seen == {0, 1, 2, 3, 4}


def test_the_quadrant_sums_are_the_superblock_sad():
    """The split-0 SAD of a vector over the clipped superblock is the sum of its SADs over the four clipped quadrants, in
    every component, whatever the precision: clipping and the bilinear form are per sample."""
    seen = 0
    for name in ("precision_3", "clipped_padded", "block_16x8", "block_32x32", "padded_x"):
        c = C.CASES[name]
        src, refs, fields, level1, level2 = C.inputs(name)
        table = C.expected(name)[5]
        P = C.params_of(c)
        nbx, nby, blocks, sizes = R.geometry(P, c["w"], c["h"])
        dims = (P["h_shift"], P["v_shift"])
        ups = [[R.UpFrame(r[k], c["ext"]) for k in range(3)] for r in refs]
        for n in range(len(table)):
            i, j = 4 * (n % (nbx // 4)), 4 * (n // (nbx // 4))
            for ref in range(c["refs"]):
                for cand, (vx, vy) in enumerate(M.candidates(fields, level1, level2, nbx, i, j, ref, c["prec"])):
                    e = table[n][ref * M.M_REF_INTS + cand * M.M_CAND_INTS:][:M.M_CAND_INTS]
                    if not e[M.M_OK0] or cand % 5 != 0:
                        continue
                    whole = [0, 0]
                    for k in range(3):
                        x0, y0 = i * blocks[k][0], j * blocks[k][1]
                        w, h = min(4 * blocks[k][0], sizes[k][0] - x0), min(4 * blocks[k][1], sizes[k][1] - y0)
                        dx = (vx >> (dims[0] if k else 0)) + (x0 << c["prec"])
                        dy = (vy >> (dims[1] if k else 0)) + (y0 << c["prec"])
                        whole[k > 0] += M._sad(src, ups, ref, k, x0, y0, w, h, dx, dy, c["prec"])
                    quads = [(int(e[M.M_QUAD + 2 * q]), int(e[M.M_QUAD + 2 * q + 1])) for q in range(4) if e[M.M_QUAD + 2 * q] != M.M_NONE]
                    assert whole == [sum(a for a, _ in quads), sum(b for _, b in quads)], (name, n, ref, cand)
                    seen += 1
    assert seen > 50


@pytest.mark.parametrize("prec", [0, 1, 2, 3])
def test_the_shared_fetch_buffers_at_split_1_and_split_0(prec):
    """Rule 6: at mv_precision 2 and 3 the bi-reference trials of a split-1 quadrant, of split 0 and of the zero vectors
    measure luma against V's prediction in the corner V covers and U against V's; at 0 and 1 every component against its
    own."""
    name = "precision_%d" % prec
    c = C.CASES[name]
    src, refs, fields, level1, level2 = C.inputs(name)
    P = C.params_of(c)
    ups = [[R.UpFrame(r[k], c["ext"]) for k in range(3)] for r in refs]
    hs, vs = P["h_shift"], P["v_shift"]
    for split, (x, y), v0, v1 in ((1, (6, 2), (3, -2), (-5, 1)), (0, (4, 4), (-3, 2), (2, 2)), (0, (8, 4), (0, 0), (0, 0))):
        scale = 4 >> split
        ok, luma, chroma = M.biref_metric(src, ups, P, c["ext"], split, x, y, v0, v1)
        assert ok
        pred, orig = [], []
        for k in range(3):
            bw, bh = c["xb"] >> (hs if k else 0), c["yb"] >> (vs if k else 0)
            both = []
            for r, (vx, vy) in enumerate((v0, v1)):
                both.append(ups[r][k].block(((x * bw) << prec) + (vx >> (hs if k else 0)), ((y * bh) << prec) + (vy >> (vs if k else 0)), prec,
                                            scale * bw, scale * bh))
            pred.append((both[0] + both[1] + 1) >> 1)
            orig.append(src[k][y * bh:(y + scale) * bh, x * bw:(x + scale) * bw].astype(np.int32))
        own = [int(np.abs(orig[k] - pred[k]).sum()) for k in range(3)]
        if prec < 2:
            assert (luma, chroma) == (own[0], own[1] + own[2])
        else:
            mixed = pred[0].copy()
            mixed[:pred[2].shape[0], :pred[2].shape[1]] = pred[2]
            assert luma == int(np.abs(orig[0] - mixed).sum()) != own[0]
            assert chroma == int(np.abs(orig[1] - pred[2]).sum()) + own[2]
    if (8 // 4, 4 // 4) == (2, 1):
        table = C.expected(name)[5]
        zero = table[1 * (c["nbx"] // 4) + 2][M.M_ZERO_BI:]
        assert (int(zero[0]), int(zero[1]), int(zero[2])) == (1, luma, chroma)


def test_the_duplicate_test_shifts_what_is_shifted_already():
    """Rule 2, on `doubles`: in every quadrant the second sub-pel vector (the true motion unshifted) is dropped because,
    shifted, it equals the first; the third, a true copy of the first, is kept.  With the right shift (none) it would be
    the other way round."""
    name = "doubles"
    c = C.CASES[name]
    stats = C.expected(name)[6]
    dropped = [(ref, slot) for ref, slot, shift in stats["dropped"] if slot % 5 == 1 and shift == c["prec"]]
    assert len(dropped) >= c["nbx"] * c["nby"] // 4         # (every quadrant, both references, unless the first was INT_MAX)
    assert not [1 for ref, slot, shift in stats["dropped"] if slot % 5 == 2 and shift == c["prec"]]
    assert stats["dropped_by_the_shift"] > 0 and stats["kept_by_the_shift"] > 0
    # precision 0 shifts by nothing: the rule cannot show
    assert C.expected("precision_0")[6]["dropped_by_the_shift"] == 0 == C.expected("precision_0")[6]["kept_by_the_shift"]


def test_a_level_hint_is_a_copy_of_its_record():
    """Rule 2: where the level-1 hint wins a quadrant, the record carries the field's other slot and flag bytes."""
    seen = 0
    for name in ("precision_1", "precision_0", "format_444", "lambda_10", "one_reference_padded"):
        c = C.CASES[name]
        motion = C.expected(name)[0]
        _, _, fields, level1, level2 = C.inputs(name)
        nbx = c["nbx"]
        for y in range(0, c["nby"], 2):
            for x in range(0, nbx, 2):
                n = y * nbx + x
                rec = motion[n]
                flags = int(rec["flags"])
                if (flags >> 3) & 3 != 1 or flags & 3 == 3 or x * c["xb"] >= c["w"] or y * c["yb"] >= c["h"]:
                    continue
                r = (flags & 3) - 1
                level = level1[r][n]
                if (int(level["v"][r]) << c["prec"], int(level["v"][2 + r]) << c["prec"]) != (int(rec["v"][r]), int(rec["v"][2 + r])):
                    continue
                subs = [fields[r][n + d] for d in (0, 1, nbx, nbx + 1)]
                if any((int(s["v"][r]), int(s["v"][2 + r])) == (int(rec["v"][r]), int(rec["v"][2 + r])) for s in subs):
                    continue                                # (a sub-pel hint with the same vector may have won instead)
                assert (int(rec["v"][1 - r]), int(rec["v"][3 - r])) == (int(level["v"][1 - r]), int(level["v"][3 - r]))
                assert flags >> 5 == int(level["flags"]) >> 5
                seen += 1
    assert seen > 0


def test_a_quadrant_outside_the_picture_keeps_the_predicted_form():
    """Rule 3: where split 1 wins, a quadrant outside the picture holds split 1, the predicted mode and the predicted
    vector in that mode's slot -- not split 2's constant record."""
    seen = modes = 0
    for name in ("padded_x", "clipped_padded", "block_16x8", "one_reference_padded"):
        c = C.CASES[name]
        motion = C.expected(name)[0]
        nbx = c["nbx"]
        for y in range(0, c["nby"], 2):
            for x in range(0, nbx, 2):
                rec = motion[y * nbx + x]
                flags = int(rec["flags"])
                if (flags >> 3) & 3 == 1 and (x * c["xb"] >= c["w"] or y * c["yb"] >= c["h"]):
                    assert flags & 0xff in (0x09, 0x0a) and int(rec["metric"]) == 0
                    seen += 1
                    modes |= flags & 3
    assert seen > 0 and modes & 1
    # (mode 2 is predicted for outside quadrants of trials in these cases too: test_the_wants_across_the_set)
    assert sum(C.expected(name)[6]["outside_quadrant_mode"][2] for name in ("padded_x", "clipped_padded", "block_16x8")) > 0


def test_using_global_travels_with_a_hint():
    """Rule 11: a sub-pel record with the using_global bit set is a candidate with entropy 0, and the bit reaches the
    field."""
    name = "precision_1"
    c = C.CASES[name]
    src, refs, fields, level1, level2 = C.inputs(name)
    fields = [f.copy() for f in fields]
    for f in fields:
        f["flags"][::3] |= 4
    out = C.reference(c, src, refs, fields, level1, level2)
    plain = C.expected(name)
    assert out[0].tobytes() != plain[0].tobytes()
    split = (out[0]["flags"] >> 3) & 3
    assert ((out[0]["flags"] & 4 != 0) & (split == 1)).sum() > 0
    assert ((out[0]["flags"] & 4 != 0) & (split == 2)).sum() == 0   # (the split-2 trial clears it)
    again = C.reference(c, src, refs, fields, level1, level2, order="diagonal")
    assert same(out, again)


def test_rule_7_and_an_invalid_split_0_trial_on_crafted_tables():
    fields, level1, level2, table2, table, out, stats = C.crafted()
    c = C.CRAFTED
    again = M.choose(table2, table, C.params_of(c), c["w"], c["h"], c["lam"], fields, level1, level2, C._no_reads, order="diagonal")
    assert same(out, again)
    trials = out[2]
    shown = 0
    for n in range(len(trials)):
        t2, t1, t0, tz = trials[n]
        if t0["state"] == 1 and tz["state"] == 1 and t0["score"] < tz["score"] < t1["score"]:
            # the zero vectors replace a split-0 winner that scores better than they do
            assert out[1]["score"][n] == tz["score"]
            shown += 1
    assert shown == stats["rule7"] > 0


def test_the_statistics_against_a_direct_computation():
    for name in ("precision_1", "block_16x8", "one_reference_padded", "lambda_0"):
        c = C.CASES[name]
        motion, sb, trials, stats = C.expected(name)[:4]
        size = 16 * c["xb"] * c["yb"] * 2 // 3
        total = 0.0
        for e in sb["error"]:
            total = total + (float(int(e)) * float(int(e))) / float(size * size)
        n = c["nbx"] * c["nby"]
        step = total / 57600.0
        step = step / c["nbx"]
        step = step * c["nby"]
        step = step / 16
        assert stats[0] == step
        assert stats[1] == float(int((sb["error"] > 10 * size).sum())) / (n // 16)
        assert stats[2] == float(int((motion["flags"] & 3 == 0).sum())) / n
    # rule 1 reaches them: an odd number of single-reference quadrants makes mc_error astronomic
    assert C.expected("precision_1")[3][0] > 1e6


def test_fused_scoring_gives_another_result():
    """Rule 9: with the products and sums fused the walk decides otherwise somewhere in the set."""
    differs = 0
    for name in ("lambda_small", "precision_1", "format_444", "lambda_10", "padded_x"):
        differs += not same(C.expected(name), walk(name, fused=True))
    assert differs > 0


@pytest.mark.parametrize("split", [1, 0])
def test_the_rounding_cases_separate_fused_from_unfused_scores(split):
    """Rule 9 at split 1 and at split 0: candidates that tie in exact arithmetic; the trial's winner differs between the
    two roundings, and the anti-diagonal order gives the unfused result."""
    fields, level1, level2, table2, table, plain, fused = C.rounding(split)
    level = 1 if split == 1 else 2
    assert plain[2][0][level]["entropy"] != fused[2][0][level]["entropy"] and plain[0].tobytes() != fused[0].tobytes()
    c = C.CRAFTED
    again = M.choose(table2, table, C.params_of(c), c["w"], c["h"], c["lam"], fields, level1, level2, C._no_reads, order="diagonal")
    assert same(plain, again)
