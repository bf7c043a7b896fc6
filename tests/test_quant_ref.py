"""CPU: tests/quant_ref.py, the checker of the encoder's quantisation, is the reference's arithmetic.

Pinned on the reference's compiled kernels: for every quant index 0 .. 60, inter and intra, all 65 536 s16 values through
the Orc program schro_frame_data_quantise picks, with its arguments -- the SHA-256 of the quantised and of the
reconstructed array, recorded from oracle/_ref (tests/golden/make_quant_golden.py), and the kernels themselves where
oracle/_ref is built.  The s32 path against schro_quantise / schro_dequantise taken literally; the round trip through the
decoder's dequantisation (oracle_lib, pinned on the reference decoder); the DC recurrence against a per-codeblock walk."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import quant_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = json.load(open(os.path.join(HERE, "golden", "quant_ref_digests.json")))
CASES = [(qi, intra) for intra in (0, 1) for qi in range(61)]


def key(qi, intra):
    return "q%02d_%s" % (qi, "intra" if intra else "inter")


def test_tables_are_complete_and_agree_with_the_decoder_side_fixture():
    t = Q.tables()
    assert sorted(t) == ["schro_table_inverse_quant", "schro_table_offset_1_2", "schro_table_offset_3_8", "schro_table_quant"]
    assert all(len(v) == 61 for v in t.values())
    old = json.load(open(os.path.join(HERE, "golden", "quant_tables.json")))
    for name, v in old.items():
        assert t[name] == v, name
    assert t["schro_table_offset_3_8"] == O.quant_offset_3_8()
    # the inverse is 0 exactly where the shift form is taken
    assert [q for q in range(61) if t["schro_table_inverse_quant"][q] == 0] == list(range(0, 61, 4))


def test_every_value_every_index_reproduces_the_recorded_digests():
    assert len(DIGESTS) == 122 + 2
    x = Q.all_s16()
    for qi, intra in CASES:
        q, r = Q.quantise_s16(x, qi, intra)
        assert Q.sha(q) == DIGESTS[key(qi, intra)]["quant"], (qi, intra, "quantised")
        assert Q.sha(r) == DIGESTS[key(qi, intra)]["recon"], (qi, intra, "reconstructed")
        if O.ref_available():       # ... and the kernels themselves where oracle/_ref is built
            rq, rr = Q.quantise_s16_orc(x, qi, intra)
            assert np.array_equal(q, rq) and np.array_equal(r, rr), (qi, intra)


def test_the_reciprocal_multiply_is_not_the_division():
    """A kernel that divides fails: somewhere quantdequant1 parts from schro_quantise, and early."""
    first = None
    for qi, intra in CASES:
        if qi == 0 or (qi & 3) == 0 or qi == 3:
            continue
        x = np.arange(0, 4096, dtype=np.int16)
        q = Q.quantise_s16(x, qi, intra)[0]
        lit = [Q.schro_quantise(int(v), Q.quant_factor(qi), Q.quant_offset(qi, intra)) for v in x]
        bad = np.flatnonzero(q != np.array(lit))
        if bad.size and (first is None or bad[0] < first[0]):
            first = (int(bad[0]), qi, intra)
    assert first is not None and first[0] < 100, first


def test_subtract_reproduces_the_recorded_digests():
    for u8 in (0, 1):
        d, s = Q.subtract_pin_inputs(u8)
        assert Q.sha(Q.subtract(d[None], s[None])[0]) == DIGESTS["subtract_%s" % ("u8" if u8 else "s16")]
        if O.ref_available():
            assert np.array_equal(Q.subtract_orc(d, s), Q.subtract(d[None], s[None])[0])
    # the common size, the rest of dst unchanged
    d, s = np.full((3, 5), -32768, np.int16), np.full((2, 7), 1, np.uint8)
    out = Q.subtract(d, s)
    assert (out[:2] == 32767).all() and (out[2] == -32768).all()


def test_s32_equals_schro_quantise_taken_literally():
    rng = np.random.default_rng(1)
    edge = np.array([0, 1, -1, 2, -2, 3, (1 << 27) - 1, -(1 << 27), (1 << 28) - 1, -(1 << 28) + 1])
    for qi, intra in CASES:
        v = np.concatenate([rng.integers(-(1 << 27), 1 << 27, 60), rng.integers(-400, 400, 60), edge])
        q, r = Q.quantise_s32(v, qi, intra)
        f, o = Q.quant_factor(qi), Q.quant_offset(qi, intra)
        ql = [Q.schro_quantise(int(a), f, o) for a in v]
        assert q.tolist() == ql and r.tolist() == [Q.schro_dequantise(a, f, o) for a in ql], (qi, intra)


def test_round_trip_through_the_decoder_dequantisation():
    """For every index and both offset tables the decoder's dequantisation (arith 0, and the 16-bit arith 1) of the
    checker's quantised values is the checker's reconstruction over |x| <= 4095.  (Over all s16 values the first
    departure is |x| = 5793 at index 50, intra: beyond the range a coefficient of an 8 .. 12-bit picture takes.)"""
    x = np.arange(-4095, 4096, dtype=np.int16)[None, :]
    for qi, intra in CASES:
        q, r = Q.quantise_s16(x, qi, intra)
        for arith in (0, 1):
            d = np.zeros_like(x)
            O.dequant_codeblock(d, q, qi, intra, arith)
            assert np.array_equal(d, r), (qi, intra, arith, x[0, np.flatnonzero(d != r)[:3]])
        q, r = Q.quantise_s32(x.astype(np.int32), qi, intra)
        d = np.zeros_like(r)
        O.dequant_codeblock(d, q, qi, intra, 0)
        assert np.array_equal(d, r), (qi, intra, "s32")


def codeblock_walk(band, recs_xy, intra):
    """schro_encoder_quantise_subband's loop taken literally: codeblock by codeblock in the order given, each with
    schro_frame_data_quantise_dc_predict's two loops and its (x, y) arguments (the codeblock's indices)."""
    line = band.astype(np.int64).copy()
    quant = np.zeros_like(line)
    s16 = band.dtype == np.int16
    wrap = Q._w16 if s16 else Q._w32
    for (cx, cy, x0, y0, w, h, qi) in recs_xy:
        f, o = Q.quant_factor(qi), Q.quant_offset(qi, intra)
        for j in range(h):
            for i in range(w):
                Y, X = y0 + j, x0 + i
                if cy + j > 0:
                    if cx + i > 0:
                        a = int(line[Y, X - 1] + line[Y - 1, X] + line[Y - 1, X - 1] + 1)
                        pred = ((a * 21845 + 10922) >> 16) if s16 else a // 3
                    else:
                        pred = int(line[Y - 1, X])
                else:
                    pred = int(line[Y, X - 1]) if cx + i > 0 else 0
                q = Q.schro_quantise(int(line[Y, X]) - pred, f, o)
                line[Y, X] = wrap(Q.schro_dequantise(q, f, o) + pred)
                quant[Y, X] = wrap(q)
    return quant.astype(band.dtype), line.astype(band.dtype)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_dc_recurrence_equals_the_codeblock_loop(dtype):
    """The raster-order recurrence over the band is the reference's loop over codeblocks (3 x 2 of them here)."""
    rng = np.random.default_rng(3)
    w, h = 13, 9
    band = (rng.integers(-32768, 32768, (h, w)) if dtype == np.int16 else rng.integers(-(1 << 20), 1 << 20, (h, w))).astype(dtype)
    xs, ys = [0, 4, 8, 13], [0, 4, 9]
    recs, qi_map = [], np.zeros((h, w), int)
    for cy in range(2):
        for cx in range(3):
            qi = (9 + 11 * len(recs)) % 61
            recs.append((cx, cy, xs[cx], ys[cy], xs[cx + 1] - xs[cx], ys[cy + 1] - ys[cy], qi))
            qi_map[ys[cy]:ys[cy + 1], xs[cx]:xs[cx + 1]] = qi
    q, r = Q.quantise_dc(band, qi_map, True)
    wq, wr = codeblock_walk(band, recs, True)
    assert np.array_equal(q, wq) and np.array_equal(r, wr)


def test_summaries():
    assert Q.summary_of(np.array([[0, -5], [3, 0]], np.int16)) == (2, 5)
    assert Q.summary_of(np.array([-32768, 1], np.int16)) == (2, 32768)
    assert Q.summary_of(np.zeros((4, 4), np.int32)) == (0, 0)
