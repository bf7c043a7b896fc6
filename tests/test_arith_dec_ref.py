"""Without a device: the restatement of the arithmetic transform-data decoder (tests/arith_dec_ref.py) against
oracle/dirac_stream.py -- which the reference decoder's digests pin -- on the reference's own stream, against hand-derived
bins, and on constructed cases for every result counter; the test writer by its round trip."""
import json
import os

import numpy as np

import arith_dec_draws as AD
import arith_dec_ref as AR
import arith_stream as AS
import noarith_enc_ref as enc
import stream_lib as S

D = S.D


def test_transform_data_is_the_tail_of_every_parse_unit():
    """All 100 pictures: the re-serialised transform data is exactly the end of the picture's parse unit, so the bytes the
    device tests feed are the stream's own."""
    n = 0
    for pic, payload in AS.units():
        data = AS.serialise(pic)
        assert len(data) > 100 and payload.endswith(data), pic.number
        n += 1
    assert n == 100


def test_first_twelve_pictures_equal_the_oracle():
    """Coded order, the compat state carried from picture to picture: the coefficient planes (behind DC prediction for the
    intra picture) are Decoder.decode_coefficients', the quant planes its quantised=True values."""
    compat = 0
    for rec in AS.pictures(limit=12):
        P = rec["twin"]
        assert P["compat"] == compat
        shapes = [c.shape for c in rec["coeffs"]]
        coeffs = [np.full(s, 0x5a5a, np.int16) for s in shapes]
        quant = [np.full(s, 0x3c3c, np.int16) for s in shapes]
        r = AR.decode_transform_data(rec["arith"], coeffs, quant, P["depth"], P["horiz_cb"], P["vert_cb"], P["cb_mode"], P["is_intra"], compat)
        compat = r["compat_quant_offset"]
        assert all(r[k] == v for k, v in AD.CLEAN.items()) and r["bytes_read"] == len(rec["arith"]), (rec["number"], r)
        assert r["bins"] > 4 * len(rec["arith"])
        for k in range(3):
            if P["is_intra"]:
                ll = enc.subband(coeffs[k], P["depth"], 0)
                wide = ll.astype(np.int32)
                D.dc_predict_s16(wide)
                ll[...] = wide.astype(np.int16)
            assert np.array_equal(coeffs[k], rec["coeffs"][k]), (rec["number"], k)
            assert np.array_equal(quant[k], rec["quant"][k].astype(np.int16)), (rec["number"], k)
        for k in range(3):
            for i, (q, payload) in enumerate(rec["picture"].subbands[k]):
                assert r["subband_length"][k, i] == len(payload) and (not payload or r["subband_quant_index"][k, i] == q)
    # picture 0 has one codeblock in sub-band 0 and codeblock mode 1: it runs the compat test, which turns the state on
    first = next(AS.pictures(limit=1))["twin"]
    assert (first["horiz_cb"][0], first["vert_cb"][0], first["cb_mode"], first["compat"]) == (1, 1, 1, 0) and compat == 1


def test_the_device_table_is_the_reference_table():
    """arith_dec.hip states the 256 numbers again; they are tests/golden/arith_lut.json's."""
    src = open(os.path.join(os.path.dirname(S.GOLDEN), "..", "schroedinger_amd", "csrc", "arith_dec.hip")).read()
    body = src[src.index("kAdLut[256] = {") + len("kAdLut[256] = {"):]
    body = body[:body.index("};")]
    assert [int(v) for v in body.replace("\n", " ").split(",") if v.strip()] == json.load(open(os.path.join(S.GOLDEN, "arith_lut.json")))["arith_lut"]


def one_band(payload, dtype=np.int16, qi=0, w=2, h=2):
    """A depth-0 4:4:4 picture of w x h whose luma is `payload`, chroma zero: (luma plane, quant plane, result)."""
    data = AD.header(len(payload), qi) + payload + AD.header(0, 0) * 2
    coeffs = [np.full((h, w), 77, dtype) for _ in range(3)]
    quant = [np.full((h, w), 78, dtype) for _ in range(3)]
    r = AR.decode_transform_data(data, coeffs, quant, 0, [1], [1], 0, 1, 0)
    assert not coeffs[1].any() and not quant[2].any()
    return coeffs[0], quant[0], r


def test_hand_derived_bins():
    """ff ff ff ff: code = 0xffffffff, range = 0xffff0000.  Bin 1 (ZPZN_F1, p = 0x8000): no renormalisation (range >
    0x40000000); range_x_prob = (0xffff * 0x8000) & 0xffff0000 = 0x7fff0000; code >= it: the bit is 1 -- the uint ends at
    once, value 0 --, code = 0x8000ffff, range = 0x80000000, p = 0x8000 - lut[0x80] = 0x8000 - 1935 = 0x7871.  Bin 2 (the
    next coefficient: left is 0, the same context): range_x_prob = (0x8000 * 0x7871) & 0xffff0000 = 0x3c380000 <= code: 1
    again, code = 0x43c8ffff, range = 0x43c80000.  Every value is 0, four bins for four coefficients."""
    lut = AR.tables()[0]
    assert lut[0x80] == 1935 and lut[127] == 1920
    a = D.Arith(b"\xff" * 4, lut)
    assert (a.bit(D.CTX_ZPZN_F1), a.code, a.range, a.prob[D.CTX_ZPZN_F1]) == (1, 0x8000ffff, 0x80000000, 0x7871)
    assert (a.bit(D.CTX_ZPZN_F1), a.code, a.range) == (1, 0x43c8ffff, 0x43c80000)
    plane, quant, r = one_band(b"\xff" * 4)
    assert not plane.any() and not quant.any() and r["bins"] == 4 and r["not_consumed"] == 0 and r["overran"] == 0
    """80 00 00 00 at quant index 0, intra (factor 4, offset 1: a value is stored as read): code = 0x80000000.  Bin 1: 1 as
    above (0x80000000 >= 0x7fff0000), value 0, code = 0x00010000, range = 0x80000000.  Bin 2 (ZPZN_F1, p = 0x7871):
    range_x_prob = 0x3c380000 > code: 0 -- a data bin follows --, range = 0x3c380000, p = 0x7871 + lut[255 - 0x78] =
    0x7871 + lut[135] = 0x7871 + 1980.  Bin 3 (COEFF_DATA, p = 0x8000): one shift (range 0x78700000, code 0x00020000);
    range_x_prob = (0x7870 * 0x8000) & 0xffff0000 = 0x3c380000 > code: data bit 0, bits = 0b10.  Bin 4 (ZP_F2, 0x8000): one
    shift (range 0x78700000, code 0x00040000), range_x_prob 0x3c380000 > code: 0, another data bin ... the code runs on
    over 0-bits: the first coefficient is 0, the second a large number."""
    a = D.Arith(b"\x80\x00\x00\x00", lut)
    assert (a.bit(D.CTX_ZPZN_F1), a.code, a.range) == (1, 0x00010000, 0x80000000)
    assert (a.bit(D.CTX_ZPZN_F1), a.range, a.prob[D.CTX_ZPZN_F1]) == (0, 0x3c380000, 0x7871 + lut[135])
    assert (a.bit(D.CTX_COEFF_DATA), a.range, a.code) == (0, 0x3c380000, 0x00020000)
    assert (a.bit(D.CTX_ZP_F2), a.range, a.code) == (0, 0x3c380000, 0x00040000)
    plane, quant, r = one_band(b"\x80\x00\x00\x00", np.int32)
    assert plane[0, 0] == 0 and quant[0, 1] != 0 and plane[0, 1] == quant[0, 1]
    """00 00 00 00: code = 0.  Bin 1: range_x_prob = 0x7fff0000 > 0: the bit is 0, range = 0x7fff0000, p = 0x8000 + lut[127]
    = 0x8000 + 1920.  Bin 2 (COEFF_DATA): range_x_prob = (0x7fff * 0x8000) & 0xffff0000 = 0x3fff0000 > 0: data bit 0, range
    = 0x3fff0000.  Bin 3 (ZP_F2): one shift, range = 0x7ffe0000; 0 again.  The code only ends in the 0xff bytes behind the
    payload, after 30 data bins of 1 ... 1: the value is 2^30 - 1, and at quant index 0 its reconstruction 1 + 4 v + 2 =
    2^32 - 1 wraps to -1, >> 2: -1 -- the defined reading of what C leaves undefined."""
    a = D.Arith(bytes(4), lut)
    assert (a.bit(D.CTX_ZPZN_F1), a.range, a.prob[D.CTX_ZPZN_F1]) == (0, 0x7fff0000, 0x8000 + 1920)
    assert (a.bit(D.CTX_COEFF_DATA), a.range) == (0, 0x3fff0000)
    assert (a.bit(D.CTX_ZP_F2), a.range, a.cntr) == (0, 0x3fff0000, 15)
    plane, quant, r = one_band(bytes(4), np.int32)
    assert quant[0, 0] == (1 << 30) - 1 and plane[0, 0] == -1 and r["long_codes"] == 0 and r["bins"] == 75


def test_every_counter_on_a_constructed_case():
    by_name = {c.name: c for c in AD.hostile()}
    r = by_name["cut-middle"].expected()[2]
    assert r["truncated"] == 1 and r["bytes_read"] > by_name["cut-middle"].data_bytes
    r = by_name["length-past-input"].expected()[2]
    assert (r["truncated"], r["not_consumed"], r["bytes_read"], r["subband_length"][0, 0], r["subband_quant_index"][0, 0]) == (1, 1, 4015, 4000, 7)
    r = by_name["zeros-64"].expected()[2]
    assert r["overran"] == 1 and r["long_codes"] == 1 and r["bins"] > 64 * 8 * 100          # the slowest input per byte
    r = by_name["ff-payloads"].expected()[2]
    assert r["not_consumed"] == 12 and r["bins"] == 24 and not any(p.any() for p in by_name["ff-payloads"].expected()[0])
    r = by_name["zeros-64-mode1-s32"].expected()[2]
    assert r["clamped_quant"] == 6 and r["overran"] == 6
    for name in ("long-codes-int16", "long-codes-int32"):
        coeffs, quant, r = by_name[name].expected()
        assert r["long_codes"] == 2
        ll = enc.subband(quant[0], 1, 0)
        # 33 data bins: bits wraps to 6, the value is 5; 31 data bins: (int) (2^31 + 1 - 1) is INT_MIN, its negation too
        assert ll[0, 1] == 5 and ll[1, 1] == 3 and ll[1, 0] == (0 if name.endswith("16") else -(1 << 31))
    coeffs, quant, r = by_name["index-61"].expected()
    assert coeffs is None and (r["error"], r["first_error"], r["compat_quant_offset"], r["bins"]) == (1, 1, 1, 0)
    r = by_name["empty"].expected()[2]
    assert r["bytes_read"] == 12 and r["bins"] == 0
    draws = {c.name: c for c in AD.draws()}
    assert draws["offsets-420"].expected()[2]["clamped_quant"] > 0 and draws["compat-on"].expected()[2]["compat_quant_offset"] == 1
