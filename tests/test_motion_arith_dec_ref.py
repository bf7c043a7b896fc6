"""CPU: the restatement of the arithmetic motion-data decoder (tests/motion_arith_dec_ref.py) pinned -- on the reference's own
stream against oracle/dirac_stream.py, whose fields the reference decoder's digests hold; by hand-derived cases; its two
forms against each other; its writer by the round trip; its counters by witnesses."""
import json
import os
import re

import numpy as np
import pytest

import motion_arith_dec_cases as AC
import motion_arith_dec_ref as A
import noarith_twin as T
from schroedinger_amd import MV_DTYPE

M32 = 0xffffffff
INTACT, LIMITS, HOSTILE, WITNESS = AC.all_cases()


def test_the_device_table_is_the_reference_table():
    """motion_arith_dec.hip states the 256 numbers again (a __constant__ array belongs to one file): they are
    tests/golden/arith_lut.json's, and arith_dec.hip's."""
    import stream_lib as S
    csrc = os.path.join(os.path.dirname(S.GOLDEN), "..", "schroedinger_amd", "csrc")
    tables = []
    for name, symbol in (("motion_arith_dec.hip", "kMaLut"), ("arith_dec.hip", "kAdLut")):
        body = re.search(r"%s\[256\] = \{(.*?)\};" % symbol, open(os.path.join(csrc, name)).read(), re.S).group(1)
        tables.append([int(v) for v in body.replace("\n", " ").split(",") if v.strip()])
    assert tables[0] == tables[1] == json.load(open(os.path.join(S.GOLDEN, "arith_lut.json")))["arith_lut"]


# ---- on the stream -------------------------------------------------------------------------------------------------------------

def test_all_96_inter_pictures_of_the_stream():
    """The motion data re-serialised from Picture.motion_buffers (per section: uint length, sync, payload) is byte for byte
    a slice of the parse unit's payload, so what the device tests feed are the stream's own bytes.  The restatement's field
    is dirac_stream's, its per-section values are the recorded ones, section_bytes are the stream's lengths, and the result
    is clean: nothing truncated, overran, long or unverified.  not_consumed is NOT part of clean: the reference's encoder
    often ends a section a byte behind the decoder's last fetch (offset == length - 1, never further back), which is the
    condition of the reference's own debug message at schrodecoder.c:2594."""
    pictures = A.stream_pictures()
    recs = list(T.motion_pictures())
    assert len(pictures) == len(recs) == 96
    behind = 0
    for (pic, payload, data), rec in zip(pictures, recs):
        assert pic.number == rec["number"]
        assert payload.count(data) == 1, pic.number
        log = [[] for _ in range(9)]
        field, result = A.decode(data, rec["nbx"], rec["nby"], rec["num_refs"], 0, log)
        assert field.tobytes() == rec["mv"].tobytes(), pic.number
        assert log == rec["log"], pic.number
        lengths = [0 if b is None else len(b) for b in pic.motion_buffers]
        assert result["section_bytes"] == lengths and result["bytes"] == len(data)
        assert result["section_units"] == [len(v) if s != 1 else len(v) // (1 + (rec["num_refs"] > 1)) for s, v in enumerate(rec["log"])]
        assert (result["truncated"], result["overran"], result["long_codes"], result["unverified"], result["first_unverified"]) == (0, 0, 0, 0, -1)
        for s in range(9):
            if pic.motion_buffers[s] is not None:
                assert lengths[s] - 1 <= result["section_offset"][s] <= lengths[s] + 6, (pic.number, s)
                assert bool(result["not_consumed"] >> s & 1) == (result["section_offset"][s] == lengths[s] - 1)
        behind += bool(result["not_consumed"])
    assert behind        # (the debug message's condition does occur on the reference's own stream)


@pytest.mark.parametrize("number", [3, 1, 41])
def test_phased_form_on_stream_pictures(number):
    rec = next(T.motion_pictures(numbers={number}))
    data = A.stream_motion(number)
    args = (data, rec["nbx"], rec["nby"], rec["num_refs"], 0)
    field, result = A.decode_phased(*args)
    assert field.tobytes() == rec["mv"].tobytes() and result == A.decode(*args)[1]


# ---- the two forms ---------------------------------------------------------------------------------------------------------------

def test_serial_and_phased_agree_on_everything_small():
    n = 0
    for case in INTACT + LIMITS + HOSTILE:
        if case[2] * case[3] > AC.SMALL:
            continue
        a, b = A.decode(*case[1:6]), A.decode_phased(*case[1:6])
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1], case[0]
        n += 1
    assert n > 200


# ---- by hand ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_refs", [1, 2])
def test_the_empty_input(num_refs):
    """Every coder starts at code 0xffffffff under range 0xffff0000.  code - range = 0xffff >= 0 holds through every bin that
    decides 1 (both lose range_x_prob) and every shift (a 1 comes in), so EVERY bin is 1: a split residual is 0 in one bin,
    a vector or DC residual is 0 in one bin, and a mode bin is 1 -- the modes are not 0: the top-left unit's is all ones,
    and a unit whose prediction is all ones gets 0.  8 x 8: superblocks (0, 0) and (1, 1) have the mode, (1, 0) and (0, 1),
    which predict it from one neighbour, have 0; the vectors predict 0 and the DCs predict 0."""
    field, result = A.decode(b"", 8, 8, num_refs, 0)
    ones = 3 if num_refs == 2 else 1
    flags = field["flags"].reshape(8, 8)
    assert (flags[:4, :4] == ones).all() and (flags[4:, 4:] == ones).all() and (flags[:4, 4:] == 0).all() and (flags[4:, :4] == 0).all()
    assert not field["v"].any() and not field["metric"].any() and not field["chroma_metric"].any()
    two = 2 if num_refs == 2 else 0
    assert result["section_units"] == [4, 4, 2, 2, two, two, 2, 2, 2]
    assert result["section_bins"] == [4, 4 * num_refs, 2, 2, two, two, 2, 2, 2]
    assert result["section_bytes"] == [0] * 9 and result["bytes"] == 0
    assert (result["truncated"], result["not_consumed"], result["long_codes"], result["unverified"]) == (0, 0, 0, 0)
    # one bin per coder (4 x 4): nothing has been shifted in, the offset is the fresh coder's
    field, result = A.decode(b"", 4, 4, 1, 0)
    assert result["section_offset"] == [3, 3, 3, 3, 0, 0, 3, 3, 3] and result["section_bins"] == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert result["overran"] == 0           # 3 <= 0 + 6
    assert A.decode_phased(b"", 4, 4, 1, 0)[1] == result


@pytest.mark.parametrize("num_refs", [1, 2])
@pytest.mark.parametrize("split", [0, 1, 2])
def test_one_superblock(split, num_refs):
    """4 x 4.  The split residual is the split.  The first unit's mode residual is all ones, every later unit predicts that
    mode and has residual 0.  The first unit's vectors are (5, -3) and (7, 2); every later unit predicts them -- from one
    neighbour itself, from two equal ones their mean, from three the median -- and has residual 0.  Bins: a uint of v takes
    2 n + 1 with n = bit_length (v + 1) - 1, a non-zero sint one more."""
    units = 4 ** split
    nbits = num_refs
    log = [[split], [1] * nbits + [0] * (nbits * (units - 1)), [5] + [0] * (units - 1), [-3] + [0] * (units - 1)]
    log += [[7] + [0] * (units - 1), [2] + [0] * (units - 1)] if num_refs == 2 else [[], []]
    log += [[], [], []]
    data = A.write(log, num_refs)
    field, result = A.decode(data, 4, 4, num_refs, 0)
    want = np.zeros(16, MV_DTYPE)
    want["flags"] = (3 if num_refs == 2 else 1) | (split << 3)
    want["v"] = [5, 7, -3, 2] if num_refs == 2 else [5, 0, -3, 0]
    assert field.tobytes() == want.tobytes()
    two = units if num_refs == 2 else 0
    assert result["section_units"] == [1, units, units, units, two, two, 0, 0, 0]
    tail = units - 1
    assert result["section_bins"] == [1 if split == 0 else 3, nbits * units, 6 + tail, 6 + tail, (8 + tail) if two else 0, (4 + tail) if two else 0,
                                      0, 0, 0]
    assert result["section_offset"][6:] == [3, 3, 3] and (num_refs == 2 or result["section_offset"][4:6] == [0, 0])
    assert (result["truncated"], result["overran"], result["long_codes"], result["unverified"]) == (0, 0, 0, 0)
    phased = A.decode_phased(data, 4, 4, num_refs, 0)
    assert phased[0].tobytes() == field.tobytes() and phased[1] == result


def test_one_superblock_of_dc_blocks():
    """4 x 4 at split 2, every unit mode 0: the mode residuals are 0 (the prediction is 0 everywhere), the first unit's DCs
    are (10, -20, 30) and every later unit predicts them: one neighbour itself, two their rounded mean ((2 v + 1) >> 1 = v),
    three schro_divide3 (3 v + 1) = v for these three values."""
    log = [[2], [0] * 32, [], [], [], [], [10] + [0] * 15, [-20] + [0] * 15, [30] + [0] * 15]
    data = A.write(log, 2)
    field, result = A.decode(data, 4, 4, 2, 0)
    want = np.zeros(16, MV_DTYPE)
    want["flags"] = 2 << 3
    want["v"] = [10, -20, 30, 0]
    assert field.tobytes() == want.tobytes()
    assert result["section_units"] == [1, 16, 0, 0, 0, 0, 16, 16, 16]
    # 10: 11 = 1011b, n = 3: 7 bins and the sign; 20: 21 = 10101b, n = 4: 9 and the sign; 30: 31 = 11111b, n = 4
    assert result["section_bins"] == [3, 32, 0, 0, 0, 0, 8 + 15, 10 + 15, 10 + 15]
    assert result["unverified"] == 0


def test_a_section_of_length_0_among_others():
    case = next(c for c in LIMITS if c[0] == "a section of length 0 among others")
    base = AC.intact_by_name("12x12 mixed refs 2")
    field, result = AC.expected(case)
    intact = AC.expected(base)[1]
    assert result["section_bytes"][2] == 0 and result["section_bytes"][3:] == intact["section_bytes"][3:]
    # the empty section reads 0xff: every residual 0, a bin each; the others are asked what they were asked before
    assert result["section_units"] == intact["section_units"] and result["section_bins"][2] == result["section_units"][2] > 0
    assert result["section_bins"][:2] == intact["section_bins"][:2] and result["section_bins"][3:] == intact["section_bins"][3:]
    assert not result["overran"] >> 2 & 1 or result["section_offset"][2] > 6
    assert field.tobytes() != AC.expected(base)[0].tobytes()


# ---- the writer and the counters ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", INTACT, ids=lambda c: c[0])
def test_the_writer_round_trips(case):
    """Every intact field -- every encoder case, both reference counts, global motion -- comes back from its bytes, with
    nothing truncated, overran, long; the units are the field's values."""
    field, result = AC.expected(case)
    assert field.tobytes() == AC.field_of(case).tobytes()
    assert (result["truncated"], result["overran"], result["long_codes"]) == (0, 0, 0)
    log = A.values_of_field(field, *case[2:6])
    nbits = 1 + (case[4] > 1)
    assert result["section_units"][0] == len(log[0]) and result["section_units"][2:] == [len(v) for v in log[2:]]
    assert result["section_bins"][1] == len(log[1]) and (case[5] or result["section_units"][1] * nbits == len(log[1]))
    assert result["bytes"] == len(case[1])


def test_long_splits_and_the_mod_3_rule():
    """Residuals 2^32 (32 data bins) and 2^31 + 1 (31): both long.  The first is kept mod 2^32: bits = 2^32 + 1 -> 1, value 0,
    split (0 + 0) % 3 = 0 where (0 + 2^32) % 3 would be 1.  The second is exact: pred 0 (its left neighbour's split), (0 + 2^31
    + 1) % 3 = 0 as well (2^31 = 2 mod 3); the third superblock has residual 1 under a prediction of 0."""
    case = next(c for c in LIMITS if c[0] == "splits of 32 and 31 data bins")
    field, result = AC.expected(case)
    assert (1 << 32) % 3 == 1 and ((1 << 31) + 1) % 3 == 0
    splits = (field["flags"].reshape(8, 8)[::4, ::4] >> 3).tolist()
    assert splits == [[0, 0], [1, (0 + 0 + 1 + 1) // 3 % 3]]
    assert result["long_codes"] == 2 and result["section_bins"][0] == (2 * 32 + 1) + (2 * 31 + 1) + 3 + 1


def test_the_cap_of_30_data_bins():
    """-(2^30 + 5): bits = 2^30 + 6 has 30 data bins; the loop stops without a continuation bin and the next bin is the sign.
    (int16_t) (0 - 2^30 - 5) = -5; the residual behind it, 3, predicts from -5: -2."""
    case = next(c for c in LIMITS if c[0] == "a DC residual of 30 data bins")
    field, result = AC.expected(case)
    units = result["section_units"][6]
    assert result["section_bins"][6] == (60 + 1) + (5 + 1) + (units - 2) and result["long_codes"] == 0
    dcs = [int(v[0]) for v in field["v"]]
    assert dcs[0] == -5 and -2 in dcs and result["unverified"] == 0


def test_every_counter_has_witnesses():
    """Asserted from the restatement, each class non-empty (motion_arith_dec_cases.hostile): truncated, overran,
    not_consumed, long_codes, a DC outside -128 .. 127, a damaged payload that decodes to another field."""
    print(AC.describe())
    for key in ("truncated", "overran", "not_consumed", "long_codes", "unverified", "payload_damage_seen"):
        assert WITNESS[key] > 0, key
    cut = next(c for c in LIMITS if c[0] == "a payload that ends inside a code")
    r = AC.expected(cut)[1]
    s = max(range(9), key=lambda k: AC.expected(AC.intact_by_name("12x12 mixed refs 2"))[1]["section_bytes"][k])
    assert r["overran"] >> s & 1 and r["section_offset"][s] > r["section_bytes"][s] + 6
    for c in HOSTILE:
        r = AC.expected(c)[1]
        if "length past the input" in c[0]:
            assert r["truncated"] >> 8 & 1, c[0]
        if "cut: " in c[0]:
            assert r["bytes"] <= len(c[1])
        assert all(b <= M32 for b in r["section_bins"])


def test_a_filled_payload_costs_what_design_says():
    """A payload of zero bytes costs about 1277 bins a byte: FILL_MAX keeps a filled section a fraction of a
    second on the device."""
    worst = max(max(AC.expected(c)[1]["section_bins"]) for c in HOSTILE if "filled: " in c[0])
    assert worst <= 1500 * AC.FILL_MAX + 3000 + 16384
