"""CPU: the VLC restatements against data the REFERENCE produced -- the noarith twin of its own stream (tests/noarith_twin.py).

tests/motion_enc_ref.py, motion_dec_ref.py, noarith_enc_ref.py and noarith_dec_ref.py are what the four VLC kernels are
compared with; until here they were held by hand-derived byte strings and by round trips through each other.  The twin is
made without them from tests/golden/test_stream.drc: the residuals oracle/dirac_stream.py's arithmetic decoders yield --
under predictions the reference decoder's frame digests hold (tests/test_oracle_stream.py) -- as exp-Golomb codes.

PINNED by reference output, on all 96 inter and 4 intra pictures: the mode prediction, the vector prediction (none, one,
the mean of two, the median of three) and the DC prediction, the framing of the nine sections, the order of units at split
2, the exp-Golomb codes themselves; the transform data's headers, codeblock walk, zero flags and dequantisation for s16
with one quant index per sub-band; the intra DC prediction behind it.

NOT PINNED, because the stream has none of it (asserted below, so that a richer stream would say so): the split
prediction's mean (every split is 2, so every residual but the first is 0), the units of split 0 and split 1, sub-pel
vectors (mv_precision is 0), global motion, non-zero quant offsets, several codeblocks in sub-band 0 (where the encoder's
and the decoder's zero-flag rules part), s32 samples, codes of 31 or more data bits.  For those the restatements rest on
the hand-derived strings of tests/test_motion_enc_ref.py, test_motion_dec_ref.py, test_noarith_enc_ref.py and
test_noarith_dec_ref.py as before.

Measured, one CPU core: 46 s for the file -- 5 s for the motion data of the 96 pictures through both restatements, 40 s for
the pass over the 100 pictures' transform data (the stream's own decode, two writers, two decodes)."""
import numpy as np
import pytest

import motion_dec_ref as MD
import motion_enc_ref as ME
import noarith_dec_ref as ND
import noarith_enc_ref as NE
import noarith_twin as T
import oracle_lib as O

PATTERN = 0x2b67            # what the planes hold before the decoder writes them


# ---- motion data ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def motion():
    """Per inter picture (coded order): the twin record, the restated encoder's (bytes, result), the restated decoder's
    (field, result)."""
    out = []
    for rec in T.motion_pictures():
        args = (rec["nbx"], rec["nby"], rec["num_refs"], 0)
        out.append((rec, ME.encode(rec["mv"], *args), MD.decode(rec["motion"], *args)))
    return out


def test_motion_twin_is_the_restated_encoders_bytes(motion):
    assert len(motion) == 96
    for rec, (data, result), _ in motion:
        n = rec["number"]
        if data != rec["motion"]:
            first = next(i for i, (a, b) in enumerate(zip(data, rec["motion"])) if a != b) if len(data) == len(rec["motion"]) else -1
            raise AssertionError("picture %d: the restated encoder writes %d bytes, the twin has %d; first difference at byte %d, in %s"
                                 % (n, len(data), len(rec["motion"]), first, ME.section_of(rec["motion"], rec["num_refs"], max(first, 0))))
        assert result["unverified"] == 0 and result["asserted"] == 0, n
        assert result["bytes"] == len(rec["motion"]) and result["section_bytes"] == rec["section_bytes"], n
        assert result["section_units"] == [len(v) if s != 1 else len(v) // rec["num_refs"] for s, v in enumerate(rec["log"])], n


def test_motion_twin_decodes_to_the_streams_field(motion):
    for rec, _, (field, result) in motion:
        n = rec["number"]
        assert field.tobytes() == ME.canonical(rec["mv"]).tobytes(), n
        assert result["bytes"] == len(rec["motion"]) and result["section_bytes"] == rec["section_bytes"], n
        assert (result["truncated"], result["overran"], result["not_consumed"], result["long_codes"], result["unverified"]) == (0, 0, 0, 0, 0), n
        assert result["first_unverified"] == -1, n


def motion_statistics(rec):
    flags, v = rec["mv"]["flags"], rec["mv"]["v"].astype(np.int64)
    mode = flags & 3
    used = np.concatenate([np.abs(v[(mode & 1) != 0][:, [0, 2]]).ravel(), np.abs(v[(mode & 2) != 0][:, [1, 3]]).ravel()])
    return dict(modes=[int((mode == m).sum()) for m in range(4)], vmax=int(used.max(initial=0)), nbytes=len(rec["motion"]))


def test_what_the_streams_motion_data_pins_and_the_eight_pictures(motion):
    """The stream's motion data is what the module's docstring says, and noarith_twin.MOTION_EIGHT names the pictures it is
    commented to name."""
    recs = [rec for rec, _, _ in motion]
    stats = {rec["number"]: motion_statistics(rec) for rec in recs}
    order = [rec["number"] for rec in recs]
    assert order == T.motion_numbers() and order[-1] == 98
    for rec in recs:
        flags, st = rec["mv"]["flags"], stats[rec["number"]]
        assert (rec["blocks"], rec["nbx"], rec["nby"], rec["mv_precision"]) == ((12, 12, 8, 8), 40, 32, 0)
        assert ((flags >> 3) == 2).all()                                # split 2, no upper bits
        assert not (flags & 4).any()                                    # no global motion
        assert rec["log"][0][0] == 2 and not any(rec["log"][0][1:])     # ... so the split prediction never has to take a mean
        assert st["modes"][0] in (90, 91) and st["vmax"] <= 37
        if rec["num_refs"] == 1:
            assert st["modes"][2] == st["modes"][3] == 0 and st["modes"][1] > 0
        else:
            assert all(st["modes"])                                     # modes 0 .. 3 all occur
    assert sorted({rec["num_refs"] for rec in recs}) == [1, 2]
    assert max(st["vmax"] for st in stats.values()) >= 16

    chosen = []

    def first(want, among=order):
        chosen.append(next(n for n in among if want(n) and n not in chosen))

    def extreme(key, pick):
        best = pick(stats[n][key] if isinstance(key, str) else key(n) for n in order)
        first(lambda n: (stats[n][key] if isinstance(key, str) else key(n)) == best)

    by_number = {rec["number"]: rec for rec in recs}
    first(lambda n: by_number[n]["num_refs"] == 1)
    first(lambda n: by_number[n]["num_refs"] == 2)
    extreme(lambda n: stats[n]["modes"][2], max)
    extreme(lambda n: stats[n]["modes"][3], max)
    extreme("vmax", max)
    extreme("nbytes", max)
    extreme("nbytes", min)
    chosen.append(order[-1])
    assert chosen == T.MOTION_EIGHT and len(set(chosen)) == 8
    assert T.FIRST_TWELVE[1:] == order[:11]


# ---- transform data ---------------------------------------------------------------------------------------------------------

def decoded(data, rec, compat):
    """The s16 planes a VLC decoder in state `compat` makes of `data` over planes that held PATTERN, as the stream's decoder
    leaves them -- the LL band of an intra picture DC-predicted --, and the result."""
    P = rec["twin"]
    planes = [np.full(shape, PATTERN, np.int16) for shape in (P["iwt"][0], P["iwt"][1], P["iwt"][1])]
    result = ND.decode_transform_data(data, planes, None, P["depth"], P["horiz_cb"], P["vert_cb"], P["cb_mode"], P["is_intra"], compat)
    if P["is_intra"]:
        for p in planes:
            ll = NE.subband(p, P["depth"], 0)
            ll[...] = O.dc_predict(ll)
    return planes, result


def clean(result, nbytes):
    return (result["error"], result["truncated"], result["not_consumed"], result["overran"], result["long_codes"], result["clamped_quant"]) \
        == (0, 0, 0, 0, 0, 0) and result["bytes_read"] == nbytes


@pytest.fixture(scope="module")
def transform():
    """One pass over the 100 pictures (the planes are not kept): per picture what the tests below assert."""
    facts = []
    for rec in T.pictures():
        assert not rec["zero_residual"]
        P = rec["twin"]
        f = dict(number=rec["number"], num_refs=rec["num_refs"], wavelet=P["wavelet"], depth=P["depth"], cb_mode=P["cb_mode"],
                 counts0=(P["horiz_cb"][0], P["vert_cb"][0]), compat=P["compat"], dtype=rec["coeffs"][0].dtype,
                 qmax=max(int(np.abs(q).max()) for q in rec["quant"]))
        # the twin, read by a decoder in the stream decoder's state
        planes, result = decoded(rec["transform"], rec, P["compat"])
        f["twin_equal"] = all(np.array_equal(a, b) for a, b in zip(planes, rec["coeffs"]))
        f["twin_clean"] = clean(result, len(rec["transform"]))
        f["headers"] = all(int(result["subband_quant_index"][k, i]) == rec["quant_indices"][k][i] for k in range(3)
                           for i in range(1 + 3 * P["depth"]) if result["subband_length"][k, i])
        # the encoder's restated writer on the same quant planes, as s16 like the device's: its rules are the decoder's where
        # sub-band 0 has one codeblock and the decoder is in compat mode
        quant = [q.astype(np.int16) for q in rec["quant"]]
        f["s16_quant"] = all(np.array_equal(a, b) for a, b in zip(quant, rec["quant"]))
        data, bits, false_zero = NE.encode_transform_data(quant, P["depth"], P["horiz_cb"], P["vert_cb"], P["cb_mode"], rec["quant_indices"])
        planes, result = decoded(data, rec, 1)
        f["encoder_equal"] = all(np.array_equal(a, b) for a, b in zip(planes, rec["coeffs"]))
        f["encoder_clean"] = clean(result, len(data)) and not any(false_zero.values())
        # ... so that for a decoder in compat mode the two writers give the same bytes
        f["encoder_bytes"] = data == rec["transform"] if P["compat"] else data != rec["transform"]
        facts.append(f)
    return facts


def failing(facts, key):
    return [f["number"] for f in facts if not f[key]]


def test_transform_twin_decodes_to_the_streams_coefficients(transform):
    assert [f["number"] for f in transform][:12] == T.FIRST_TWELVE and len(transform) == 100
    assert failing(transform, "twin_equal") == []
    assert failing(transform, "twin_clean") == [] and failing(transform, "headers") == []


def test_the_encoders_restated_writer_agrees(transform):
    """noarith_enc_ref.encode_transform_data differs from the decoder's rules only where sub-band 0 has several codeblocks:
    in this stream it never has."""
    assert all(f["counts0"] == (1, 1) for f in transform)
    assert failing(transform, "encoder_equal") == [] and failing(transform, "encoder_clean") == []
    assert failing(transform, "encoder_bytes") == []
    # the stream is an early encoder's: its first picture switches the compat mode on, and it stays on
    assert [f["compat"] for f in transform] == [0] + [1] * 99


def test_what_the_streams_transform_data_pins(transform):
    intra = [f["number"] for f in transform if f["num_refs"] == 0]
    assert len(intra) == 4 and intra[0] == 0
    for f in transform:
        assert (f["wavelet"], f["depth"]) == ((0, 4) if f["num_refs"] == 0 else (1, 4)), f["number"]
        assert f["cb_mode"] == 1 and f["dtype"] == np.int16 and f["s16_quant"], f["number"]
        # (one quant index per sub-band: noarith_twin.transform_twin asserts it of every codeblock record)
        assert 0 < f["qmax"] <= 268, f["number"]
    assert max(f["qmax"] for f in transform) >= 128             # values that take codes of 15 bits and more
