"""tests/noarith_dec_ref.py pinned without a device: hand-derived byte strings for the smallest pictures (each bit below
follows schrounpack.c:177-245 and schrodecoder.c:2939-2987, :3279-3449 by hand), the writer -> decoder identity on every
case, the chunk model against serial decoding, and the encoder's restatement decoded where the two rule sets agree."""
import numpy as np
import pytest

import noarith_dec_cases as DC
import noarith_dec_ref as ref
import noarith_enc_cases as NC
import noarith_enc_ref as enc


def decode(hexbytes, shapes, depth, hc, vc, mode, compat, intra=0, dtype=np.int16):
    coeffs = [np.full(s, 99, dtype) for s in shapes]
    quant = [np.full(s, 99, dtype) for s in shapes]
    result = ref.decode_transform_data(bytes.fromhex(hexbytes), coeffs, quant, depth, hc, vc, mode, intra, compat)
    return coeffs, quant, result


def test_bit_reader_codes():
    def sint(bits):
        r = ref.Reader(b"", 0)
        r.bits, r.nbits = bits + "1" * 72, len(bits)
        return ref.s32(r.decode_sint32()), r.pos, r.long_codes
    assert sint("1") == (0, 1, 0) and sint("0010") == (1, 4, 0) and sint("0111") == (-2, 4, 0) and sint("000010") == (3, 6, 0)
    assert sint("0" * 28 + "0111") == (-32768, 32, 0)
    # cut codes end on guard bits: data 1, follow 1, sign 1
    assert sint("0") == (-2, 4, 0) and sint("00") == (-1, 4, 0) and sint("000") == (-4, 6, 0) and sint("") == (0, 1, 0)
    # 30 data bits: the longest code the reference defines; 31 and more: v mod 2^32, counted
    assert sint("01" * 30 + "10") == ((1 << 31) - 2, 62, 0)
    assert sint("01" * 31 + "10") == (-2, 64, 1)          # v = 2^32 - 1, magnitude 2^32 - 2: as int32, -2
    assert sint("00" * 32 + "11") == (1, 66, 1)           # v = 2^32 mod 2^32 = 0, magnitude 2^32 - 1, negated: 1


def test_three_one_sample_components():
    """depth 0, three 1 x 1 components, mode 0.  Y: header uint (1) uint (5) = 001 01001 -> 29, payload sint (1) = 0010 -> 20.
    U: uint (0) -> 80.  V: header uint (1) uint (7) = 001 0000001 -> 20 40, payload sint (-2) = 0111 -> 70.
    Quant factor 10 / offset_3_8 4 at index 5: (4 + 10 + 2) >> 2 = 4; factor 13 / offset 5 at index 7: (5 + 26 + 2) >> 2 = 8."""
    coeffs, quant, r = decode("2920" "80" "204070", [(1, 1)] * 3, 0, [1], [1], 0, 0)
    assert [int(q[0, 0]) for q in quant] == [1, 0, -2] and [int(c[0, 0]) for c in coeffs] == [4, 0, -8]
    assert r["bytes_read"] == 6 and r["subband_length"][:, 0].tolist() == [1, 0, 1] and r["subband_quant_index"][:, 0].tolist() == [5, 0, 7]
    assert (r["error"], r["truncated"], r["not_consumed"], r["overran"], r["long_codes"], r["clamped_quant"]) == (0,) * 6
    # intra: offset_1_2 is 5 and 7: (5 + 10 + 2) >> 2 = 4, (7 + 26 + 2) >> 2 = 8
    assert [int(c[0, 0]) for c in decode("292080204070", [(1, 1)] * 3, 0, [1], [1], 0, 0, intra=1)[0]] == [4, 0, -8]


def test_one_by_one_band_has_an_offset_unless_compat():
    """depth 0, Y 2 x 1 with one codeblock, mode 1.  Header uint (2) uint (3) = 011 00001 -> 61; payload sint (+2) = 0110,
    sint (1) = 0010, sint (0) = 1 -> 62 80.  Not compat: index 3 + 2 = 5, values (1, 0), 9 bits read.  Compat: no offset,
    values (2, 1) at index 3 (factor 7, offset 3: (3 + 14 + 2) >> 2 = 4, (3 + 7 + 2) >> 2 = 3), 8 bits read."""
    shapes = [(1, 2)] * 3
    coeffs, quant, r = decode("61" "6280" "80" "80", shapes, 0, [1], [1], 1, 0)
    assert quant[0].tolist() == [[1, 0]] and coeffs[0].tolist() == [[4, 0]] and r["compat_quant_offset"] == 0
    assert r["subband_quant_index"][0, 0] == 3 and r["not_consumed"] == 0 and r["bytes_read"] == 5
    coeffs, quant, r = decode("61" "6280" "80" "80", shapes, 0, [1], [1], 1, 1)
    assert quant[0].tolist() == [[2, 1]] and coeffs[0].tolist() == [[4, 3]] and r["compat_quant_offset"] == 1
    # the compat test fires: header index 59 = uint 0101010 0001 -> 011 01010100001 -> 6a 84; 59 + 2 leaves 0 .. 60
    coeffs, quant, r = decode("6a84" "6280" "80" "80", shapes, 0, [1], [1], 1, 0)
    assert quant[0].tolist() == [[2, 1]] and r["compat_quant_offset"] == 1 and r["subband_quant_index"][0, 0] == 59 and r["clamped_quant"] == 0
    # mode 0 never has an offset and never fires
    assert decode("6a84628080" "80", shapes, 0, [1], [1], 0, 0)[2]["compat_quant_offset"] == 0


def test_two_by_one_band_zero_codeblock_and_offset():
    """depth 0, Y 4 x 1 in (2, 1) codeblocks, mode 1: sub-band 0 HAS zero flags (the decoder's rule).  Payload: bit (1) the
    first codeblock is zero; bit (0), sint (-3) = 000011, sint (2) = 0110, sint (-1) = 0011 -> 1 0 000011 0110 0011 = 83 63.
    Header uint (2) = 011, uint (10) = 0001011 -> 62 c0.  Index 10 - 3 = 7: factor 13, offset 5: (5 + 26 + 2) >> 2 = 8,
    (5 + 13 + 2) >> 2 = 5."""
    shapes = [(1, 4)] * 3
    coeffs, quant, r = decode("62c0" "8363" "80" "80", shapes, 0, [2], [1], 1, 0)
    assert quant[0].tolist() == [[0, 0, 2, -1]] and coeffs[0].tolist() == [[0, 0, 8, -5]]
    assert not coeffs[1].any() and not quant[2].any()
    assert r["subband_quant_index"][0, 0] == 10 and r["subband_length"][0, 0] == 2 and r["bytes_read"] == 6
    assert (r["not_consumed"], r["overran"], r["clamped_quant"]) == (0, 0, 0)
    # the writer gives the same bytes back
    data, used = ref.write_transform_data(quant, 0, [2], [1], 1, 0, [[10], [0], [0]], lambda k, i, x, y: -3)
    assert data.hex() == "62c0" "8363" "80" "80" and used[0, 0].tolist() == [[-1, 7]]
    # an offset that clamps: header index 2 = uint 011 -> 011 011 -> 6c: 2 - 3 -> 0
    r = decode("6c" "8363" "80" "80", shapes, 0, [2], [1], 1, 0)[2]
    assert r["clamped_quant"] == 1


def test_payload_one_byte_short():
    """The same band with a stated length of 1: header 001 0001011 -> 22 c0.  Payload 83 = 1 0 000011: the offset is read,
    both values are guard bits (0, 0); 10 bits read.  Payload 84 = 1 0 000100: the offset's code is cut in its third
    pair -- data 0, then guard bits: follow 1, sign 1 -> v = 1010b, -9, index 1; 12 bits read."""
    shapes = [(1, 4)] * 3
    for payload, bits in (("83", 10), ("84", 12)):
        coeffs, quant, r = decode("22c0" + payload + "80" "80", shapes, 0, [2], [1], 1, 0)
        assert not quant[0].any() and not coeffs[0].any() and r["bytes_read"] == 5
        assert (r["truncated"], r["not_consumed"], r["overran"], r["clamped_quant"]) == (0, 0, 0, 0), payload
    # the input itself one byte short: the stated 2 bytes reach past it
    coeffs, quant, r = decode("62c0" "83", shapes, 0, [2], [1], 1, 0)
    assert r["truncated"] == 1 and r["bytes_read"] == 6 and not quant[0].any() and r["subband_length"][0, 0] == 2


def test_header_error():
    """uint (61) = 62 = 111110b -> 0101010100 1: header 001 01010101001 -> 2a a4."""
    coeffs, quant, r = decode("80" "2aa4" "ff", [(1, 1)] * 3, 0, [1], [1], 0, 1)
    assert r["error"] == 1 and r["first_error"] == 19 and r["bytes_read"] == 3 and r["compat_quant_offset"] == 1
    assert all((p == 99).all() for p in coeffs + quant)


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_writer_decoder_identity(case):
    coeffs, quant, r = case.expected()
    assert all(np.array_equal(a, b) for a, b in zip(quant, case.planes))
    assert r["error"] == 0 and r["bytes_read"] == len(case.data) and r["truncated"] == 0 and r["overran"] == 0


def test_hostile_cases_are_defined():
    for case in DC.HOSTILE:
        coeffs, quant, r = case.expected()
        assert (coeffs is None) == bool(r["error"]), case.name


@pytest.mark.parametrize("seed", range(6))
def test_chunked_decoding_is_serial_decoding(seed):
    """Seeded random bit strings, with runs of zeros and ones, from each of the four entry states."""
    rng = np.random.default_rng(seed)
    for trial in range(12):
        n = int(rng.integers(1, 700))
        p = (0.5, 0.2, 0.8, 0.05)[trial % 4]
        bits = "".join("1" if v else "0" for v in rng.random(n) < p)
        for entry in (ref.A, ref.D, ref.F, ref.S):
            want = ref.serial_codes(bits, entry)
            got, sums = ref.chunked_codes(bits, entry)
            assert got[:len(want)] == want and not any(got[len(want):]), (seed, trial, entry)
            # the composition of all summaries is the summary of the whole string
            total = ref.IDENTITY
            for s in sums:
                total = ref.compose(total, s)
            padded = bits + "1" * (-len(bits) % ref.CHUNK)
            assert total == ref.summarize(padded)


def test_zero_flag_is_entering_at_the_sign_state():
    """A zero flag that reads 0 consumes one bit and counts one completion too many: the known correction."""
    assert ref.step(ref.S, 0) == (ref.A, 1) and ref.step(ref.S, 1) == (ref.A, 1)


AGREE = [c for c in NC.CASES if c.counts(0) == (1, 1)]


@pytest.mark.parametrize("case", AGREE, ids=lambda c: c.name)
def test_the_encoders_streams_decode_where_the_rules_agree(case):
    """Sub-band 0 with one codeblock, and mode 0 or compat on: noarith_enc_ref.encode_transform_data is what this decoder
    reads."""
    data, bits, stats = case.expected()
    coeffs = [np.zeros_like(p) for p in case.planes]
    quant = [np.zeros_like(p) for p in case.planes]
    r = ref.decode_transform_data(data, coeffs, quant, case.depth, case.hc, case.vc, case.mode, 0, 1 if case.mode else 0)
    assert r["error"] == 0 and r["bytes_read"] == len(data) and r["clamped_quant"] == 0
    # (magnitudes from 2^31 - 1 take 31 data bits: the device encoder writes them on s32, the value is right, and they count)
    assert r["long_codes"] == sum(int(np.count_nonzero(np.abs(p.astype(np.int64)) >= (1 << 31) - 1)) for p in quant)
    if stats["false_zero_codeblocks"] + stats["false_zero_subbands"] == 0:
        assert all(np.array_equal(a, b) for a, b in zip(quant, case.planes))
    for k in range(3):
        for i in range(case.nsub):
            assert (r["subband_length"][k, i] > 0) == (bits[k, i] > 0)
            if bits[k, i]:
                assert r["subband_quant_index"][k, i] == case.qidx[k][i]


def test_the_agreeing_cases_include_the_named_ones():
    names = {c.name for c in AGREE}
    for t in ("s16", "s32"):
        assert {t + "-32x16-d3-mixed-m1", t + "-16x8-d2-one-m0", t + "-window-64", t + "-window-65", t + "-wide-400"} <= names
