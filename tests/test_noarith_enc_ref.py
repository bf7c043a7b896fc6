"""tests/noarith_enc_ref.py pinned without a device: hand-derived byte strings for the smallest pictures (each bit below
follows schropack.c:137-178 and schroencoder.c:4072-4192 by hand) and the round trip through the restated decoder."""
import numpy as np
import pytest

import noarith_enc_cases as NC
import noarith_enc_draws as ND
import noarith_enc_ref as ref


def test_bit_writer_codes():
    def bits(fn, v):
        p = ref.Pack()
        getattr(p, fn)(v)
        n = 8 * len(p.data) + (7 - p.shift)
        p.sync()
        return "".join("{:08b}".format(b) for b in p.data)[:n]
    assert bits("encode_uint", 0) == "1"
    assert bits("encode_uint", 1) == "001"
    assert bits("encode_uint", 2) == "011"
    assert bits("encode_uint", 5) == "01001"
    assert bits("encode_uint", 7) == "0000001"
    assert bits("encode_sint", 0) == "1"
    assert bits("encode_sint", 1) == "0010"
    assert bits("encode_sint", -2) == "0111"
    assert bits("encode_sint", 3) == "000010"
    # the code lengths of the contract: s16 1 .. 32 bits, s32 up to 64
    assert len(bits("encode_sint", 32767)) == 32 and len(bits("encode_sint", -32768)) == 32
    assert bits("encode_sint", -32768) == "0" * 28 + "0111"
    assert len(bits("encode_sint", (1 << 31) - 1)) == 64 and len(bits("encode_sint", (1 << 28) - 1)) == 58


def test_three_one_sample_components():
    """depth 0, three 1 x 1 components: 1 at quant index 5, 0, -2 at quant index 7.
    Y: sub-pack sint (1) = 0010 -> 20; header uint (1) uint (5) = 001 01001 -> 29.  U: uint (0) -> 80 after the sync.
    V: sub-pack sint (-2) = 0111 -> 70; header uint (1) uint (7) = 001 0000001 -> 20 40."""
    planes = [np.array([[v]], np.int16) for v in (1, 0, -2)]
    data, bits, stats = ref.encode_transform_data(planes, 0, [1], [1], 0, [[5], [0], [7]])
    assert data == bytes.fromhex("2920" "80" "204070")
    assert bits[:, 0].tolist() == [16, 0, 24] and not bits[:, 1:].any()         # trap (b): header + payload, or 0
    assert stats == {"false_zero_codeblocks": 0, "false_zero_subbands": 0}


@pytest.mark.parametrize("mode,hl", [(1, "24a6"), (0, "248c")])
def test_flags_and_quant_offset(mode, hl):
    """depth 1, 4 x 2 in 4:4:4, (1, 1) codeblocks in the LL band and (2, 1) above.  Y = [[3, 0, 0, -1], [0, 0, 0, 0]].
    LL (3, 0), one codeblock, no flags: 000010 1 -> 0a; header uint (1) uint (0) = 001 1 -> 30.
    HL (0, -1), quant index 1: bit (1) for the zero codeblock; bit (0), [sint (0) = 1 when codeblock_mode_index is 1,]
    sint (-1) = 0011: 1 0 1 0011 -> a6, or 1 0 0011 -> 8c; header 001 001 -> 24.  Everything else: 80."""
    y = np.array([[3, 0, 0, -1], [0, 0, 0, 0]], np.int16)
    planes = [y, np.zeros_like(y), np.zeros_like(y)]
    q = [[0, 1, 2, 3]] * 3
    data, bits, stats = ref.encode_transform_data(planes, 1, [1, 2], [1, 1], mode, q)
    assert data == bytes.fromhex("300a" + hl + "8080" + "80" * 8)
    assert bits[0, :4].tolist() == [16, 16, 0, 0]
    got, indices, used = ref.decode_transform_data(data, [(2, 4)] * 3, np.int16, 1, [1, 2], [1, 1], mode)
    assert used == len(data) and all(np.array_equal(a, b) for a, b in zip(got, planes))
    assert indices[0][1].tolist() == [[1, 1]] and indices[0][2] is None


def test_all_zero_pictures():
    for case in (NC.BY_NAME["s16-zero-d2"], NC.BY_NAME["s32-zero-d6"]):
        data, bits, stats = case.expected()
        assert data == b"\x80" * (3 * case.nsub) and len(data) <= 57 and not bits.any()


def test_s16_zero_test_wraps():
    """Trap (a) at its smallest: the row (-32768, -32768) as a whole sub-band.  On s16 the sum wraps to 0 and the sub-band
    is one 1-bit; on s32 the same values are written: header uint (8) uint (0) = 0000011 1 -> 07, each value 28 zeros 0111."""
    for dtype, want, fz in ((np.int16, "808080", 1), (np.int32, "07" + "00000007" * 2 + "8080", 0)):
        planes = [np.array([[-32768, -32768]], dtype), np.zeros((1, 2), dtype), np.zeros((1, 2), dtype)]
        data, bits, stats = ref.encode_transform_data(planes, 0, [1], [1], 0, [[0]] * 3)
        assert data == bytes.fromhex(want)
        assert stats["false_zero_subbands"] == fz and bits[0, 0] == (0 if fz else 72)


def test_trap_cases_are_what_they_claim():
    data, bits, stats = NC.BY_NAME["s16-trap-codeblock"].expected()
    assert stats == {"false_zero_codeblocks": 1, "false_zero_subbands": 0} and bits[0, 1] > 0
    case = NC.BY_NAME["s16-trap-subband"]
    data, bits, stats = case.expected()
    assert stats == {"false_zero_codeblocks": 0, "false_zero_subbands": 1} and bits[0, 2] == 0 and bits[0, 1] > 0
    hc, vc = case.counts(2)
    assert not any(ref.is_zero(ref.get_codeblock(case.band(0, 2), x, 0, hc, vc)) for x in range(2))


def roundtrip(case):
    data, bits, stats = case.expected()
    shapes = [(h, w) for w, h in case.sizes]
    got, indices, used = ref.decode_transform_data(data, shapes, case.dtype, case.depth, case.hc, case.vc, case.mode)
    assert used == len(data)
    for k in range(3):
        for i in range(case.nsub):
            if indices[k][i] is not None:
                assert (indices[k][i] == case.qidx[k][i]).all()
                assert bits[k, i] > 0
            else:
                assert bits[k, i] == 0
    return all(np.array_equal(a, b) for a, b in zip(got, case.planes))


@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c.name)
def test_round_trip_of_the_cases(case):
    """encode -> decode gives back every value, except where the s16 zero test called non-zero values zero."""
    data, bits, stats = case.expected()
    same = roundtrip(case)
    assert same == (stats["false_zero_codeblocks"] + stats["false_zero_subbands"] == 0)


def test_round_trip_of_all_draws():
    kinds = set()
    for case in ND.DRAWS:
        data, bits, stats = case.expected()
        assert stats == {"false_zero_codeblocks": 0, "false_zero_subbands": 0}, case.name
        assert roundtrip(case), case.name
        assert max(int(np.abs(p.astype(np.int64)).max()) for p in case.planes) <= ND.MAX_ABS
        kinds.add((case.dtype.itemsize, case.depth > 0, case.mode))
    assert len(kinds) == 8      # both sample sizes, depth 0 and deeper, both codeblock modes


def test_round_trip_of_the_deep_draws():
    """Depths 4 .. 6: every (depth, sample size, codeblock mode) once, every one with coded sub-bands in every component."""
    kinds = set()
    for case in ND.DEEP_DRAWS:
        data, bits, stats = case.expected()
        assert stats == {"false_zero_codeblocks": 0, "false_zero_subbands": 0}, case.name
        assert roundtrip(case), case.name
        assert max(int(np.abs(p.astype(np.int64)).max()) for p in case.planes) <= ND.MAX_ABS
        assert all(np.asarray(bits)[k].any() for k in range(3)), case.name
        kinds.add((case.depth, case.dtype.itemsize, case.mode))
    assert kinds == {(d, b, m) for d in ND.DEEP_DEPTHS for b in (2, 4) for m in (0, 1)} and len(ND.DEEP_DRAWS) == len(kinds)
    # the first 24 draws are what they were before the deep ones came
    assert [c.depth for c in ND.DRAWS] == [(n >> 2) % 4 for n in range(ND.NDRAWS)]
