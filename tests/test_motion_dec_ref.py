"""CPU: tests/motion_dec_ref.py pinned -- hand-derived byte strings, the round trip through motion_enc_ref.encode, the serial
form against the wavefront form on every case and every damaged stream, the chunked code extraction against the serial
one."""
import numpy as np
import pytest

import motion_dec_cases as DC
import motion_dec_ref as D
import motion_enc_cases as MC
import motion_enc_ref as R
from schroedinger_amd import MV_DTYPE


def field_of(records):
    """records: per block (flags, v0, v1, v2, v3)."""
    f = np.zeros(len(records), MV_DTYPE)
    f["flags"] = [r[0] for r in records]
    f["v"] = [r[1:] for r in records]
    return f


def both(data, *geometry):
    a, b = D.decode(data, *geometry), D.decode_wavefront(data, *geometry)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1], (a[1], b[1])
    return a


def test_an_empty_stream():
    """No bytes: every header reads guard bits and gives length 0; every code is made of guard bits: split 0, mode residual
    1 (so mode 1, or 3 with two references), vector residual 0."""
    field, r = both(b"", 4, 4, 1, 0)
    assert field.tobytes() == field_of([(1, 0, 0, 0, 0)] * 16).tobytes()
    assert r == {"bytes": 0, "section_bytes": [0] * 9, "section_units": [1, 1, 1, 1, 0, 0, 0, 0, 0],
                 "section_bits": [1, 1, 1, 1, 0, 0, 0, 0, 0], "truncated": 0, "overran": 0b1111, "not_consumed": 0, "long_codes": 0,
                 "unverified": 0, "first_unverified": -1}
    field, r = both(b"", 8, 4, 2, 0)
    # the second superblock predicts mode 3 from its left neighbour and reads residual 3: mode 0, DCs of 0
    assert field.tobytes() == field_of(([(3, 0, 0, 0, 0)] * 4 + [(0, 0, 0, 0, 0)] * 4) * 4).tobytes()
    assert r["section_units"] == [2, 2, 1, 1, 1, 1, 1, 1, 1] and r["section_bits"] == [2, 4, 1, 1, 1, 1, 1, 1, 1]
    assert r["overran"] == 0x1ff


def test_sections_of_0x80_only():
    """Every section is the one byte 0x80 -- length 0 --, as the encoder writes an empty one: the field of the empty stream,
    and `bytes` is the stream's length."""
    for num_refs in (1, 2):
        n = 7 if num_refs == 1 else 9
        field, r = both(b"\x80" * n, 4, 4, num_refs, 0)
        assert field.tobytes() == both(b"", 4, 4, num_refs, 0)[0].tobytes()
        assert r["bytes"] == n and r["section_bytes"] == [0] * 9 and r["truncated"] == 0 and r["long_codes"] == 0
    # one byte short: the last header reads guard bits
    assert both(b"\x80" * 8, 4, 4, 2, 0)[1]["bytes"] == 8


# One superblock at each split.  A section is its length code on a byte of its own (0x80: length 0; uint 1 is 0 0 1, so one
# byte of payload is announced by 001 00000 = 0x20), then the payload.  Codes: uint 0 is 1, 1 is 001, 2 is 011; sint +1 is
# 0010, -1 is 0011, +2 is 0110, -2 is 0111.
L1 = b"\x20"                    # "one byte follows"
L2 = b"\x60"                    # uint 2 = 011: "two bytes follow"
L3 = b"\x08"                    # uint 3 = 00001
L4 = b"\x18"                    # uint 4 = 00011


def test_one_superblock_split_0():
    # one reference: split residual 0 (1.......), mode residual 1 (mode 1), x residual +2 (0110....), y residual -1 (0011....)
    data = L1 + b"\x80" + L1 + b"\x80" + L1 + b"\x60" + L1 + b"\x30" + b"\x80" * 3
    field, r = both(data, 4, 4, 1, 0)
    assert field.tobytes() == field_of([(1, 2, 0, -1, 0)] * 16).tobytes()
    assert r["bytes"] == len(data) == 11 and r["section_bytes"] == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert r["section_units"] == [1, 1, 1, 1, 0, 0, 0, 0, 0] and r["section_bits"] == [1, 1, 4, 4, 0, 0, 0, 0, 0]
    assert r["overran"] == 0 and r["not_consumed"] == 0 and r["truncated"] == 0
    # two references: mode residual 0 0 (mode 0): DCs +1, -2, 0
    data = L1 + b"\x80" + L1 + b"\x00" + b"\x80" * 4 + L1 + b"\x20" + L1 + b"\x70" + L1 + b"\x80"
    field, r = both(data, 4, 4, 2, 0)
    assert field.tobytes() == field_of([(0, 1, -2, 0, 0)] * 16).tobytes()
    assert r["section_units"] == [1, 1, 0, 0, 0, 0, 1, 1, 1] and r["section_bits"] == [1, 2, 0, 0, 0, 0, 4, 4, 1]


def test_one_superblock_split_1():
    # split residual 1 (001.....); four units.  One reference, modes 1 0 1 1: the predictions are 0, 1 (left), 1 (above),
    # majority (0, 1, 1) = 1, so the residuals are 1 1 0 0 (1100....).  Unit 0: x +1, y 0; unit 2 (below unit 0): predicted from
    # above (1, 0), x residual 0, y -1; unit 3: left (1, -1), above is DC, diagonal (1, 0): the mean of two, (1, 0) [(-1 + 0 + 1) >> 1],
    # residuals 0, 0: the y payload is 1 0011 1.. = 0x9c.  Unit 1: DC +1 0 0.
    data = L1 + b"\x20" + L1 + b"\xc0" + L1 + b"\x2c" + L1 + b"\x9c" + L1 + b"\x20" + L1 + b"\x80" + L1 + b"\x80"
    field, r = both(data, 4, 4, 1, 0)
    a, b, c, d = (1 | 8, 1, 0, 0, 0), (0 | 8, 1, 0, 0, 0), (1 | 8, 1, 0, -1, 0), (1 | 8, 1, 0, 0, 0)
    assert field.tobytes() == field_of([a, a, b, b] * 2 + [c, c, d, d] * 2).tobytes()
    assert r["section_units"] == [1, 4, 3, 3, 0, 0, 1, 1, 1] and r["section_bits"] == [3, 4, 6, 6, 0, 0, 4, 1, 1]
    assert r["overran"] == 0 and r["not_consumed"] == 0
    # two references: every unit mode 3 (residuals 11 00 00 00 = 0xc0), all vector residuals 0 (1111....)
    data = L1 + b"\x20" + L1 + b"\xc0" + (L1 + b"\xf0") * 4 + b"\x80" * 3
    field, r = both(data, 4, 4, 2, 0)
    assert field.tobytes() == field_of([(3 | 8, 0, 0, 0, 0)] * 16).tobytes()
    assert r["section_units"] == [1, 4, 4, 4, 4, 4, 0, 0, 0] and r["section_bits"] == [3, 8, 4, 4, 4, 4, 0, 0, 0]


def test_one_superblock_split_2():
    # split residual 2 (011.....); sixteen units, one reference, all mode 1: residual 1 for the first, 0 for the others (their
    # predictions are 1): 0x80 0x00; x residual +1 for the first, 0 after it (the prediction carries the 1 on): 0010 1111 1111 1111 111.....
    data = L1 + b"\x60" + L2 + b"\x80\x00" + L3 + b"\x2f\xff\xe0" + L2 + b"\xff\xff" + b"\x80" * 3
    field, r = both(data, 4, 4, 1, 0)
    assert field.tobytes() == field_of([(1 | 16, 1, 0, 0, 0)] * 16).tobytes()
    assert r["section_units"] == [1, 16, 16, 16, 0, 0, 0, 0, 0] and r["section_bits"] == [3, 16, 19, 16, 0, 0, 0, 0, 0]
    assert r["overran"] == 0 and r["not_consumed"] == 0
    # two references, all DC (mode residuals 0): 32 zero bits; DC Y residual -1 first, then 0
    data = L1 + b"\x60" + L4 + b"\x00" * 4 + b"\x80" * 4 + (L3 + b"\x3f\xff\xe0") + (L2 + b"\xff\xff") * 2
    field, r = both(data, 4, 4, 2, 0)
    assert field.tobytes() == field_of([(16, -1, 0, 0, 0)] * 16).tobytes()
    assert r["section_units"] == [1, 16, 0, 0, 0, 0, 16, 16, 16] and r["section_bits"][1] == 32 and r["section_bits"][6] == 19


def test_the_wrap_rule_and_long_codes():
    """31 data bits: v = 2^31 | data, the value v - 1; 32 data bits: the leading 1 is shifted out; a signed code with data
    bits always has a sign bit, even where the value wraps to 0."""
    bits = "01" * 31 + "1"
    r = D.Bits(DC.to_bytes(bits))
    assert r.code(False) == (1 << 32) - 1 - 1 and r.longs == 1 and r.pos == 63
    bits = "00" + "01" * 31 + "1" + "1"
    r = D.Bits(DC.to_bytes(bits))
    assert r.code(True) == (-(0x7fffffff - 1)) & 0xffffffff and r.pos == 66 and r.longs == 1
    r = D.Bits(DC.to_bytes("00" * 32 + "1" + "0" + "1"))
    assert r.code(True) == 0xffffffff and r.pos == 66      # v wrapped to 0: the value is -1 mod 2^32, its sign bit is read
    r = D.Bits(DC.to_bytes("00" * 30 + "1"))
    assert r.code(False) == (1 << 30) - 1 and r.longs == 0
    # a split residual of 2^32 - 2 on a prediction of 0: (0 + 4294967294) % 3 = 2 without a second wrap
    assert ((1 << 32) - 2) % 3 == 2
    data = DC.assemble([DC.to_bytes("01" * 31 + "1")] + [b""] * 8, 1)
    field, res = both(data, 4, 4, 1, 0)
    assert (field["flags"] >> 3 == 2).all() and res["long_codes"] == 1


@pytest.mark.parametrize("case", [c for c in MC.all_cases() if c[6]], ids=lambda c: c[0])
def test_round_trip(case):
    name, field, nbx, nby, num_refs, hg, _ = case
    data, enc = R.encode(field, nbx, nby, num_refs, hg)
    f = D.decode if nbx * nby <= 5000 else D.decode_wavefront
    got, r = f(data, nbx, nby, num_refs, hg)
    assert got.tobytes() == R.canonical(field).tobytes()
    assert got.tobytes() == R.decode(data, nbx, nby, num_refs, hg).tobytes()
    assert r["bytes"] == len(data) and r["section_bytes"] == enc["section_bytes"] and r["section_units"] == enc["section_units"]
    assert r["truncated"] == r["overran"] == r["not_consumed"] == r["long_codes"] == 0
    # in a decoded field schro_motion_verify can only object to a DC outside -128 .. 127 (the extremes)
    wide = np.flatnonzero(((got["flags"] & 3) == 0) & ((got["v"][:, :3] < -128) | (got["v"][:, :3] > 127)).any(axis=1))
    assert r["unverified"] == wide.size and r["first_unverified"] == (wide[0] if wide.size else -1)
    assert (wide.size > 0) == name.startswith("extremes")
    assert all(0 <= 8 * b - n < 8 for b, n in zip(r["section_bytes"], r["section_bits"]))


def small():
    intact, limits, damaged, _ = DC.all_cases()
    return [c for c in intact + limits + damaged if c[2] * c[3] <= DC.SMALL]


def test_serial_is_wavefront_on_everything_small():
    cases = small()
    assert len(cases) > 150
    for c in cases:
        a, b = D.decode(*c[1:6]), D.decode_wavefront(*c[1:6])
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1], (c[0], a[1], b[1])


def test_the_witnesses():
    w = DC.all_cases()[3]
    assert w["streams"] >= 4 * 40 and w["never_ending"] >= 1 and 2 * w["payload_damage_seen"] >= w["payload_damaged"]


def test_chunked_extraction_is_serial_extraction():
    """Seeded bit strings, signed and unsigned, dense and sparse in code starts: the same values by index, and chunks are
    entered in every state of the machine."""
    entered = {True: set(), False: set()}
    for seed in range(60):
        rng = np.random.default_rng(7000 + seed)
        n = int(rng.integers(1, 200))
        p = (0.5, 0.15, 0.85, 0.02)[seed % 4]
        payload = np.packbits(rng.random(8 * n) < p).tobytes()
        for signed in (False, True):
            for ceiling in (3, 1 << 20):
                serial = D.Section(payload, signed, ceiling)
                got, states = D.extract_chunked(payload, signed, ceiling)
                assert len(got) >= len(serial.values) and got == [serial.value(i) for i in range(len(got))], (seed, signed)
                entered[signed] |= states
    assert entered[True] == {D.A, D.D, D.F, D.S} and entered[False] == {D.A, D.D, D.F}


def test_summaries_compose_from_every_entry_state():
    for seed in range(20):
        payload = np.random.default_rng(7100 + seed).integers(0, 256, 16, dtype=np.uint8).tobytes()
        for signed in (False, True):
            r = D.Bits(payload)
            first, then = D.summary(r, 0, signed), D.summary(r, 1, signed)
            for state in range(4):
                s, done = state, 0
                r.pos = 0
                for _ in range(128):
                    s, d = D.step(s, r.bit(), signed)
                    done += d
                mid, a = first[state]
                end, b = then[mid]
                assert (end, a + b) == (s, done)
