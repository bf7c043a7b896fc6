"""CPU: tests/motion_enc_ref.py, the restatement the device's motion data is held against, pinned by byte strings derived
by hand from schropack.c and by the round trip through the restated decoder."""
import numpy as np
import pytest

import motion_enc_cases as MC
import motion_enc_ref as R
from schroedinger_amd import MV_DTYPE, motion_encode_bound


def one_superblock(split, mode=1, v=(0, 0, 0, 0), ug=0):
    f = np.zeros(16, MV_DTYPE)
    f["flags"] = mode | (ug << 2) | (split << 3)
    f["v"] = v
    return f


def hexs(data):
    return " ".join("%02x" % b for b in data)


def test_split_0_mode_1_zero_vector():
    # split: uint (0) = "1" -> payload 80, length uint (1) = "001" -> 20.  modes: 1 ^ 0 = "1" -> 20 80.  x, y: sint (0) = "1"
    # -> 20 80 each.  three empty DC sections: 80 each.
    data, res = R.encode(one_superblock(0), 4, 4, 1, 0)
    assert hexs(data) == "20 80 20 80 20 80 20 80 80 80 80"
    assert res["section_bytes"] == [1, 1, 1, 1, 0, 0, 0, 0, 0] and res["section_units"] == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert res["unverified"] == 0 and res["first_unverified"] == -1 and res["asserted"] == 0


def test_split_2_sixteen_zero_blocks():
    # split: uint (2) = "011" -> 60.  modes: the first block 1 ^ 0, every other one 1 ^ 1: "1" and fifteen "0" -> 80 00 behind
    # uint (2) = 60.  vectors: sixteen "1" -> ff ff behind 60.
    data, res = R.encode(one_superblock(2), 4, 4, 1, 0)
    assert hexs(data) == "20 60 60 80 00 60 ff ff 60 ff ff 80 80 80"
    assert res["section_units"] == [1, 16, 16, 16, 0, 0, 0, 0, 0]


def test_a_dc_block_beside_a_vector_block():
    # One superblock at split 1, two references.  Units (0, 0) DC (10, -3, 0), (2, 0) mode 1 vector (2, -1), (0, 2) mode 3
    # vectors (1, 1) and (0, -2), (2, 2) DC (12, -3, 1).
    f = np.zeros((4, 4), MV_DTYPE)
    def put(y, x, mode, v):
        f["flags"][y:y + 2, x:x + 2] = mode | (1 << 3)
        f["v"][y:y + 2, x:x + 2] = v
    put(0, 0, 0, (10, -3, 0, 99))           # (the fourth slot is not a DC: never read)
    put(0, 2, 1, (2, 55, -1, 66))           # (dx[1], dy[1] are not named by mode 1)
    put(2, 0, 3, (1, 0, 1, -2))
    put(2, 2, 0, (12, -3, 1, 0))
    data, res = R.encode(f.reshape(-1), 4, 4, 2, 0)
    # split: residual (1 - 0 + 3) % 3 = 1, uint (1) = "001" -> 20; section 20 20.
    # modes, two bits a unit, low bit first.  (0, 0): 0 ^ 0 -> "00".  (2, 0): y == 0, prediction the left block (1, 0), a
    #   copy of unit (0, 0): mode 0; 1 ^ 0 -> "10".  (0, 2): x == 0, prediction block (0, 1): mode 0; 3 -> "11".  (2, 2):
    #   neighbours (1, 2) mode 3, (2, 1) mode 1, (1, 1) mode 0: majority 1; 0 ^ 1 = 1 -> "10".  "00101110" = 2e; 20 2e.
    # ref-1 x.  (2, 0): the left neighbour is DC, no prediction: sint (2): uint (2) = "011", sign "0".  (0, 2): above is DC:
    #   sint (1): uint (1) = "001", sign "0".  "0110 0010" = 62; 20 62.
    # ref-1 y.  (2, 0): sint (-1) = "0011".  (0, 2): sint (1) = "0010".  "00110010" = 32; 20 32.
    # ref-2 x.  (0, 2) only: sint (0) = "1" -> 80; 20 80.   ref-2 y: sint (-2) = "0111" -> 70; 20 70.
    # dc Y.  (0, 0): no neighbour: sint (10): 11 = 1011b, "0 0 0 1 0 1 1" = "0001011" and sign "0" -> "00010110".  (2, 2):
    #   neighbours (1, 2) mode 3, (2, 1) mode 1 do not count, (1, 1) is DC 10: one neighbour, prediction 10; sint (2) =
    #   "0110".  "00010110 0110" -> 16 60; length 2: uint (2) = "011" -> 60; 60 16 60.
    # dc U.  sint (-3): 4 = 100b, "0 0 0 0 1" and sign "1" -> "000011"; then -3 - (-3) = 0 -> "1".  "0000111" -> 0e; 20 0e.
    # dc V.  sint (0) = "1", then 1 - 0: sint (1) = "0010".  "10010" -> 90; 20 90.
    assert hexs(data) == "20 20 20 2e 20 62 20 32 20 80 20 70 60 16 60 20 0e 20 90"
    assert res["section_units"] == [1, 4, 2, 2, 1, 1, 2, 2, 2]
    assert res["unverified"] == 0
    back = R.decode(data, 4, 4, 2, 0)
    assert back.tobytes() == R.canonical(f.reshape(-1)).tobytes()


def test_global_motion_bits():
    # One superblock at split 1, one reference, have_global_motion.  (0, 0): mode 1, global; (2, 0): mode 1, vector (3, 0);
    # (0, 2): mode 0, DC 0; (2, 2): mode 1, global.
    f = np.zeros((4, 4), MV_DTYPE)
    def put(y, x, mode, ug, v):
        f["flags"][y:y + 2, x:x + 2] = mode | (ug << 2) | (1 << 3)
        f["v"][y:y + 2, x:x + 2] = v
    put(0, 0, 1, 1, (0, 0, 0, 0))
    put(0, 2, 1, 0, (3, 0, 0, 0))
    put(2, 0, 0, 0, (0, 0, 0, 0))
    put(2, 2, 1, 1, (0, 0, 0, 0))
    data, res = R.encode(f.reshape(-1), 4, 4, 1, 1)
    # split 20 20 as above.
    # modes, one mode bit and, where the mode is not 0, the global bit.  (0, 0): "1", global 1 ^ 0 -> "1".  (2, 0): mode
    #   1 ^ 1 = "0", global: y == 0, the left block is global: 0 ^ 1 -> "1".  (0, 2): mode 0 ^ 1 (block (0, 1)) = "1", no
    #   global bit.  (2, 2): modes of (1, 2) 0, (2, 1) 1, (1, 1) 1: majority 1, 1 ^ 1 = "0"; global flags 0, 0, 1: sum 1 < 2,
    #   1 ^ 0 -> "1".  "11 01 1 01" = "1101101" -> da; 20 da.
    # ref-1 x: (2, 0) alone (the others are global or DC); its left neighbour is global and does not predict: sint (3):
    #   4 = 100b -> "00001", sign "0" -> "000010" -> 08; 20 08.  ref-1 y: sint (0) -> 20 80.
    # DC: unit (0, 2), no DC neighbour: "1" in each -> 20 80 three times.
    assert hexs(data) == "20 20 20 da 20 08 20 80 20 80 20 80 20 80"
    assert res["section_units"] == [1, 4, 1, 1, 0, 0, 1, 1, 1]
    back = R.decode(data, 4, 4, 1, 1)
    assert back.tobytes() == R.canonical(f.reshape(-1)).tobytes()


def test_divide3_is_an_arithmetic_shift():
    assert [R.divide3(a) for a in (0, 1, 2, 3, 4, -1, -2, -3, -4, 98302, -98303)] == [0, 0, 0, 1, 1, -1, -1, -1, -2, 32767, -32768]


@pytest.mark.parametrize("case", MC.all_cases(), ids=lambda c: c[0])
def test_round_trip(case):
    name, field, nbx, nby, num_refs, hg, round_trips = case
    data, res = R.encode(field, nbx, nby, num_refs, hg)
    assert res["bytes"] == len(data) <= motion_encode_bound(nbx, nby, num_refs, hg)
    back = R.decode(data, nbx, nby, num_refs, hg)
    same = back.tobytes() == R.canonical(field).tobytes()
    if round_trips:
        assert same, name
        assert res["asserted"] == 0
    else:
        assert not same, name
        assert res["unverified"] > 0 or res["asserted"] > 0


def test_broken_copies_do_not_round_trip_and_are_reported():
    broken = [c for c in MC.all_cases() if c[0].startswith("broken copies")]
    assert len(broken) == 2
    for name, field, nbx, nby, num_refs, hg, _ in broken:
        data, res = R.encode(field, nbx, nby, num_refs, hg)
        assert R.decode(data, nbx, nby, num_refs, hg).tobytes() != R.canonical(field).tobytes()
        assert res["unverified"] == 1 and res["asserted"] == 0
        where = {"broken copies split 0": 12 * 5 + 6, "broken copies split 1": 8 * 3 + 3}[name]
        assert res["first_unverified"] == where


def test_asserts_are_counted():
    by_name = {c[0]: c for c in MC.all_cases()}
    _, field, nbx, nby, num_refs, hg, _ = by_name["split 3"]
    assert R.encode(field, nbx, nby, num_refs, hg)[1]["asserted"] == 1
    _, field, nbx, nby, num_refs, hg, _ = by_name["using_global without the flag"]
    res = R.encode(field, nbx, nby, num_refs, hg)[1]
    m = R.Motion(field, nbx, nby, num_refs, hg)
    assert res["asserted"] == sum(m.using_global[m.at(x, y)] for x, y in R.units(m)) > 0


@pytest.mark.parametrize("num_refs", [1, 2])
def test_bound_holds_on_the_extreme_field(num_refs):
    nbx, nby = 16, 12
    field = MC.extreme(nbx, nby, num_refs)
    data, res = R.encode(field, nbx, nby, num_refs, 0)
    bound = motion_encode_bound(nbx, nby, num_refs, 0)
    assert len(data) <= bound
    # and the field is extreme: most codes take the full 34 bits
    assert 8 * sum(res["section_bytes"][2:]) > 0.8 * 34 * sum(res["section_units"][2:])
