"""CPU: tests/unpack_ref.py, the numpy restatement of the encoder-direction schro_frame_convert, pinned without a device:
(a) it inverts the oracle's pack direction wherever that is an identity, (b) its per-sample steps are the reference's
compiled Orc programs (where oracle/_ref is built), (c) hand-derived byte strings for the v210 tail cases and v216's
high-byte rule; and the refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import unpack_ref as U


def rng(seed):
    return np.random.default_rng(seed)


def planes_of(r, dtype, lo, hi, width, height, hs, vs):
    cw, ch = U.shifted(width, hs), U.shifted(height, vs)
    return [r.integers(lo, hi + 1, (h, w)).astype(dtype) for (w, h) in ((width, height), (cw, ch), (cw, ch))]


# ---- (a) the oracle's pack direction, inverted -------------------------------------------------------------------

@pytest.mark.parametrize("width", [6, 7, 12, 22])
def test_v210_round_trip(width):
    p = planes_of(rng(width), np.int16, -512, 511, width, 3, 1, 0)
    buf = O.pack_v210(p, 1, 0, width, 3)
    got, hs, vs = U.unpack(buf, U.V210, width, 3)
    assert (hs, vs) == (1, 0)
    for g, w in zip(got, p):
        assert g.dtype == np.int16 and np.array_equal(g, w)


@pytest.mark.parametrize("fmt,hs", [(U.YUYV, 1), (U.UYVY, 1), (U.AYUV, 0)])
@pytest.mark.parametrize("width", [2, 6, 22])
def test_u8_round_trip(fmt, hs, width):
    p = planes_of(rng(fmt + width), np.uint8, 0, 255, width, 3, hs, 0)
    buf = O.pack_u8(p, hs, 0, fmt, width, 3)
    got, ghs, gvs = U.unpack(buf, fmt, width, 3)
    assert (ghs, gvs) == (hs, 0)
    for g, w in zip(got, p):
        assert g.dtype == np.uint8 and np.array_equal(g, w)


@pytest.mark.parametrize("width", [1, 7, 22])
def test_ay64_round_trip(width):
    p = planes_of(rng(width), np.int32, -32768, 32767, width, 2, 0, 0)
    buf = O.pack_wide(p, 0, 0, width, 2, U.AY64)
    got, hs, vs = U.unpack(buf, U.AY64, width, 2)
    assert (hs, vs) == (0, 0)
    for g, w in zip(got, p):
        assert g.dtype == np.int32 and np.array_equal(g, w)


@pytest.mark.parametrize("width", [2, 6, 22])
def test_v216_is_the_high_byte_of_what_the_oracle_packed(width):
    p = planes_of(rng(width), np.int16, -32768, 32767, width, 2, 1, 0)
    buf = O.pack_wide(p, 1, 0, width, 2, U.V216)
    words = buf.view("<u2")
    got, hs, vs = U.unpack(buf, U.V216, width, 2)
    assert (hs, vs) == (1, 0)
    assert np.array_equal(got[0], (words[:, 1::2] >> 8).astype(np.int16))
    assert np.array_equal(got[1], (words[:, 0::4] >> 8).astype(np.int16))
    assert np.array_equal(got[2], (words[:, 2::4] >> 8).astype(np.int16))


# ---- (b) the reference's compiled Orc programs ---------------------------------------------------------------------

def orc(name, out_dtype, src):
    src = np.ascontiguousarray(src)
    out = np.zeros(src.size, out_dtype)
    getattr(O.reforc(), name)(out.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), C.c_int(src.size))
    return out


needs_ref = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref is not built")


@needs_ref
def test_unpack_steps_are_the_orc_programs():
    pairs = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    assert np.array_equal(U.yuyv_y(pairs), orc("orc_unpack_yuyv_y", np.uint8, pairs))
    assert np.array_equal(U.uyvy_y(pairs), orc("orc_unpack_uyvy_y", np.uint8, pairs))
    # every value of each byte of the 32-bit word, the other bytes random
    r = rng(1)
    quads = r.integers(0, 2 ** 32, 4 * 256, dtype=np.uint64).astype(np.uint32)
    for b in range(4):
        q = quads[256 * b:256 * (b + 1)]
        q &= ~np.uint32(0xff << (8 * b))
        q |= np.arange(256, dtype=np.uint32) << np.uint32(8 * b)
    for name, f in (("orc_unpack_yuyv_u", U.yuyv_u), ("orc_unpack_yuyv_v", U.yuyv_v), ("orc_unpack_uyvy_u", U.uyvy_u),
                    ("orc_unpack_uyvy_v", U.uyvy_v)):
        assert np.array_equal(f(quads), orc(name, np.uint8, quads)), name


@needs_ref
def test_depth_steps_are_the_orc_programs():
    u8 = np.arange(256, dtype=np.uint32).astype(np.uint8)
    s16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    assert np.array_equal(U.offsetconvert_s16_u8(u8), orc("orc_offsetconvert_s16_u8", np.int16, u8))
    assert np.array_equal(U.offsetconvert_s32_u8(u8), orc("orc_offsetconvert_s32_u8", np.int32, u8))
    assert np.array_equal(U.offsetconvert_u8_s16(s16), orc("orc_offsetconvert_u8_s16", np.uint8, s16))
    assert np.array_equal(U.convert_s32_s16(s16), orc("orc_convert_s32_s16", np.int32, s16))
    # the 32-bit inputs: every value that fits 17 bits, and random ones.  orc_offsetconvert_u8_s32: the shipped C fallback
    # (convsuslw) and the Orc source (convssslw) part above 32767 - 128 (tests/test_oracle_frame.py); the restatement
    # follows the Orc source like the rest of the project, the compiled program is compared below that
    s32 = np.concatenate([np.arange(-65536, 65536, dtype=np.int32), rng(2).integers(-2 ** 31, 2 ** 31, 4096).astype(np.int32)])
    assert np.array_equal(U.convert_s16_s32(s32), orc("orc_convert_s16_s32", np.int16, s32))
    low = s32[(s32.astype(np.int64) + 128 <= 32767) & (s32.astype(np.int64) + 128 >= -2 ** 31)]
    assert np.array_equal(U.offsetconvert_u8_s32(low), orc("orc_offsetconvert_u8_s32", np.uint8, low))
    assert U.offsetconvert_u8_s32(np.array([32640, 70000, 2 ** 31 - 1], np.int32)).tolist() == [255, 255, 0]


# ---- (c) hand-derived bytes ----------------------------------------------------------------------------------------

def v210_word(a, b, c, pad=0):
    return np.array([a | b << 10 | c << 20 | pad << 30], "<u4").view(np.uint8)


def test_v210_tail_groups_by_hand():
    # one group: words (U0 Y0 V0) (Y1 U1 Y2) (V1 Y3 U2) (Y4 V2 Y5), schrovirtframe.c:776-857; the pad bits are set
    row = np.concatenate([v210_word(1, 2, 3, 3), v210_word(4, 5, 6, 3), v210_word(7, 8, 9, 3), v210_word(10, 11, 12, 3)])[None, :]
    want_y, want_u, want_v = [2, 4, 6, 8, 10, 12], [1, 5, 9], [3, 7, 11]
    for width in range(1, 7):
        (y, u, v), hs, vs = U.unpack(row, U.V210, width, 1)
        cw = (width + 1) // 2
        assert (y + 512).tolist() == [want_y[:width]]
        assert (u + 512).tolist() == [want_u[:cw]] and (v + 512).tolist() == [want_v[:cw]]
    # width 7: the seventh pixel and the fourth chroma pair come from the second group's first words
    row2 = np.concatenate([row[0], v210_word(100, 200, 300), v210_word(0, 0, 0), v210_word(0, 0, 0), v210_word(0, 0, 0)])[None, :]
    (y, u, v), _, _ = U.unpack(row2, U.V210, 7, 1)
    assert (y + 512).tolist() == [want_y + [200]] and (u + 512).tolist() == [want_u + [100]] and (v + 512).tolist() == [want_v + [300]]
    # 10-bit extremes: 0 -> -512, 1023 -> 511
    ext = np.concatenate([v210_word(0, 1023, 0), v210_word(1023, 0, 1023), v210_word(0, 0, 0), v210_word(0, 0, 0)])[None, :]
    (y, u, v), _, _ = U.unpack(ext, U.V210, 3, 1)
    assert y.tolist() == [[511, 511, 511]] and u.tolist() == [[-512, -512]] and v.tolist() == [[-512, -512]]


def test_v216_takes_the_high_byte_and_no_offset():
    # U Y0 V Y1 as little-endian 16-bit words 0x11aa 0x22bb 0x33cc 0xff01
    row = np.array([[0xaa, 0x11, 0xbb, 0x22, 0xcc, 0x33, 0x01, 0xff]], np.uint8)
    (y, u, v), hs, vs = U.unpack(row, U.V216, 2, 1)
    assert y.dtype == np.int16 and y.tolist() == [[0x22, 0xff]] and u.tolist() == [[0x11]] and v.tolist() == [[0x33]]


def test_ay64_and_u8_formats_by_hand():
    row = np.array([[9, 9, 0, 0, 0xff, 0xff, 0x00, 0x80]], np.uint8)      # A, Y = 0, U = 0xffff, V = 0x8000
    (y, u, v), _, _ = U.unpack(row, U.AY64, 1, 1)
    assert y.dtype == np.int32 and (y[0, 0], u[0, 0], v[0, 0]) == (-32768, 32767, 0)
    row = np.array([[1, 2, 3, 4]], np.uint8)
    assert [p.tolist() for p in U.unpack(row, U.YUYV, 2, 1)[0]] == [[[1, 3]], [[2]], [[4]]]
    assert [p.tolist() for p in U.unpack(row, U.UYVY, 2, 1)[0]] == [[[2, 4]], [[1]], [[3]]]
    assert [p.tolist() for p in U.unpack(row, U.AYUV, 1, 1)[0]] == [[[2]], [[3]], [[4]]]


# ---- the chain ---------------------------------------------------------------------------------------------------

def test_depth_comes_before_chroma_and_size_clamps():
    r = rng(5)
    buf = r.integers(0, 256, (5, U.row_bytes(U.V210, 14)), dtype=np.uint8)
    (y, u, v), _, _ = U.unpack(buf, U.V210, 14, 5)
    out = U.convert((buf, U.V210, 14, 5), np.uint8, 1, 1, 16, 6)          # v210 -> u8 4:2:0, extended
    assert [p.shape for p in out] == [(6, 16), (3, 8), (3, 8)]
    y8, u8 = U.offsetconvert_u8_s16(y), U.offsetconvert_u8_s16(u)
    assert np.array_equal(out[0][:5, :14], y8) and np.all(out[0][5] == out[0][4]) and np.all(out[0][:, 15] == out[0][:, 13])
    assert np.array_equal(out[1][:, :7], u8[0::2]) and np.all(out[1][:, 7] == out[1][:, 6])
    # the same change asked of an s16 frame asserts in the reference
    with pytest.raises(U.Refused):
        U.convert((buf, U.V210, 14, 5), np.int16, 1, 1, 16, 6)
    # repetition: 4:2:2 -> 4:4:4
    b8 = r.integers(0, 256, (2, U.row_bytes(U.UYVY, 6)), dtype=np.uint8)
    o = U.convert((b8, U.UYVY, 6, 2), np.uint8, 0, 0, 6, 2)
    assert o[1].tolist() == np.repeat(b8[:, 0::4], 2, axis=1).tolist()


def test_refusals():
    buf = np.zeros((4, 64), np.uint8)
    for bad in (lambda: U.convert((buf, U.ARGB, 4, 4), np.int16, 0, 0, 4, 4),
                lambda: U.convert((buf, U.AY64, 4, 4), np.uint8, 0, 0, 4, 4),
                lambda: U.convert((buf, U.YUYV, 5, 4), np.uint8, 1, 0, 5, 4),
                lambda: U.convert((buf, U.UYVY, 5, 4), np.uint8, 1, 0, 5, 4),
                lambda: U.convert((buf, U.V216, 3, 4), np.int16, 1, 0, 3, 4),
                lambda: U.convert((buf, U.AYUV, 4, 4), np.int16, 1, 0, 4, 4),
                lambda: U.convert((buf, U.AYUV, 4, 4), np.uint8, 0, 0, 6, 2),
                lambda: U.convert((buf, U.AYUV, 4, 4), np.uint8, 0, 0, 2, 6)):
        with pytest.raises(U.Refused):
            bad()


def test_row_bytes_is_the_librarys():
    import schroedinger_amd as sa
    for fmt in U.PACKED:
        for w in (1, 2, 6, 7, 22, 331):
            assert sa.unpack_row_bytes(fmt, w) == U.row_bytes(fmt, w)
