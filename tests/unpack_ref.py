"""The encoder-direction schro_frame_convert (schroframe.c:869-979), restated in numpy: what the chain of virtual frames
renders when a packed picture (or a planar frame) is converted into a planar frame.

  unpack   schro_virt_frame_new_unpack (schrovirtframe.c:616-940)
  depth    schroframe.c:905-924 -- before the chroma step
  chroma   schro_virt_frame_new_subsample (schrovirtframe.c:1438-1576): u8 frames only
  size     schro_virt_frame_new_crop / _edgeextend (schrovirtframe.c:1823-1960)

`convert` is the whole chain and raises Refused where the reference asserts or reads lines of the wrong type; tests/
test_unpack_ref.py pins it (the oracle's pack direction inverted, the reference's compiled Orc programs, hand-derived
bytes), the GPU tests compare schro_hip_unpack_batch and schro_hip_unpack_iwt_batch with it bit for bit."""
import numpy as np

YUYV, UYVY, AYUV, ARGB, V216, V210, AY64 = 0x100, 0x101, 0x102, 0x103, 0x105, 0x106, 0x107
PACKED = (YUYV, UYVY, AYUV, V210, V216, AY64)
# the unpacked frame of each packed format: dtype, h_shift, v_shift (schrovirtframe.c:902-933)
NATURAL = {YUYV: (np.uint8, 1, 0), UYVY: (np.uint8, 1, 0), AYUV: (np.uint8, 0, 0), V210: (np.int16, 1, 0),
           V216: (np.int16, 1, 0), AY64: (np.int32, 0, 0)}


class Refused(ValueError):
    pass


def shifted(v, shift):
    return (v + (1 << shift) - 1) >> shift


def row_bytes(fmt, width):
    return {YUYV: 4 * (width // 2), UYVY: 4 * (width // 2), AYUV: 4 * width, V216: 8 * (width // 2),
            V210: 16 * (-(-width // 6)), AY64: 8 * width}[fmt]


# ---- the per-sample steps (schroorc.orc) -----------------------------------------------------------------------------

def yuyv_y(pairs):
    """orc_unpack_yuyv_y: select0wb of each 16-bit word."""
    return (np.asarray(pairs, np.uint16) & 0xff).astype(np.uint8)


def uyvy_y(pairs):
    """orc_unpack_uyvy_y: select1wb."""
    return (np.asarray(pairs, np.uint16) >> 8).astype(np.uint8)


def yuyv_u(quads):
    """orc_unpack_yuyv_u: select0lw, select1wb of each 32-bit word."""
    return ((np.asarray(quads, np.uint32) >> 8) & 0xff).astype(np.uint8)


def yuyv_v(quads):
    return ((np.asarray(quads, np.uint32) >> 24) & 0xff).astype(np.uint8)


def uyvy_u(quads):
    return (np.asarray(quads, np.uint32) & 0xff).astype(np.uint8)


def uyvy_v(quads):
    return ((np.asarray(quads, np.uint32) >> 16) & 0xff).astype(np.uint8)


def offsetconvert_s16_u8(x):
    return (np.asarray(x, np.uint8).astype(np.int32) - 128).astype(np.int16)


def offsetconvert_s32_u8(x):
    return np.asarray(x, np.uint8).astype(np.int32) - 128


def offsetconvert_u8_s16(x):
    """addw 128 (wraps at 16 bits), convsuswb."""
    t = (np.asarray(x, np.int16).astype(np.int32) + 128).astype(np.int16)
    return np.clip(t, 0, 255).astype(np.uint8)


def offsetconvert_u8_s32(x):
    """addl 128 (wraps at 32 bits), convssslw, convsuswb (schroorc.orc:513-521)."""
    t = (np.asarray(x, np.int32).astype(np.int64) + 128 + 2 ** 31) % 2 ** 32 - 2 ** 31
    return np.clip(np.clip(t, -32768, 32767), 0, 255).astype(np.uint8)


def convert_s16_s32(x):
    """convlw: the low 16 bits."""
    return np.asarray(x, np.int32).astype(np.int16)


def convert_s32_s16(x):
    return np.asarray(x, np.int16).astype(np.int32)


# ---- the chain ---------------------------------------------------------------------------------------------------

V210_LUMA = ((0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20))        # (word of the group, shift) per pixel of a group
V210_U = ((0, 0), (1, 10), (2, 20))
V210_V = ((0, 20), (2, 0), (3, 10))


def _v210_component(words, table, n):
    per = len(table)
    x = np.arange(n)
    word = 4 * (x // per) + np.array([t[0] for t in table])[x % per]
    shift = np.array([t[1] for t in table], np.uint32)[x % per]
    return (((words[:, word] >> shift) & 0x3ff).astype(np.int32) - 512).astype(np.int16)


def unpack(buf, fmt, width, height):
    """(planes [Y, U, V], h_shift, v_shift) of the unpacked frame.  buf: height rows of at least row_bytes (fmt, width)
    bytes (a uint8 array)."""
    if fmt == ARGB:
        raise Refused("ARGB: unpack_argb writes 16-bit samples into a frame labelled U8_444 (schrovirtframe.c:693-732, 927-929)")
    if fmt in (YUYV, UYVY, V216) and width & 1:
        raise Refused("odd width: width / 2 chroma samples of a (width + 1) / 2 wide component (schrovirtframe.c:629, 881)")
    buf = np.ascontiguousarray(np.asarray(buf, np.uint8)[:height, :row_bytes(fmt, width)])
    dt, hs, vs = NATURAL[fmt]
    cw = shifted(width, hs)
    if fmt == YUYV:
        planes = [buf[:, 0::2], buf[:, 1::4], buf[:, 3::4]]
    elif fmt == UYVY:
        planes = [buf[:, 1::2], buf[:, 0::4], buf[:, 2::4]]
    elif fmt == AYUV:
        planes = [buf[:, 1::4], buf[:, 2::4], buf[:, 3::4]]
    elif fmt == V216:             # the HIGH byte of each 16-bit word, no offset (schrovirtframe.c:876-888)
        planes = [buf[:, 3::4].astype(np.int16), buf[:, 1::8].astype(np.int16), buf[:, 5::8].astype(np.int16)]
    elif fmt == AY64:
        w16 = buf.view("<u2").astype(np.int32) - 32768
        planes = [w16[:, 1::4], w16[:, 2::4], w16[:, 3::4]]
    else:
        words = buf.view("<u4")
        planes = [_v210_component(words, V210_LUMA, width), _v210_component(words, V210_U, cw),
                  _v210_component(words, V210_V, cw)]
    sizes = [width, cw, cw]
    return [np.ascontiguousarray(p[:, :n]).astype(dt) for p, n in zip(planes, sizes)], hs, vs


def depth(planes, dtype):
    src, dst = np.dtype(planes[0].dtype), np.dtype(dtype)
    if src == dst:
        return planes
    step = {(np.uint8, np.int16): offsetconvert_s16_u8, (np.uint8, np.int32): offsetconvert_s32_u8,
            (np.int16, np.int32): convert_s32_s16, (np.int32, np.int16): convert_s16_s32,
            (np.int16, np.uint8): offsetconvert_u8_s16, (np.int32, np.uint8): offsetconvert_u8_s32}[(src.type, dst.type)]
    return [step(p) for p in planes]


def chroma(planes, src_shifts, dst_shifts, width, height):
    """Decimation / repetition of the chroma planes of a width x height u8 frame."""
    if tuple(src_shifts) == tuple(dst_shifts):
        return planes
    if planes[0].dtype != np.uint8:
        raise Refused("chroma change on an s16 / s32 frame (schrovirtframe.c:1549-1569)")
    (hs_s, vs_s), (hs_d, vs_d) = src_shifts, dst_shifts
    x, y = np.arange(shifted(width, hs_d)), np.arange(shifted(height, vs_d))
    x = x * 2 if hs_d > hs_s else x >> 1 if hs_d < hs_s else x
    y = y * 2 if vs_d > vs_s else y >> 1 if vs_d < vs_s else y
    return [planes[0]] + [p[np.ix_(y, x)] for p in planes[1:]]


def size(planes, shifts, src_size, dst_size):
    (sw, sh), (w, h) = src_size, dst_size
    if (w < sw or h < sh) and (w > sw or h > sh):
        raise Refused("crop and extension mixed (schrovirtframe.c:1861-1862, 1939-1940)")
    out = []
    for k, p in enumerate(planes):
        hs, vs = shifts if k else (0, 0)
        x = np.minimum(np.arange(shifted(w, hs)), shifted(sw, hs) - 1)
        y = np.minimum(np.arange(shifted(h, vs)), shifted(sh, vs) - 1)
        out.append(np.ascontiguousarray(p[np.ix_(y, x)]))
    return out


def convert(source, dtype, h_shift, v_shift, width, height):
    """schro_frame_convert (planar dest, source).  source: (buf, fmt, src_width, src_height), or (planes, h_shift, v_shift,
    src_width, src_height) for a planar frame.  Returns the planes [Y, U, V] of the width x height destination."""
    if len(source) == 4:
        buf, fmt, sw, sh = source
        if fmt == AY64 and np.dtype(dtype) == np.uint8:
            raise Refused("AY64 -> u8: schroframe.c:908 tests the packed format code's depth and reads s32 lines as s16")
        planes, hs, vs = unpack(buf, fmt, sw, sh)
    else:
        planes, hs, vs, sw, sh = source
        planes = [np.asarray(p)[:shifted(sh, vs if k else 0), :shifted(sw, hs if k else 0)] for k, p in enumerate(planes)]
    if min(width, height, sw, sh) <= 0:
        raise Refused("sizes must be positive")
    planes = depth(planes, dtype)
    planes = chroma(planes, (hs, vs), (h_shift, v_shift), sw, sh)
    return size(planes, (h_shift, v_shift), (sw, sh), (width, height))


def chain(buf, fmt, src_size, picture_size, iwt_size, shifts, dtype):
    """The frame schro_hip_unpack_iwt_batch transforms: the packed picture into a picture_size frame of the format's own
    depth, that into an iwt_size frame of `dtype` (the offset removed, the edges extended)."""
    (sw, sh), (w, h), (iw, ih), (hs, vs) = src_size, picture_size, iwt_size, shifts
    a = convert((buf, fmt, sw, sh), NATURAL[fmt][0], hs, vs, w, h)
    return convert((a, hs, vs, w, h), dtype, hs, vs, iw, ih)
