"""GPU: schro_hip_unpack_batch (unpack.hip), the encoder-direction schro_frame_convert, against its numpy restatement
(tests/unpack_ref.py), bit for bit.

Sources and destinations are carved out of a guarded block (tests/guard_lib.py): every byte outside the destination
components' rectangles must stay as it was, and since paddings and guards hold random bytes, a result that depends on
bytes outside the source rows shows up as a mismatch.  The packed sources are random bytes -- every v210 word has all 30
bits and its two pad bits drawn, v216 words have unlike low bytes, AY64 rows hold 0 and 0xffff -- so the depth steps see
their whole input range.

Sizes: 64 x 32; 331 x 150 out of 352 x 160 (a crop whose last v210 group, last YUYV pair and last 16-byte store piece
are partial); 150 x 62 extended to 160 x 64; 6 x 1, 7 x 2 (out of 8 x 2 where the format has no odd widths) and 2 x 2."""
import numpy as np
import pytest

import guard_lib as G
import schroedinger_amd as sa
import unpack_ref as U

pytestmark = pytest.mark.gpu

EINVAL = -1             # SCHRO_HIP_EINVAL (include/schro_hip.h)
NAMES = {U.YUYV: "yuyv", U.UYVY: "uyvy", U.AYUV: "ayuv", U.V210: "v210", U.V216: "v216", U.AY64: "ay64"}
EVEN_ONLY = (U.YUYV, U.UYVY, U.V216)
# (source size, destination size)
SIZES = [((64, 32), (64, 32)), ((352, 160), (331, 150)), ((150, 62), (160, 64)), ((6, 1), (6, 1)), ((7, 2), (7, 2)), ((2, 2), (2, 2))]


def packed_bytes(fmt, sw, sh, seed):
    r = np.random.default_rng(seed)
    buf = r.integers(0, 256, (sh, U.row_bytes(fmt, sw)), dtype=np.uint8)
    if fmt == U.AY64:           # both ends of the 16-bit range
        w = buf.view("<u2")
        w[0, 1::4] = 0
        w[-1, 2::4] = 0xffff
        w[0, 3] = 0xffff
    if fmt == U.V210 and seed % 2:      # the pad bits set in every word
        buf[:, 3::4] |= 0xc0
    return buf


def planar_planes(dtype, hs, vs, sw, sh, seed):
    r = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    return [r.integers(info.min, info.max + 1, (U.shifted(sh, vs if k else 0), U.shifted(sw, hs if k else 0))).astype(dtype)
            for k in range(3)]


def picture(src, dst_dtype, hs, vs, size, **kw):
    """src: (fmt, sw, sh) or (dtype, hs, vs, sw, sh)."""
    return dict(src=src, dtype=np.dtype(dst_dtype), hs=hs, vs=vs, w=size[0], h=size[1], **kw)


def run(ctx, pictures, seed=0, expect=None):
    """One call.  Options per picture: src_pad (extra bytes of source stride), src_skew (bytes the source starts after a
    256-byte boundary), dst_pad, dst_skew likewise for the destination planes.  expect: an error code the call must
    return, the block then untouched."""
    lay, specs = G.Layout(), []
    for n, p in enumerate(pictures):
        if len(p["src"]) == 3:
            fmt, sw, sh = p["src"]
            row = U.row_bytes(fmt, sw)
            s = [lay.plane(sh, row, np.uint8, stride=max(row, 1) + p.get("src_pad", 0), skew=p.get("src_skew", 0), footprint=None,
                           name="src%d" % n)]
        else:
            dt, shs, svs, sw, sh = p["src"]
            dt = np.dtype(dt)
            s = []
            for k in range(3):
                cw, ch = U.shifted(sw, shs if k else 0), U.shifted(sh, svs if k else 0)
                s.append(lay.plane(ch, cw, dt, stride=cw * dt.itemsize + p.get("src_pad", 0) * dt.itemsize,
                                   skew=p.get("src_skew", 0) * dt.itemsize, footprint=None, name="src%d.%d" % (n, k)))
        d = []
        for k in range(3):
            cw, ch = U.shifted(p["w"], p["hs"] if k else 0), U.shifted(p["h"], p["vs"] if k else 0)
            bpp = p["dtype"].itemsize
            d.append(lay.plane(ch, cw, p["dtype"], stride=p.get("dst_stride", cw * bpp + p.get("dst_pad", 0) * bpp),
                               skew=p.get("dst_skew", 0) * bpp, name="dst%d.%d" % (n, k)))
        specs.append((s, d))
    blk = G.GuardedBlock(ctx, lay, seed=seed)
    jobs, expected = [], {}
    try:
        for n, (p, (s, d)) in enumerate(zip(pictures, specs)):
            if len(p["src"]) == 3:
                fmt, sw, sh = p["src"]
                buf = packed_bytes(fmt, sw, sh, seed * 100 + n)
                blk[s[0]].upload(buf)
                source, ref_source = (blk[s[0]], fmt, sw, sh), (buf, fmt, sw, sh)
            else:
                dt, shs, svs, sw, sh = p["src"]
                planes = planar_planes(dt, shs, svs, sw, sh, seed * 100 + n)
                for sp, a in zip(s, planes):
                    blk[sp].upload(a)
                source, ref_source = ([blk[sp] for sp in s], shs, svs, sw, sh), (planes, shs, svs, sw, sh)
            if expect is None:
                want = U.convert(ref_source, p["dtype"], p["hs"], p["vs"], p["w"], p["h"])
                for sp, a in zip(d, want):
                    expected[sp] = a
            jobs.append((source, [blk[sp] for sp in d], p["hs"], p["vs"], p["w"], p["h"]))
        ctx.synchronize()
        if expect is None:
            ctx.unpack_batch(jobs)
            ctx.synchronize()
        else:
            with pytest.raises(sa.SchroHipError) as e:
                ctx.unpack_batch(jobs)
            assert e.value.code == expect, e.value
            ctx.synchronize()
        blk.check(expected)
        return blk, specs
    finally:
        blk.free()


def natural(fmt):
    return U.NATURAL[fmt][1:]


def all_formats_pictures(dtype):
    out = []
    for fmt in U.PACKED:
        if fmt == U.AY64 and np.dtype(dtype) == np.uint8:
            continue
        hs, vs = natural(fmt)
        for (src, dst) in SIZES:
            if fmt in EVEN_ONLY and src[0] & 1:
                src = (src[0] + 1, src[1])      # 7 x 2 out of 8 x 2
            out.append(picture((fmt,) + src, dtype, hs, vs, dst))
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32], ids=["u8", "s16", "s32"])
def test_every_format_and_size_in_one_call(ctx, dtype):
    pics = all_formats_pictures(dtype)
    assert len(pics) <= 85
    run(ctx, pics, seed=np.dtype(dtype).itemsize)


def test_depths_mix_in_one_call(ctx):
    pics = []
    for n, fmt in enumerate(U.PACKED):
        hs, vs = natural(fmt)
        for m, dt in enumerate((np.uint8, np.int16, np.int32)):
            if fmt == U.AY64 and dt == np.uint8:
                continue
            src, dst = SIZES[(n + m) % 3]
            pics.append(picture((fmt,) + src, dt, hs, vs, dst))
    run(ctx, pics, seed=7)


def test_u8_chroma_decimation_and_repetition(ctx):
    pics = [picture((U.AYUV, 64, 32), np.uint8, 1, 0, (64, 32)),          # 4:4:4 -> 4:2:2
            picture((U.AYUV, 64, 32), np.uint8, 1, 1, (64, 32)),          # 4:4:4 -> 4:2:0
            picture((U.UYVY, 64, 32), np.uint8, 1, 1, (64, 32)),          # 4:2:2 -> 4:2:0
            picture((U.UYVY, 352, 160), np.uint8, 1, 1, (331, 150)),
            picture((U.AYUV, 331, 151), np.uint8, 1, 1, (331, 151)),      # odd sizes: components rounded up
            picture((U.AYUV, 150, 62), np.uint8, 1, 0, (160, 64)),
            picture((U.YUYV, 150, 62), np.uint8, 0, 0, (160, 64)),        # repetition 4:2:2 -> 4:4:4
            picture((U.V210, 64, 32), np.uint8, 1, 1, (64, 32)),          # depth first, then chroma
            picture((U.V210, 331, 150), np.uint8, 1, 1, (352, 160)),
            picture((U.V216, 64, 32), np.uint8, 0, 0, (64, 32)),
            picture((np.uint8, 1, 1, 150, 62), np.uint8, 0, 0, (160, 64)),        # planar 4:2:0 -> 4:4:4
            picture((np.int16, 0, 0, 64, 32), np.uint8, 1, 1, (64, 32)),
            picture((np.int32, 1, 0, 7, 3), np.uint8, 1, 1, (7, 3))]
    run(ctx, pics, seed=11)


def test_planar_sources_every_depth_pair(ctx):
    """The identity unpack: what makes the intra picture's convert into the transform frame (schroencoder.c:2454)
    expressible.  Full-range samples: s32 -> s16 truncates, s16 -> u8 wraps at 16 bits before it clamps, s32 -> u8 at 32."""
    pics = []
    for n, sd in enumerate((np.uint8, np.int16, np.int32)):
        for m, dd in enumerate((np.uint8, np.int16, np.int32)):
            src, dst = SIZES[(n + m) % 3]
            hs, vs = ((0, 0), (1, 0), (1, 1))[(n + 2 * m) % 3]
            pics.append(picture((sd, hs, vs) + src, dd, hs, vs, dst))
            pics.append(picture((sd, hs, vs, 7, 2), dd, hs, vs, (7, 2)))
    run(ctx, pics, seed=13)


def test_pointers_and_strides_that_force_the_scalar_tail(ctx):
    pics = []
    for n, fmt in enumerate(U.PACKED):
        hs, vs = natural(fmt)
        for m, dt in enumerate((np.uint8, np.int16, np.int32)):
            if fmt == U.AY64 and dt == np.uint8:
                continue
            # destination one sample off a 256-byte boundary, stride three samples over the row; the source an odd number
            # of bytes off and of odd stride (AY64: 2-byte aligned)
            odd = 2 if fmt == U.AY64 else 1
            pics.append(picture((fmt, 352, 160), dt, hs, vs, (331, 150), dst_skew=1, dst_pad=3, src_skew=odd, src_pad=odd))
            pics.append(picture((fmt, 22, 3), dt, hs, vs, (22, 3), dst_skew=1 + m, src_skew=odd * 3, src_pad=4 + odd))
    run(ctx, pics, seed=17)


def test_aligned_destination_with_unaligned_source(ctx):
    pics = [picture((fmt, 64, 32), U.NATURAL[fmt][0], *natural(fmt), (64, 32), src_skew=2, src_pad=6) for fmt in U.PACKED]
    run(ctx, pics, seed=19)


REFUSALS = {
    "argb": picture((U.AYUV, 8, 4), np.int16, 0, 0, (8, 4), fmt_override=U.ARGB),
    "ay64-u8": picture((U.AY64, 8, 4), np.uint8, 0, 0, (8, 4)),
    "yuyv-odd": picture((U.YUYV, 8, 4), np.uint8, 1, 0, (7, 4), sw_override=7),
    "uyvy-odd": picture((U.UYVY, 8, 4), np.uint8, 1, 0, (7, 4), sw_override=7),
    "v216-odd": picture((U.V216, 8, 4), np.int16, 1, 0, (7, 4), sw_override=7),
    "chroma-s16": picture((U.AYUV, 8, 4), np.int16, 1, 0, (8, 4)),
    "chroma-v210": picture((U.V210, 12, 4), np.int16, 1, 1, (12, 4)),
    "chroma-planar-s32": picture((np.int32, 0, 0, 8, 4), np.int32, 1, 0, (8, 4)),
    "wider-shorter": picture((U.AYUV, 8, 4), np.uint8, 0, 0, (10, 3)),
    "narrower-taller": picture((U.UYVY, 8, 4), np.uint8, 1, 0, (6, 5)),
    "src-stride": picture((U.V210, 12, 4), np.int16, 1, 0, (12, 4), src_stride_override=31),
    "dst-stride": picture((U.UYVY, 8, 4), np.int16, 1, 0, (8, 4), dst_stride=14),
    "dst-misaligned": picture((U.UYVY, 8, 4), np.int16, 1, 0, (8, 4), dst_ptr_offset=1),
    "planar-src-misaligned": picture((np.int16, 1, 0, 8, 4), np.int16, 1, 0, (8, 4), src_ptr_offset=1),
    "ay64-misaligned": picture((U.AY64, 8, 4), np.int32, 0, 0, (8, 4), src_ptr_offset=1),
    "overlap": picture((U.AYUV, 8, 4), np.uint8, 0, 0, (8, 4), overlap=True),
    "zero-width": picture((U.AYUV, 8, 4), np.uint8, 0, 0, (8, 4), w_override=0),
    "negative-src-height": picture((U.AYUV, 8, 4), np.uint8, 0, 0, (8, 4), sh_override=-1),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_launch_nothing(ctx, case):
    """Every refusal returns EINVAL and names the reference's line where there is one; the guarded block (a good picture in
    front of the bad one included) is untouched."""
    bad = REFUSALS[case]
    good = picture((U.UYVY, 8, 4), np.uint8, 1, 0, (8, 4))
    lay = G.Layout()
    planes = []
    for p in (good, bad):
        if len(p["src"]) == 3:
            fmt, sw, sh = p["src"]
            s = [lay.plane(sh, U.row_bytes(fmt, sw), np.uint8, footprint=None)]
        else:
            dt, shs, svs, sw, sh = p["src"]
            s = [lay.plane(U.shifted(sh, svs if k else 0), U.shifted(sw, shs if k else 0), dt, footprint=None) for k in range(3)]
        d = [lay.plane(U.shifted(p["h"], p["vs"] if k else 0), U.shifted(p["w"], p["hs"] if k else 0), p["dtype"], footprint=None)
             for k in range(3)]
        planes.append((s, d))
    blk = G.GuardedBlock(ctx, lay, seed=23)
    try:
        arr = (sa._lib.UnpackPicture * 2)()
        for a, p, (s, d) in zip(arr, (good, bad), planes):
            if len(p["src"]) == 3:
                a.format, a.src_width, a.src_height = p["src"]
                a.src[0], a.src_stride[0] = blk[s[0]].ptr, blk[s[0]].stride
            else:
                dt, a.src_h_shift, a.src_v_shift, a.src_width, a.src_height = p["src"]
                a.src_bpp = np.dtype(dt).itemsize
                for k in range(3):
                    a.src[k], a.src_stride[k] = blk[s[k]].ptr, blk[s[k]].stride
            for k in range(3):
                a.dst[k], a.dst_stride[k] = blk[d[k]].ptr, p.get("dst_stride", blk[d[k]].stride)
            a.dst_bpp, a.h_shift, a.v_shift, a.width, a.height = p["dtype"].itemsize, p["hs"], p["vs"], p["w"], p["h"]
            a.format = p.get("fmt_override", a.format)
            a.src_width = p.get("sw_override", a.src_width)
            a.src_height = p.get("sh_override", a.src_height)
            a.width = p.get("w_override", a.width)
            a.src_stride[0] = p.get("src_stride_override", a.src_stride[0])
            a.dst[1] += p.get("dst_ptr_offset", 0)
            a.src[0] += p.get("src_ptr_offset", 0)
            if p.get("overlap"):
                a.dst[2] = a.src[0] + 3
        assert ctx.lib.schro_hip_unpack_batch(ctx.h, arr, 1) == 0         # the good picture alone is accepted
        ctx.synchronize()
        good_want = U.convert((blk[planes[0][0][0]].initial(), U.UYVY, 8, 4), np.uint8, 1, 0, 8, 4)
        for sp, a in zip(planes[0][1], good_want):
            assert np.array_equal(blk[sp].download(), a)
            blk[sp].upload(blk[sp].initial())                             # back to the canary
        ctx.synchronize()
        assert ctx.lib.schro_hip_unpack_batch(ctx.h, arr, 2) == EINVAL, case
        msg = ctx.lib.schro_hip_last_error().decode()
        assert "picture 1" in msg or case in ("overlap",), msg
        if case in ("argb", "ay64-u8", "yuyv-odd", "uyvy-odd", "v216-odd", "chroma-s16", "chroma-v210", "chroma-planar-s32",
                    "wider-shorter", "narrower-taller"):
            assert "schrovirtframe.c:" in msg or "schroframe.c:" in msg, msg
        ctx.synchronize()
        blk.check({})
    finally:
        blk.free()
