"""GPU: schro_hip_unpack_iwt_batch -- an intra picture from packed bytes to wavelet coefficients -- against
O.forward_iwt of the restated convert chain (tests/unpack_ref.py chain), bit for bit.

FUSED pictures never exist as planes: the level-0 launch of iwt_fwd.hip fetches the packed rows, clamps the coordinate to
the picture (the edge extension) and removes the offset in registers.  Every case reports its routes; an all-FUSED call
launches nothing of the "convert" profile class; sources and coefficient planes are carved out of a guarded block
(tests/guard_lib.py).  The transform sizes 352 x 160 (picture 331 x 150) and 160 x 64 (picture 150 x 62) are several tiles
across and down for every filter's tile with partial last tiles, the picture's edge inside a tile's halo and inside its
useful part; 44 x 12 (picture 41 x 11) at depth 1 has sub-band rows that are no whole vectors.  EXTENSION_SIZES holds
pictures far smaller than their transform: whole tiles lie in the edge extension, one picture is a deep crop."""
import os

import numpy as np
import pytest

import guard_lib as G
import oracle_lib as O
import schroedinger_amd as sa
import unpack_ref as U

pytestmark = pytest.mark.gpu

EVEN_ONLY = (U.YUYV, U.UYVY, U.V216)
# (transform size, picture size, source size less the picture size)
SIZES = [((64, 32), (64, 32), (0, 0)), ((352, 160), (331, 150), (5, 2)), ((160, 64), (150, 62), (-2, -2))]
DEPTH1_SIZE = ((44, 12), (41, 11), (0, 0))


def source_size(fmt, pic, delta):
    sw, sh = pic[0] + delta[0], pic[1] + delta[1]
    if fmt in EVEN_ONLY and sw & 1:
        sw += 1 if delta[0] >= 0 else -1
    return sw, sh


def packed_bytes(fmt, sw, sh, seed):
    r = np.random.default_rng(seed)
    buf = r.integers(0, 256, (sh, U.row_bytes(fmt, sw)), dtype=np.uint8)
    if fmt == U.AY64:
        w = buf.view("<u2")
        w[0, 1::4] = 0
        w[-1, 2::4] = 0xffff
    return buf


def pic(fmt, size, shifts=None, **kw):
    iwt, p, delta = size
    return dict(fmt=fmt, iwt=iwt, pic=p, src=source_size(fmt, p, delta), shifts=shifts or U.NATURAL[fmt][1:], **kw)


# Which format x sample size x filter takes FUSED in the product library: where scripts/unpack_iwt_ab.py --sweep did not
# measure the packed level 0 slower than the chain by more than the larger of the two forms' spreads (profiles/unpack_iwt.txt;
# unpack_fused_combination, plane_unpack.cpp).  Everything else keeps the two passes.
# tests/test_gpu_unpack_experiments.py runs this file again on the experiments library with SCHRO_HIP_UNPACK_FUSED=1 (every
# combination on FUSED) and with SCHRO_HIP_UNPACK_TWO_PASS=1 (every picture on the two passes).
FUSED_FILTERS = {(fmt, 2): (3, 4) for fmt in (U.YUYV, U.UYVY, U.AYUV, U.V210, U.V216)}
FUSED_FILTERS.update({(fmt, 4): (0, 1, 2, 3, 4, 6) for fmt in (U.YUYV, U.UYVY, U.AYUV, U.V210, U.V216)})
FUSED_FILTERS.update({(U.AY64, 2): (0, 1, 2, 3, 4, 6), (U.AY64, 4): (0, 1, 2, 3, 4, 5, 6)})
_EXP = "exp" in os.path.basename(os.environ.get("SCHRO_HIP_LIB", ""))
FORCED_FUSED = _EXP and os.environ.get("SCHRO_HIP_UNPACK_FUSED") == "1"
FORCED_TWO_PASS = _EXP and os.environ.get("SCHRO_HIP_UNPACK_TWO_PASS") == "1"


def expected_route(p, filt, dtype):
    """The route of a picture: FUSED needs an aligned source, the packed format's own chroma format and a measured
    combination."""
    aligned = p.get("src_pad", 0) % 16 == 0 and p.get("src_skew", 0) % 16 == 0
    if FORCED_TWO_PASS or not aligned or tuple(p["shifts"]) != tuple(U.NATURAL[p["fmt"]][1:]):
        return "two_pass"
    return "fused" if FORCED_FUSED or filt in FUSED_FILTERS[(p["fmt"], np.dtype(dtype).itemsize)] else "two_pass"


def layout_of(pictures, dtype, footprint="rect"):
    lay, specs = G.Layout(), []
    for n, p in enumerate(pictures):
        sw, sh = p["src"]
        row = U.row_bytes(p["fmt"], sw)
        s = lay.plane(sh, row, np.uint8, stride=-(-row // 16) * 16 + p.get("src_pad", 0), skew=p.get("src_skew", 0), footprint=None,
                      name="src%d" % n)
        hs, vs = p["shifts"]
        d = [lay.plane(U.shifted(p["iwt"][1], vs if k else 0), U.shifted(p["iwt"][0], hs if k else 0), dtype,
                       footprint=footprint, name="coeff%d.%d" % (n, k)) for k in range(3)]
        specs.append((s, d))
    return lay, specs


def job_of(blk, p, s, d):
    return (blk[s], p["fmt"], p["src"][0], p["src"][1], p["pic"][0], p["pic"][1], [blk[x] for x in d], p["shifts"][0],
            p["shifts"][1], p["iwt"][0], p["iwt"][1])


def run(ctx, pictures, depth, filt, dtype, seed=0):
    lay, specs = layout_of(pictures, dtype)
    blk = G.GuardedBlock(ctx, lay, seed=seed)
    try:
        jobs, expected, want_routes = [], {}, {"fused": 0, "two_pass": 0}
        for n, (p, (s, d)) in enumerate(zip(pictures, specs)):
            buf = packed_bytes(p["fmt"], p["src"][0], p["src"][1], 1000 * seed + n)
            blk[s].upload(buf)
            frame = U.chain(buf, p["fmt"], p["src"], p["pic"], p["iwt"], p["shifts"], dtype)
            for sp, a in zip(d, frame):
                expected[sp] = O.forward_iwt(a, depth, filt)
            jobs.append(job_of(blk, p, s, d))
            want_routes[expected_route(p, filt, dtype)] += 1
        ctx.synchronize()
        ctx.unpack_routes(reset=True)
        ctx.profile_reset()
        ctx.profile_enable(True)
        try:
            ctx.unpack_iwt_batch(jobs, depth, filt)
            ctx.synchronize()
            prof = ctx.profile_read()
        finally:
            ctx.profile_enable(False)
        routes = ctx.unpack_routes(reset=True)
        assert routes == want_routes, (routes, want_routes)
        if not want_routes["two_pass"]:
            assert prof["convert"][1] == 0, prof["convert"]
        blk.check(expected)
    finally:
        blk.free()


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("filt", range(7))
def test_fused_pictures_of_every_format(ctx, filt, depth, dtype):
    """The natural pairs: the u8 formats and v210 / v216 into s16 and s32, AY64 into s32 and (truncated) s16."""
    sizes = SIZES + ([DEPTH1_SIZE] if depth == 1 else [])
    pictures = [pic(fmt, size) for fmt in U.PACKED for size in sizes]
    run(ctx, pictures, depth, filt, dtype, seed=10 * filt + depth)


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("filt", range(7))
def test_routes_mix_in_one_call(ctx, filt, dtype):
    """Aligned pictures are FUSED; an odd source stride, a source pointer off a 16-byte boundary and a chroma change
    (u8 formats only: the reference resamples no other depth) are TWO_PASS -- in the same call."""
    depth = 1 + filt % 3
    pictures = [pic(U.UYVY, SIZES[1]), pic(U.UYVY, SIZES[1], src_pad=1), pic(U.V210, SIZES[2], src_pad=3),
                pic(U.V210, SIZES[2]), pic(U.AYUV, SIZES[2], src_skew=4), pic(U.UYVY, SIZES[0], shifts=(1, 1)),
                pic(U.AYUV, SIZES[1], shifts=(1, 0)), pic(U.AY64, SIZES[0], src_skew=2), pic(U.V216, SIZES[0], src_pad=8),
                pic(U.AY64, SIZES[2])]
    assert "two_pass" in {expected_route(p, filt, dtype) for p in pictures}
    run(ctx, pictures, depth, filt, dtype, seed=100 + filt)


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
def test_equals_the_plane_layers_chain(ctx, dtype):
    """schro_hip_unpack_batch into the packed format's own depth, schro_hip_unpack_batch (planar source) into the
    transform frame, schro_hip_iwt_batch: the same coefficients, bit for bit, for FUSED and TWO_PASS pictures."""
    depth, filt = 3, 1
    pictures = [pic(fmt, size) for fmt in U.PACKED for size in SIZES[1:]] + [pic(U.UYVY, SIZES[1], src_pad=1),
                                                                              pic(U.AYUV, SIZES[2], shifts=(1, 1))]
    lay, specs = layout_of(pictures, dtype)
    blk = G.GuardedBlock(ctx, lay, seed=5)
    try:
        jobs, first, second, transform, outs = [], [], [], [], []
        for n, (p, (s, d)) in enumerate(zip(pictures, specs)):
            blk[s].upload(packed_bytes(p["fmt"], p["src"][0], p["src"][1], n))
            jobs.append(job_of(blk, p, s, d))
            hs, vs = p["shifts"]
            (w, h), (iw, ih) = p["pic"], p["iwt"]
            own = U.NATURAL[p["fmt"]][0]
            a = [ctx.plane(U.shifted(h, vs if k else 0), U.shifted(w, hs if k else 0), own) for k in range(3)]
            b = [ctx.plane(U.shifted(ih, vs if k else 0), U.shifted(iw, hs if k else 0), dtype) for k in range(3)]
            c = [ctx.plane(U.shifted(ih, vs if k else 0), U.shifted(iw, hs if k else 0), dtype) for k in range(3)]
            first.append(((blk[s], p["fmt"], p["src"][0], p["src"][1]), a, hs, vs, w, h))
            second.append(((a, hs, vs, w, h), b, hs, vs, iw, ih))
            transform += list(zip(b, c))
            outs.append(c)
        ctx.unpack_batch(first)
        ctx.unpack_batch(second)
        ctx.iwt_batch(transform, depth, filt)
        ctx.unpack_iwt_batch(jobs, depth, filt)
        ctx.synchronize()
        expected = {}
        for (s, d), c in zip(specs, outs):
            for sp, plane in zip(d, c):
                expected[sp] = plane.download()
        blk.check(expected)
    finally:
        blk.free()


# (transform size, picture size, source size less the picture size): pictures far smaller than their transform, so that whole
# tiles of the packed level 0 lie in the edge extension -- every coordinate rows_load_packed clamps is xmax / ymax there --,
# one of them cropped out of a source larger than it by more than a tile, and the smallest picture there is
EXTENSION_SIZES = [((352, 160), (41, 11), (1, 0)), ((352, 160), (40, 12), (360, 158)), ((352, 160), (6, 2), (0, 0)),
                   ((64, 32), (1, 1), (1, 0))]


def tiles_wholly_in_the_extension(size, filt, dtype):
    """The luma tiles (tx, ty) of the forward wavelet's level 0 whose region -- useful part and halo, from the library's
    own tile lengths (sa.unpack_geometry) -- begins right of and below the last picture sample."""
    (iw, ih), (w, h), _delta = size
    uc, ur, hc, hr = sa.unpack_geometry()["iwt"][(filt, np.dtype(dtype).itemsize)]
    return [(tx, ty) for ty in range(-(-(ih // 2) // ur)) for tx in range(-(-(iw // 2) // uc))
            if 2 * (tx * uc - hc) >= w and 2 * (ty * ur - hr) >= h]


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("filt", range(7))
def test_the_cases_hold_tiles_that_lie_wholly_in_the_extension(filt, dtype):
    for size in EXTENSION_SIZES[:3]:
        assert tiles_wholly_in_the_extension(size, filt, dtype), (size, filt)
    # the deep crop: the source exceeds the picture by more than a tile's useful part either way
    uc, ur, _hc, _hr = sa.unpack_geometry()["iwt"][(filt, np.dtype(dtype).itemsize)]
    assert EXTENSION_SIZES[1][2][0] > 2 * uc and EXTENSION_SIZES[1][2][1] > 2 * ur
    # (what the sizes further up reach: pictures within 21 samples of their transform have no such tile)
    for size in SIZES + [DEPTH1_SIZE]:
        assert not tiles_wholly_in_the_extension(size, filt, dtype), size


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("filt", range(7))
def test_tiles_in_the_extension_and_deep_crops_on_both_routes(ctx, filt, depth, dtype):
    """Every format at every size of EXTENSION_SIZES with an aligned source (FUSED where the combination is), and in the same
    call one picture per size whose source stride or pointer sends it to the two passes."""
    pictures = [pic(fmt, size) for fmt in U.PACKED for size in EXTENSION_SIZES]
    for n, size in enumerate(EXTENSION_SIZES):
        fmt = U.PACKED[(n + filt) % len(U.PACKED)]
        pictures.append(pic(fmt, size, **({"src_pad": 2} if n & 1 else {"src_skew": 4 if fmt != U.AY64 else 2})))
    routes = {expected_route(p, filt, dtype) for p in pictures}
    bpp = np.dtype(dtype).itemsize
    some_fused = not FORCED_TWO_PASS and (FORCED_FUSED or any(filt in FUSED_FILTERS[(fmt, bpp)] for fmt in U.PACKED))
    assert "two_pass" in routes and ("fused" in routes) == some_fused       # (s16 Fidelity has no FUSED combination)
    run(ctx, pictures, depth, filt, dtype, seed=200 + 10 * filt + depth)


def test_refusals_are_the_chains(ctx):
    """What the chain refuses, the call refuses, nothing launched or counted."""
    good = pic(U.UYVY, SIZES[0])
    lay, specs = layout_of([good], np.int16, footprint=None)
    blk = G.GuardedBlock(ctx, lay, seed=9)
    try:
        s, d = specs[0]
        base = job_of(blk, good, s, d)

        def refused(depth=2, filt=1, **change):
            names = ("buf", "fmt", "sw", "sh", "w", "h", "dst", "hs", "vs", "iw", "ih")
            job = tuple(change.get(n, v) for n, v in zip(names, base))
            with pytest.raises(sa.SchroHipError) as e:
                ctx.unpack_iwt_batch([job], depth, filt)
            assert e.value.code == -1, e.value
            return str(e.value)

        ctx.unpack_routes(reset=True)
        assert "schrovirtframe.c:693" in refused(fmt=U.ARGB)
        assert "schrovirtframe.c:629" in refused(sw=63)
        assert "schrovirtframe.c:1549" in refused(fmt=U.V210, hs=1, vs=1)
        assert "schrovirtframe.c:1861" in refused(w=66, h=30, iw=96)
        refused(iw=60)                  # smaller than the picture
        refused(ih=34)                  # not a multiple of 1 << depth
        refused(depth=7)
        refused(filt=7)
        refused(w=0)
        assert ctx.unpack_routes() == {"fused": 0, "two_pass": 0}
        ctx.synchronize()
        blk.check({})
    finally:
        blk.free()


@pytest.mark.parametrize("complete", [1, 0], ids=["stage-complete", "enqueue-only"])
def test_frame_layer_equals_its_chain(ctx, complete):
    """schro_hipframe_unpack_iwt_transform against schro_hipframe_convert_input x 2 + schro_hipframe_iwt_transform, and both
    against the restated chain; with and without schro_hip_context_set_stage_completion."""
    import ctypes as C
    from schroedinger_amd import frames
    depth, filt = 2, 0
    (iw, ih), (w, h) = (160, 64), (150, 62)
    sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, complete))
    try:
        for n, (fmt, dtype) in enumerate([(U.UYVY, np.int16), (U.YUYV, np.int32), (U.AYUV, np.int16), (U.V210, np.int16),
                                          (U.V216, np.int32), (U.AY64, np.int32), (U.AY64, np.int16)]):
            own, hs, vs = U.NATURAL[fmt]
            buf = packed_bytes(fmt, w, h, 40 + n)
            host = frames.PackedHostFrame(fmt, w, h)
            host.rows[:, :buf.shape[1]] = buf
            packed = frames.DeviceFrame(ctx, fmt, w, h).upload(host)
            params = frames.make_params(wavelet_filter_index=filt, transform_depth=depth, iwt_luma_width=iw, iwt_luma_height=ih,
                                        iwt_chroma_width=iw >> hs, iwt_chroma_height=ih >> vs)
            fused = frames.DeviceFrame(ctx, frames.frame_format(dtype, hs, vs), iw, ih)
            a = frames.DeviceFrame(ctx, frames.frame_format(own, hs, vs), w, h)
            b = frames.DeviceFrame(ctx, frames.frame_format(dtype, hs, vs), iw, ih)
            ctx.unpack_iwt_transform(fused, packed, params, w, h)
            ctx.convert_input(a, packed)
            ctx.convert_input(b, a)
            sa.check(ctx.lib.schro_hipframe_iwt_transform(ctx.h, b.ptr(), C.byref(params)))
            ctx.synchronize()
            want = [O.forward_iwt(p, depth, filt) for p in U.chain(buf, fmt, (w, h), (w, h), (iw, ih), (hs, vs), dtype)]
            for k, (x, y, z) in enumerate(zip(fused.download(), b.download(), want)):
                assert np.array_equal(x, y) and np.array_equal(x, z), (hex(fmt), np.dtype(dtype).name, k)
            for f in (packed, fused, a, b):
                f.unref()
    finally:
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 1))
