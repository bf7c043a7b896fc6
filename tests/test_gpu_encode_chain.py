"""GPU: the VC-2 low-delay intra chain with the coefficient planes staying on the device -- picture -> schro_hip_iwt_batch ->
schro_hip_lowdelay_encode_batch -> schro_hip_lowdelay_batch -> schro_hip_iiwt_batch, no host trip in between -- so that
what one stage writes is checked as what the next one reads: strides, the sub-band layout, the s16 values, the LL band's
position.  The bytes and base indices equal tests/lowdelay_enc_ref.py's on the oracle's forward transform of the
picture; the final pictures equal the oracle's inverse transform of the oracle's slice decoder's planes of those
bytes; everything exactly.  All planes and buffers of a draw are carved from one guarded block (tests/guard_lib.py): the
pictures are not written, and nothing beside the planes, the slices, the indices and the count is.

The draws are encoder_tail_draws.chain_draws (pixel-range s16 pictures, every filter of the forward transform, depth
1 .. 3, the three chroma formats, a geometry whose serial launch stays in LDS and one that leaves it, then seeded
geometries up to 128 x 96); SCHRO_FUZZ_SCALE multiplies their number and SCHRO_FUZZ_SEED shifts the seeds, as in
tests/test_gpu_encoder_fuzz.py.  A draw whose slices over-run, or whose slice sizes fall in the length_field class of
lowdelay_enc_cases.CASES, cannot come back from any decoder: there the encoder's outputs alone are compared, and the
test asserts that this happens to at most one draw in five."""
import ctypes as C
import os

import numpy as np
import pytest

import encoder_tail_draws as D
import guard_lib as G
import lowdelay_enc_cases as K
import schroedinger_amd as sa
from schroedinger_amd import frames
from test_gpu_iwt_forward import pixel_range

SCALE = int(os.environ.get("SCHRO_FUZZ_SCALE", "1"))
SEED = int(os.environ.get("SCHRO_FUZZ_SEED", "0"))

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(360 + 60 * SCALE)]


def nbytes_of(P):
    nslices = P["n_horiz_slices"] * P["n_vert_slices"]
    return nslices, P["slice_bytes_num"] * nslices // P["slice_bytes_denom"]


def test_chain_on_the_plane_layer(ctx):
    draws = without_decode = 0
    for draw in D.chain_draws(SCALE, SEED):
        P, depth, filt, tag = draw["P"], draw["depth"], draw["filt"], draw["tag"]
        pictures = D.chain_pictures(draw, pixel_range)
        coeffs, res, planes, back = D.chain_expected(draw, pictures)
        nslices, nbytes = nbytes_of(P)
        lay = G.Layout()

        def three(name, footprint, pads):
            return [lay.plane(p.shape[0], p.shape[1], np.int16, stride=p.shape[1] * 2 + pads[k], footprint=footprint, name="%s%d" % (name, k))
                    for k, p in enumerate(pictures)]

        src, co = three("picture", None, (0, 0, 0)), three("coefficients", "rect", draw["pads"])
        sl = lay.span(nbytes, skew=draws % 4, footprint=("bytes", nbytes), name="slices")
        ix = lay.span(nslices, skew=1, footprint=("bytes", nslices), name="index")
        cn = lay.span(4, footprint=("bytes", 4), name="count")
        dec, out = three("decoded", "rect", draw["pads"][::-1]), three("back", "rect", (0, 2, 0))
        blk = G.GuardedBlock(ctx, lay, seed=nbytes)
        try:
            for s, p in zip(src, pictures):
                blk[s].upload(p)
            ctx.iwt_batch([(blk[s], blk[c]) for s, c in zip(src, co)], depth, filt)
            ctx.lowdelay_encode_batch([([blk[c] for c in co], blk[sl], blk[ix], blk[cn])], P)
            expected = dict(zip(co, coeffs))
            if planes is not None:
                # (a fresh decode target holds the canary: the decoder writes every sample of the iwt planes)
                ctx.lowdelay_batch([(blk[sl], [blk[d] for d in dec])], P)
                ctx.iiwt_batch([(blk[d], blk[o]) for d, o in zip(dec, out)], depth, filt)
                expected.update(zip(dec, planes))
                expected.update(zip(out, back))
            ctx.synchronize()
            raw = blk.raw()
            data, index = sl.payload(raw)[0], ix.payload(raw)[0]
            count = int(cn.payload(raw).view(np.uint32)[0, 0])
            assert index.tolist() == res["index"].tolist(), tag + ("indices", index.tolist(), res["index"].tolist())
            assert count == res["count"], tag + ("over-run count", count, res["count"])
            assert data.size == res["bytes"].size, tag + ("bytes", data.size, res["bytes"].size)
            bad = np.flatnonzero(data != res["bytes"])
            assert bad.size == 0, tag + ("%d bytes differ, first at %d" % (bad.size, bad[0] if bad.size else -1),)
            try:
                if planes is None:
                    # the planes the decode half would have written keep their canary: declare them unwritten
                    for s in dec + out:
                        s.footprint = None
                blk.check(expected)
            except AssertionError as e:
                raise AssertionError("%r: %s" % (tag, e)) from e
        finally:
            blk.free()
        draws += 1
        without_decode += planes is None
    assert without_decode * D.CHAIN_SKIP_CAP <= draws, ("draws without the decode half", without_decode, "of", draws)


def test_chain_on_the_frame_layer(ctx):
    """The same chain from a device frame: schro_hipframe_iwt_transform transforms the frame's components in place,
    schro_hip_encode_lowdelay_transform_data (ctx.encode_lowdelay) reads them there; the bytes then go through the plane
    layer's decoder and inverse transform.  80 x 40 4:2:2 at depth 3 in 5 x 3 slices (5 x 5 chroma LL band: rectangles 1 and
    2 high), filter 1; the frame's components are the iwt sizes."""
    draw = dict(P=None, filt=1, depth=3, fmt=422, seeds=[71, 72, 73], decodes=True, tag=("frame layer",))
    P = draw["P"] = K.params(80, 40, 422, 3, 5, 3, 700, 3)
    assert draw["decodes"] == (not D.length_field_class(P))
    pictures = D.chain_pictures(draw, pixel_range)
    coeffs, res, planes, back = D.chain_expected(draw, pictures)
    assert res["count"] == 0 and planes is not None
    assert (P["iwt_chroma_width"], P["iwt_chroma_height"]) == (P["iwt_luma_width"] >> 1, P["iwt_luma_height"])
    params = frames.make_params(wavelet_filter_index=draw["filt"], transform_depth=3, iwt_luma_width=P["iwt_luma_width"],
                                iwt_luma_height=P["iwt_luma_height"], iwt_chroma_width=P["iwt_chroma_width"],
                                iwt_chroma_height=P["iwt_chroma_height"])
    f = frames.DeviceFrame(ctx, frames.frame_format(np.int16, 1, 0), P["iwt_luma_width"], P["iwt_luma_height"])
    try:
        f.upload(frames.HostFrame(pictures, 1, 0))
        sa.check(ctx.lib.schro_hipframe_iwt_transform(ctx.h, f.ptr(), C.byref(params)))
        data, index, count = ctx.encode_lowdelay(f, P)
        assert index.tolist() == res["index"].tolist() and count == 0
        assert np.array_equal(data, res["bytes"]), np.flatnonzero(data != res["bytes"])[:4]
        assert all(np.array_equal(a, c) for a, c in zip(f.download(), coeffs))          # the encoder does not write the frame
    finally:
        f.unref()
    dec = [ctx.plane(p.shape[0], p.shape[1], np.int16) for p in pictures]
    out = [ctx.plane(p.shape[0], p.shape[1], np.int16) for p in pictures]
    ctx.lowdelay_batch([(ctx.upload_bytes(data), dec)], P)
    ctx.iiwt_batch(list(zip(dec, out)), 3, draw["filt"])
    for k in range(3):
        assert np.array_equal(dec[k].download(), planes[k]) and np.array_equal(out[k].download(), back[k]), ("component", k)
    [p.free() for p in dec + out]
