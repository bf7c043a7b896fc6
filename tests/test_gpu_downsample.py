"""GPU: schro_hip_downsample_batch / schro_hipframe_downsample against tests/analysis_ref.py (schro_frame_downsample +
schro_frame_mc_edgeextend), bit for bit: every size class of the kernel (pictures narrower than a group of four, odd
sizes, the last columns of odd and even widths, more than one tile in both directions), random pictures and the 0 / 255
checkerboard, aprons of 0, 8 and 32 samples compared sample for sample, a five-level 4:2:0 pyramid with one call per
level, batches of unlike planes in both orders, the source left as it was and the write footprint (tests/guard_lib.py)."""
import numpy as np
import pytest

import analysis_ref as A
import guard_lib as G
import schroedinger_amd as sa
from schroedinger_amd import frames

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (7, 8), (8, 8), (9, 7), (17, 33), (64, 48), (130, 70), (321, 241), (1920, 1080)]
EXTENSIONS = (0, 8, 32)


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def want(src, ext):
    return A.edgeextend(A.downsample(src), ext)


def dst_plane(ctx, src_shape, ext, stride=None):
    h, w = src_shape
    return ctx.plane((h + 1) // 2 + 2 * ext, (w + 1) // 2 + 2 * ext, np.uint8, stride)


@pytest.mark.parametrize("w,h", SIZES)
def test_every_size_and_extension_random_and_checkerboard(ctx, w, h):
    srcs = [A.picture(w, h, 31 * w + h), A.checkerboard(w, h)]
    jobs, keep = [], []
    for src in srcs:
        d_src = ctx.upload(src)
        for ext in EXTENSIONS:
            d = dst_plane(ctx, src.shape, ext).fill(0x5a)
            jobs.append((d_src, d, ext))
        keep.append(d_src)
    ctx.downsample_batch(jobs)          # one launch: six destinations of three sizes
    for n, (d_src, d, ext) in enumerate(jobs):
        assert np.array_equal(d.download(), want(srcs[n // 3], ext)), (w, h, ext, n // 3)
    for d_src, src in zip(keep, srcs):
        assert np.array_equal(d_src.download(), src)            # the source is left as it was
    [p.free() for p in keep + [j[1] for j in jobs]]


def test_five_level_pyramid_of_a_420_picture_one_call_per_level(ctx):
    ext = 32
    comps = [A.picture(176, 144, 1), A.picture(88, 72, 2), A.picture(88, 72, 3)]
    level = [ctx.upload(c) for c in comps]
    keep, refs = list(level), comps
    for n in range(5):
        dsts = [dst_plane(ctx, r.shape, ext) for r in refs]
        ctx.downsample_batch([(s, d, ext) for s, d in zip(level, dsts)])
        refs = [A.downsample(r) for r in refs]
        for d, r in zip(dsts, refs):
            assert np.array_equal(d.download(), A.edgeextend(r, ext)), n
        # the next level reads the picture inside this level's apron
        level = [sa.SubPlane(d, ext, ext, r.shape[0], r.shape[1]) for d, r in zip(dsts, refs)]
        keep += dsts
    assert refs[0].shape == (5, 6) and refs[1].shape == (3, 3)
    [p.free() for p in keep]


def test_the_frame_layer_downsamples_all_three_components(ctx):
    for (w, h, hs, vs, ext) in ((176, 144, 1, 1, 32), (75, 43, 1, 0, 8), (33, 17, 0, 0, 0)):
        cw, ch = -(-w // (1 << hs)), -(-h // (1 << vs))
        comps = [A.picture(w, h, 11), A.picture(cw, ch, 12), A.picture(cw, ch, 13)]
        src = frames.DeviceFrame(ctx, frames.frame_format(np.uint8, hs, vs), w, h).upload(frames.HostFrame(comps, hs, vs))
        planes = [dst_plane(ctx, c.shape, ext).fill(0xa5) for c in comps]
        dest = frames.PlaneFrame(ctx, planes, ext, hs, vs)
        sa.check(ctx.lib.schro_hipframe_downsample(dest.ptr(), src.ptr()))
        for p, c in zip(planes, comps):
            assert np.array_equal(p.download(), want(c, ext)), (w, h, ext)
        for got, c in zip(src.download(), comps):
            assert np.array_equal(got, c)
        src.unref()
        [p.free() for p in planes]


def test_a_batch_of_unlike_planes_in_both_orders(ctx):
    shapes = [(1080, 1920, 32), (5, 3, 8), (241, 321, 0), (72, 88, 32), (1, 1, 8), (33, 17, 1)]
    srcs = [A.picture(w, h, 100 + n) for n, (h, w, _) in enumerate(shapes)]
    wants = [want(s, e) for s, (_, _, e) in zip(srcs, shapes)]
    d_srcs = [ctx.upload(s) for s in srcs]
    for order in (list(range(len(shapes))), list(range(len(shapes)))[::-1]):
        dsts = [dst_plane(ctx, srcs[n].shape, shapes[n][2]).fill(0) for n in order]
        ctx.downsample_batch([(d_srcs[n], d, shapes[n][2]) for n, d in zip(order, dsts)])
        for n, d in zip(order, dsts):
            assert np.array_equal(d.download(), wants[n]), (order, n)
        [d.free() for d in dsts]
    [p.free() for p in d_srcs]


@pytest.mark.parametrize("skew", [0, 1, 2, 3])
def test_write_footprint_and_source_untouched(ctx, skew):
    """Every destination alignment (the groups of four start where the stores are dword-aligned), strides that are no
    multiple of four, aprons: nothing outside the picture plus its apron is written, the sources keep their bytes."""
    cases = [(321, 241, 8, 5), (130, 70, 32, 0), (9, 7, 0, 3), (64, 48, 1, 1)]      # (w, h, ext, stride padding)
    L = G.Layout()
    specs = []
    for (w, h, ext, pad) in cases:
        s = L.plane(h, w, np.uint8, stride=w + pad, skew=skew, footprint=None)
        dw, dh = (w + 1) // 2 + 2 * ext, (h + 1) // 2 + 2 * ext
        d = L.plane(dh, dw, np.uint8, stride=dw + pad, align=64, skew=(skew * 7) % 64)
        specs.append((s, d))
    block = G.GuardedBlock(ctx, L, seed=77 + skew)
    srcs = [A.picture(w, h, 5 + n) for n, (w, h, _, _) in enumerate(cases)]
    for (s, d), a in zip(specs, srcs):
        block[s].upload(a)
    ctx.downsample_batch([(block[s], block[d], c[2]) for (s, d), c in zip(specs, cases)])
    ctx.synchronize()
    expected = {d: want(a, c[2]) for (s, d), a, c in zip(specs, srcs, cases)}
    expected.update({s: a for (s, d), a in zip(specs, srcs)})
    block.check(expected)
    block.free()
