"""schro_hip_downsample_batch, schro_hip_metric_scan_batch, schro_hipframe_downsample and
schro_rough_me_heirarchical_scan_nohint_hip on the device-free sanitizer libraries (run by tests/test_analysis_api.py in
child processes, as tests/test_iwt_forward_api.py runs tests/dry_run_fwd_cases.py): 100 random legal batches of each, every
refusal and the frame layer, so that ThreadSanitizer, AddressSanitizer and UndefinedBehaviorSanitizer see the job tables,
the validation and the tile arithmetic.  Nothing is computed.

Not collected by a plain `pytest tests/` (the name): the product library has no dry mode."""
import ctypes as C
import os

import numpy as np
import pytest

import encoder_front_draws
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

if "dry" not in os.path.basename(os.environ.get("SCHRO_HIP_LIB", "")):
    pytest.skip("dry-run cases need SCHRO_HIP_LIB = a libschro_hip_dry_*.so", allow_module_level=True)

EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def test_100_random_batches(ctx):
    for down, pictures, tables in encoder_front_draws.analysis_batches(100):
        jobs, keep = [], []
        for d in down:
            src = ctx.plane(d["h"], d["w"], np.uint8, stride=d["src_stride"])
            dst = ctx.plane((d["h"] + 1) // 2 + 2 * d["ext"], (d["w"] + 1) // 2 + 2 * d["ext"], np.uint8, stride=d["dst_stride"])
            jobs.append((src, dst, d["ext"]))
            keep += [src, dst]
        ctx.downsample_batch(jobs)
        pics = []
        for p in pictures:
            f, r = ctx.plane(p["h"], p["w"], np.uint8), ctx.plane(p["h"], p["w"], np.uint8)
            pics.append((f, r, p["ext"], p["scans"]))
            keep += [f, r]
        for res, met in ctx.metric_scan_batch(pics, tables=tables):
            keep += [res] + ([met] if met is not None else [])
        ctx.synchronize()
        [p.free() for p in keep]


def test_refusals(ctx):
    lib = ctx.lib
    src, dst = ctx.plane(48, 64, np.uint8, stride=64), ctx.plane(24 + 16, 32 + 16, np.uint8, stride=64)
    D = _lib.DownsamplePlane
    d00 = dst.ptr + 8 * 64 + 8

    def down(plane):
        rc = lib.schro_hip_downsample_batch(ctx.h, (D * 1)(plane), 1)
        return rc, (lib.schro_hip_last_error() or b"").decode()

    assert down(D(src.ptr, 64, 64, 48, d00, 64, 8))[0] == 0
    cases = {
        "zero width": D(src.ptr, 64, 0, 48, d00, 64, 8),
        "negative height": D(src.ptr, 64, 64, -1, d00, 64, 8),
        "src stride shorter than a row": D(src.ptr, 63, 64, 48, d00, 64, 8),
        "dst stride shorter than a row": D(src.ptr, 64, 64, 48, d00, 31, 0),
        "dst stride shorter than a row plus its aprons": D(src.ptr, 64, 64, 48, d00, 47, 8),
        "negative extension": D(src.ptr, 64, 64, 48, d00, 64, -1),
        "in place": D(src.ptr, 64, 64, 48, src.ptr, 64, 0),
        "dst overlaps src": D(src.ptr, 64, 64, 48, src.ptr + 64 * 47, 64, 0),
        "the apron overlaps src": D(src.ptr, 64, 64, 48, src.ptr + 64 * 48 + 8 * 64 - 1, 64, 8),
        "NULL src": D(None, 64, 64, 48, d00, 64, 8),
    }
    for name, plane in cases.items():
        rc, msg = down(plane)
        assert rc == EINVAL, (name, rc)
        assert "downsample_batch" in msg, (name, msg)
    assert lib.schro_hip_downsample_batch(None, (D * 1)(), 1) == EINVAL
    assert lib.schro_hip_downsample_batch(ctx.h, None, 1) == EINVAL
    assert lib.schro_hip_downsample_batch(ctx.h, (D * 1)(), 0) == EINVAL
    with pytest.raises(sa.SchroHipError, match="overlap"):
        sa.check(down(cases["in place"])[0])

    # ---- the scan: the assertions of schrometric.c:38-45 and the limits
    f, r = ctx.plane(48, 64, np.uint8), ctx.plane(48, 64, np.uint8)
    res = ctx.plane(4, 4, np.int32, stride=16)
    good = dict(x=8, y=8, block_width=8, block_height=8, ref_x=4, ref_y=4, scan_width=9, scan_height=9, gravity_x=0, gravity_y=0,
                dx=0, dy=0)

    def scan(pic=1, ext=8, w=64, h=48, fs=None, results=True, nscans=None, **kw):
        scans = np.zeros(2, sa.SCAN_DTYPE)
        for k, v in good.items():
            scans[k] = v
        clean = scans.copy()
        for k, v in kw.items():
            scans[k][1] = v     # (the SECOND scan of the SECOND picture is the bad one)
        P = _lib.MetricScanPicture
        arr = (P * 2)()
        for n, sc in enumerate((clean, scans)):
            arr[n] = P(f.ptr, f.stride, r.ptr, r.stride, 64, 48, 8, sc.ctypes.data_as(C.POINTER(_lib.MetricScan)), 2, res.ptr, None)
        arr[pic].width, arr[pic].height, arr[pic].extension = w, h, ext
        if fs is not None:
            arr[pic].frame_stride = fs
        if not results:
            arr[pic].results = None
        if nscans is not None:
            arr[pic].nscans = nscans
        rc = lib.schro_hip_metric_scan_batch(ctx.h, arr, 2)
        return rc, (lib.schro_hip_last_error() or b"").decode()

    assert scan()[0] == 0
    assert scan(block_width=0)[0] == 0 and scan(block_height=-3)[0] == 0     # empty blocks are legal
    per_scan = {
        "window of no width": dict(scan_width=0),
        "window of negative height": dict(scan_height=-1),
        "window over 42": dict(scan_width=43, ref_x=-8, gravity_x=-16),
        "window height over 42": dict(scan_height=43, ref_y=-8, gravity_y=-16),
        "block over 64 wide": dict(block_width=65),
        "block over 64 high": dict(block_height=65),
        "window starts in front of the apron": dict(ref_x=-9, gravity_x=-17),
        "window starts above the apron": dict(ref_y=-9, gravity_y=-17),
        "window ends behind the apron": dict(ref_x=64 + 8 - 8 - 9 + 2, gravity_x=64 + 8 - 8 - 9 + 2 - 8),
        "window ends below the apron": dict(ref_y=48 + 8 - 8 - 9 + 2, gravity_y=48 + 8 - 8 - 9 + 2 - 8),
        "gravity position left of the window": dict(gravity_x=-5),
        "gravity position right of the window": dict(gravity_x=5),
        "gravity position above the window": dict(gravity_y=-5),
        "gravity position below the window": dict(gravity_y=5),
    }
    for name, kw in per_scan.items():
        rc, msg = scan(**kw)
        assert rc == EINVAL, (name, rc)
        assert "metric_scan_batch: picture 1 scan 1" in msg, (name, msg)       # a refusal names the picture and the scan
    per_picture = {
        "zero width": dict(w=0), "negative height": dict(h=-4), "negative extension": dict(ext=-1),
        "stride shorter than a row": dict(fs=63), "no results": dict(results=False), "no scans": dict(nscans=0),
    }
    for name, kw in per_picture.items():
        rc, msg = scan(**kw)
        assert rc == EINVAL, (name, rc)
        assert "metric_scan_batch: picture 1" in msg, (name, msg)
    assert lib.schro_hip_metric_scan_batch(None, None, 1) == EINVAL
    assert lib.schro_hip_metric_scan_batch(ctx.h, None, 1) == EINVAL
    # the wrapper raises with the message
    bad = np.zeros(1, sa.SCAN_DTYPE)
    for k, v in dict(good, scan_width=43).items():
        bad[k] = v
    with pytest.raises(sa.SchroHipError, match="over the limit of 42"):
        ctx.metric_scan_batch([(f, r, 8, bad)])
    # schro_metric_scan_setup asserts dist > 0 and the window limit
    s = _lib.MetricScan(x=30, y=24, block_width=8, block_height=8)
    assert lib.schro_hip_metric_scan_setup(C.byref(s), 64, 48, 8, 0, 0, 0) == EINVAL
    assert lib.schro_hip_metric_scan_setup(C.byref(s), 64, 48, 32, 0, 0, 21) == EINVAL
    assert lib.schro_hip_metric_scan_setup(None, 64, 48, 8, 0, 0, 4) == EINVAL
    assert lib.schro_hip_metric_scan_setup(C.byref(s), 64, 48, 32, 0, 0, 20) == 0
    [p.free() for p in (src, dst, f, r, res)]


def test_frame_layer(ctx):
    lib = ctx.lib
    for stage in (1, 0):
        sa.check(lib.schro_hip_context_set_stage_completion(ctx.h, stage))
        for (w, h, hs, vs, ext) in ((176, 144, 1, 1, 32), (175, 143, 1, 0, 8), (33, 17, 0, 0, 0)):
            cw, ch = -(-w // (1 << hs)), -(-h // (1 << vs))
            src = frames.DeviceFrame(ctx, frames.frame_format(np.uint8, hs, vs), w, h)
            sizes = [((h + 1) // 2, (w + 1) // 2), ((ch + 1) // 2, (cw + 1) // 2), ((ch + 1) // 2, (cw + 1) // 2)]
            planes = [ctx.plane(a + 2 * ext, b + 2 * ext, np.uint8) for a, b in sizes]
            dest = frames.PlaneFrame(ctx, planes, ext, hs, vs)
            assert (dest.c.components[1].width, dest.c.components[1].height) == sizes[1][::-1]
            sa.check(lib.schro_hipframe_downsample(dest.ptr(), src.ptr()))
            ctx.synchronize()
            # a destination of another size, or of another format, is refused
            wrong = frames.PlaneFrame(ctx, [planes[1]] * 3, ext, hs, vs)
            if sizes[1] != sizes[0]:
                assert lib.schro_hipframe_downsample(wrong.ptr(), src.ptr()) == EINVAL
            assert lib.schro_hipframe_downsample(src.ptr(), src.ptr()) == EINVAL
            # the rough scan of the frame against itself, both references
            for shift, dist in ((0, 4), (2, 12)):
                P = frames.make_params(x_num_blocks=-(-w // 8) + 2, y_num_blocks=-(-h // 8) + 1, xbsep_luma=8, ybsep_luma=8)
                mvs = np.zeros(P.x_num_blocks * P.y_num_blocks, sa.MV_DTYPE)
                for ref in (0, 1):
                    sa.check(lib.schro_rough_me_heirarchical_scan_nohint_hip(src.ptr(), src.ptr(), C.byref(P), shift, dist, ref,
                                                                             mvs.ctypes.data_as(C.c_void_p)))
                assert (mvs["flags"] == 1).all()
                assert lib.schro_rough_me_heirarchical_scan_nohint_hip(src.ptr(), src.ptr(), C.byref(P), shift, dist, 2,
                                                                       mvs.ctypes.data_as(C.c_void_p)) == EINVAL
                assert lib.schro_rough_me_heirarchical_scan_nohint_hip(src.ptr(), src.ptr(), C.byref(P), shift, 0, 0,
                                                                       mvs.ctypes.data_as(C.c_void_p)) == EINVAL
                if w > 100:     # (a window of 43 positions around the blocks in the middle)
                    assert lib.schro_rough_me_heirarchical_scan_nohint_hip(src.ptr(), src.ptr(), C.byref(P), shift, 21, 0,
                                                                           mvs.ctypes.data_as(C.c_void_p)) == EINVAL
            src.unref()
            [p.free() for p in planes]
    sa.check(lib.schro_hip_context_set_stage_completion(ctx.h, 1))
    s16 = frames.DeviceFrame(ctx, sa.FORMAT_S16_420, 64, 48)
    assert lib.schro_hipframe_downsample(s16.ptr(), s16.ptr()) == EINVAL
    assert lib.schro_hipframe_downsample(None, s16.ptr()) == EINVAL
    assert lib.schro_rough_me_heirarchical_scan_nohint_hip(s16.ptr(), s16.ptr(), None, 0, 4, 0, None) == EINVAL
    mv = np.zeros(4, sa.MV_DTYPE)
    P = frames.make_params(x_num_blocks=2, y_num_blocks=2, xbsep_luma=8, ybsep_luma=8)
    assert lib.schro_rough_me_heirarchical_scan_nohint_hip(s16.ptr(), s16.ptr(), C.byref(P), 0, 4, 0, mv.ctypes.data_as(C.c_void_p)) == EINVAL
    s16.unref()
