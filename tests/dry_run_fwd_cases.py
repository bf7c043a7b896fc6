"""schro_hip_iwt_batch and schro_hipframe_iwt_transform on the device-free sanitizer libraries (run by
tests/test_iwt_forward_api.py in child processes, as tests/test_sanitizers.py runs tests/dry_run_cases.py): 100 random
forward batches -- filters, depths, sample types, sizes, strides and alignments --, every refusal and the frame layer,
so that ThreadSanitizer, AddressSanitizer and UndefinedBehaviorSanitizer see the job tables, the scratch offsets and the
tile arithmetic.  Nothing is computed.

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


def test_100_random_forward_batches(ctx):
    for depth, filt, dtype, planes in encoder_front_draws.forward_batches(100):
        pairs, keep = [], []
        for w, h, src_stride, dst_stride in planes:
            pair = (ctx.plane(h, w, dtype, stride=src_stride), ctx.plane(h, w, dtype, stride=dst_stride))
            pairs.append(pair)
            keep += pair
        ctx.iwt_batch(pairs, depth, filt)
        ctx.synchronize()
        [p.free() for p in keep]


def refused(ctx, plane, depth=2, filt=0, bpp=2):
    arr = (_lib.IwtFwdPlane * 1)(plane)
    rc = ctx.lib.schro_hip_iwt_batch(ctx.h, arr, 1, depth, filt, bpp)
    msg = ctx.lib.schro_hip_last_error()
    return rc, (msg.decode() if msg else "")


def test_refusals(ctx):
    src, dst = ctx.plane(64, 64, np.int16, stride=128), ctx.plane(64, 64, np.int16, stride=128)
    P = _lib.IwtFwdPlane
    good = P(src.ptr, 128, dst.ptr, 128, 64, 64)
    assert refused(ctx, good)[0] == 0
    cases = {
        "width not a multiple of 2^depth": (P(src.ptr, 128, dst.ptr, 128, 62, 64), {}),
        "height not a multiple of 2^depth": (P(src.ptr, 128, dst.ptr, 128, 64, 30), {}),
        "src stride shorter than a row": (P(src.ptr, 126, dst.ptr, 128, 64, 64), {}),
        "dst stride shorter than a row": (P(src.ptr, 128, dst.ptr, 64, 64, 64), {}),
        "src stride not a multiple of the sample size": (P(src.ptr, 129, dst.ptr, 128, 64, 64), {}),
        "dst stride not a multiple of the sample size (s32)": (P(src.ptr, 128, dst.ptr, 130, 32, 32), {"bpp": 4}),
        "in place": (P(src.ptr, 128, src.ptr, 128, 64, 64), {}),
        "dst overlaps src": (P(src.ptr, 128, src.ptr + 128 * 16, 128, 64, 32), {"depth": 1}),
        "filter 7": (good, {"filt": 7}),
        "filter -1": (good, {"filt": -1}),
        "depth 0": (good, {"depth": 0}),
        "depth 7": (P(src.ptr, 256, dst.ptr, 256, 128, 128), {"depth": 7}),
        "bytes_per_sample 1": (good, {"bpp": 1}),
        "bytes_per_sample 3": (good, {"bpp": 3}),
        "bytes_per_sample 8": (good, {"bpp": 8}),
    }
    for name, (plane, kw) in cases.items():
        rc, msg = refused(ctx, plane, **kw)
        assert rc == EINVAL, (name, rc)
        assert "iwt_batch" in msg, (name, msg)
    # (the wrapper raises with the message: a 48 x 48 plane has no fifth level)
    s48, d48 = src.level_view(0), dst.level_view(0)
    s48.width = s48.height = d48.width = d48.height = 48
    with pytest.raises(sa.SchroHipError, match="multiple of 2\\^depth"):
        ctx.iwt_batch([(s48, d48)], 5, 0)
    assert ctx.lib.schro_hip_iwt_batch(None, (P * 1)(good), 1, 2, 0, 2) == EINVAL
    assert ctx.lib.schro_hip_iwt_batch(ctx.h, None, 1, 2, 0, 2) == EINVAL
    assert ctx.lib.schro_hip_iwt_batch(ctx.h, (P * 1)(good), 0, 2, 0, 2) == EINVAL
    [p.free() for p in (src, dst)]


def test_frame_layer(ctx):
    lib = ctx.lib
    for hs, vs in ((1, 1), (1, 0), (0, 0)):
        for dtype in (np.int16, np.int32):
            for stage in (1, 0):
                sa.check(lib.schro_hip_context_set_stage_completion(ctx.h, stage))
                params = frames.make_params(wavelet_filter_index=2, transform_depth=3, iwt_luma_width=320, iwt_luma_height=240,
                                            iwt_chroma_width=320 >> hs, iwt_chroma_height=240 >> vs)
                fr = frames.DeviceFrame(ctx, frames.frame_format(dtype, hs, vs), 320, 240)
                sa.check(lib.schro_hipframe_iwt_transform(ctx.h, fr.ptr(), C.byref(params)))
                ctx.synchronize()
                params.iwt_luma_width = 328     # (larger than the frame)
                assert lib.schro_hipframe_iwt_transform(ctx.h, fr.ptr(), C.byref(params)) == EINVAL
                params.iwt_luma_width, params.transform_depth = 320, 5  # (240 is not a multiple of 32)
                assert lib.schro_hipframe_iwt_transform(ctx.h, fr.ptr(), C.byref(params)) == EINVAL
                fr.unref()
    sa.check(lib.schro_hip_context_set_stage_completion(ctx.h, 1))
    u8 = frames.DeviceFrame(ctx, sa.FORMAT_U8_420, 320, 240)
    params = frames.make_params(wavelet_filter_index=0, transform_depth=2, iwt_luma_width=320, iwt_luma_height=240,
                                iwt_chroma_width=160, iwt_chroma_height=120)
    assert lib.schro_hipframe_iwt_transform(ctx.h, u8.ptr(), C.byref(params)) == EINVAL
    assert lib.schro_hipframe_iwt_transform(None, u8.ptr(), C.byref(params)) == EINVAL
    assert lib.schro_hipframe_iwt_transform(ctx.h, None, C.byref(params)) == EINVAL
    u8.unref()
