"""schro_hip_iiwt_pack_wide_batch and its frame-layer calls on the device-free sanitizer libraries (run by
tests/test_wide_build.py in a child process, as tests/test_sanitizers.py runs tests/dry_run_cases.py): random geometries,
formats, shifts and alignments through both routes and the refusals, so that AddressSanitizer and
UndefinedBehaviorSanitizer see the job tables, the scratch-block offsets and the tile arithmetic.  Nothing is computed.

Not collected by a plain `pytest tests/` (the name): the product library has no dry mode."""
import ctypes as C
import os

import numpy as np
import pytest

import schroedinger_amd as sa
from schroedinger_amd import SubPlane, frames

if "dry" not in os.path.basename(os.environ.get("SCHRO_HIP_LIB", "")):
    pytest.skip("dry-run cases need SCHRO_HIP_LIB = a libschro_hip_dry_*.so", allow_module_level=True)

FORMATS = [(sa.FORMAT_V216, 1), (sa.FORMAT_ARGB, 0), (sa.FORMAT_AY64, 0)]
ROW = {sa.FORMAT_V216: lambda w: 8 * (w // 2), sa.FORMAT_ARGB: lambda w: 4 * w, sa.FORMAT_AY64: lambda w: 8 * w}


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def test_random_calls_on_both_routes(ctx):
    rng = np.random.default_rng(1010)
    for rnd in range(120):
        depth, filt = int(rng.integers(1, 5)), int(rng.integers(0, 7))
        dtype = (np.int16, np.int32)[int(rng.integers(0, 2))]
        jobs, keep = [], []
        for n in range(int(rng.integers(1, 6))):
            fmt, hs = FORMATS[int(rng.integers(0, 3))]
            unit = 1 << (depth + hs)
            w, h = unit * int(rng.integers(1, 600 // unit + 1)), (1 << depth) * int(rng.integers(1, 300 // (1 << depth) + 1))
            ow, oh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            co = [ctx.plane(h, w if k == 0 else w >> hs, dtype) for k in range(3)]
            pad = (0, 0, 8, 4)[int(rng.integers(0, 4))]         # (8, 4: the two passes)
            dst = ctx.plane(oh, ROW[fmt](ow) + 48, np.uint8, stride=-(-(ROW[fmt](ow) + 48) // 16) * 16 + pad)
            jobs.append((co, hs, 0, dst, ow, oh, fmt, int(rng.integers(0, 8 * np.dtype(dtype).itemsize))))
            keep += co + [dst]
        ctx.wide_routes(reset=True)
        ctx.iiwt_pack_wide_batch(jobs, depth, filt)
        assert sum(ctx.wide_routes(reset=True).values()) == len(jobs)
        ctx.synchronize()
        [p.free() for p in keep]


def test_refusals(ctx):
    co = [ctx.plane(32, 64, np.int32), ctx.plane(32, 32, np.int32), ctx.plane(32, 32, np.int32)]
    dst = ctx.plane(32, 512, np.uint8)
    good = (co, 1, 0, dst, 64, 32, sa.FORMAT_V216, 0)
    for bad in [good[:6] + (sa.FORMAT_V210, 0), good[:7] + (32,), good[:7] + (-1,), good[:4] + (65, 32, sa.FORMAT_V216, 0),
                (co, 0, 0, dst, 64, 32, sa.FORMAT_V216, 0), (co, 1, 0, dst, 64, 32, sa.FORMAT_AY64, 0)]:
        with pytest.raises(sa.SchroHipError):
            ctx.iiwt_pack_wide_batch([bad], 3, 0)
    with pytest.raises(sa.SchroHipError):
        ctx.iiwt_pack_wide_batch([good], 6, 0)
    assert ctx.wide_routes(reset=True) == {"level": 0, "two_pass": 0}
    [p.free() for p in co + [dst]]


def test_frame_layer(ctx):
    lib = ctx.lib
    for fmt, hs in FORMATS:
        for dtype in (np.int16, np.int32):
            params = frames.make_params(wavelet_filter_index=2, transform_depth=3, iwt_luma_width=320, iwt_luma_height=240,
                                        iwt_chroma_width=320 >> hs, iwt_chroma_height=240, num_refs=0)
            tf = frames.DeviceFrame(ctx, frames.frame_format(dtype, hs, 0), 320, 240)
            packed = frames.DeviceFrame(ctx, fmt, 318, 236)
            sa.check(lib.schro_frame_inverse_iwt_transform_convert_hip(packed.ptr(), tf.ptr(), C.byref(params)))
            sa.check(lib.schro_frame_inverse_iwt_transform_shift_convert_hip(packed.ptr(), tf.ptr(), C.byref(params), 3))
            assert lib.schro_frame_inverse_iwt_transform_shift_convert_hip(packed.ptr(), tf.ptr(), C.byref(params), 64) != 0
            assert lib.schro_frame_inverse_iwt_transform_combine_convert_hip(packed.ptr(), tf.ptr(), C.byref(params), tf.ptr()) != 0
            packed.unref()
            tf.unref()
