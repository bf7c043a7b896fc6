"""schro_hip_histogram_batch and the frame layer's schro_hipframe_subband_histograms on the device-free sanitizer libraries
(run by tests/test_histogram_api.py in child processes, as tests/test_sanitizers.py runs tests/dry_run_cases.py): every
refusal, random batches -- sizes, skips, forms, sample types, odd starts -- and the frame layer with a geometry change and
both queues, so that AddressSanitizer, UndefinedBehaviorSanitizer and ThreadSanitizer see the job table, the band records
and the table rebuild.  Nothing is computed: the counts come back as the zeros the call's clear left.

Not collected by a plain `pytest tests/` (the name): the product library has no dry mode."""
import os

import numpy as np
import pytest

import hist_cases as HC
import hist_ref as H
import schroedinger_amd as sa
from schroedinger_amd import frames

if "dry" not in os.path.basename(os.environ.get("SCHRO_HIP_LIB", "")):
    pytest.skip("dry-run cases need SCHRO_HIP_LIB = a libschro_hip_dry_*.so", allow_module_level=True)


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def test_refusals(ctx):
    assert HC.refusal_cases(ctx) >= 12


def test_60_random_batches(ctx):
    rng = np.random.default_rng(1414)
    for rnd in range(60):
        dtype = (np.int16, np.int32)[int(rng.integers(0, 2))]
        b = np.dtype(dtype).itemsize
        jobs, keep = [], []
        for n in range(int(rng.integers(1, 5))):
            h, pitch = int(rng.integers(1, 80)), int(rng.integers(1, 300))
            co = ctx.plane(h, pitch, dtype, stride=pitch * b)
            keep.append(co)
            bands = []
            for _ in range(int(rng.integers(1, 12))):
                w, bh = int(rng.integers(1, pitch + 1)), int(rng.integers(1, h + 1))
                step = int(rng.integers(1, h // bh + 1))
                rows = (bh - 1) * step + 1
                y0, x0 = int(rng.integers(0, h - rows + 1)), int(rng.integers(0, pitch - w + 1))
                bands.append(((y0 * pitch + x0) * b, pitch * b * step, w, bh, 1 << int(rng.integers(0, 4)), int(rng.integers(0, 2))))
            jobs.append((co, bands))
        for got, (_, bands) in zip(ctx.histogram_batch(jobs), jobs):
            assert got.shape == (len(bands), 105) and not got.any()
        [p.free() for p in keep]


def test_frame_layer(ctx):
    lib = ctx.lib
    for (dtype, w, h, depth, shift, intra) in ((np.int16, 64, 48, 2, 1, 1), (np.int32, 64, 48, 3, 0, 0), (np.int16, 16, 16, 3, 1, 1),
                                               (np.int16, 64, 48, 2, 1, 0), (np.int32, 8, 8, 3, 1, 1)):
        # (16 x 16 at depth 3: a 1 x 1 chroma LL; 8 x 8: the coarsest chroma bands are 0 x 0 -- skipped, n = 0)
        fmt = frames.frame_format(dtype, shift, shift)
        iwt = frames.DeviceFrame(ctx, fmt, w, h)
        params = frames.make_params(transform_depth=depth, num_refs=0 if intra else 1, iwt_luma_width=w, iwt_luma_height=h,
                                    iwt_chroma_width=w >> shift, iwt_chroma_height=h >> shift)
        for q in (0, 1, 0):
            ctx.select_queue(q)
            n, bins, ovf = ctx.subband_histograms(iwt, params)
            assert bins.shape == (3 * (1 + 3 * depth), 104) and not bins.any() and not ovf.any()
            # n is the host's arithmetic: sampled rows x width x skip of every luma sub-band
            sizes = [(h >> (depth - (H.position(i) >> 2)), w >> (depth - (H.position(i) >> 2)), H.band_skip(i)) for i in range(1 + 3 * depth)]
            assert n[:len(sizes)].tolist() == [-(-bh // sk) * sk * bw for bh, bw, sk in sizes]
            if (w, h) == (8, 8):
                assert n[len(sizes):len(sizes) + 4].tolist() == [0, 0, 0, 0] and n[len(sizes) + 4] == 1
        ctx.select_queue(0)
        # refusals of the frame layer: no frame, no histograms, a depth out of range, a transform larger than the frame
        assert lib.schro_hipframe_subband_histograms(None, params, None, None) == HC.EINVAL
        assert b"hipframe_subband_histograms" in lib.schro_hip_last_error()
        with pytest.raises(sa.SchroHipError):
            ctx.subband_histograms(iwt, frames.make_params(transform_depth=7, iwt_luma_width=w, iwt_luma_height=h,
                                                           iwt_chroma_width=w >> shift, iwt_chroma_height=h >> shift))
        with pytest.raises(sa.SchroHipError):
            ctx.subband_histograms(iwt, frames.make_params(transform_depth=depth, iwt_luma_width=2 * w, iwt_luma_height=h,
                                                           iwt_chroma_width=w >> shift, iwt_chroma_height=h >> shift))
        host = frames.HostFrame([np.zeros((h, w), dtype), np.zeros((h >> shift, w >> shift), dtype), np.zeros((h >> shift, w >> shift), dtype)],
                                shift, shift)
        with pytest.raises(sa.SchroHipError):
            ctx.subband_histograms(host, params)
        iwt.unref()
