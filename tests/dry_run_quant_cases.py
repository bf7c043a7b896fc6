"""schro_hip_quantise_batch, schro_hip_subtract_batch and the frame layer's schro_hipframe_quantise / _subtract on the
device-free sanitizer libraries (run by tests/test_quantise_api.py in child processes, as tests/test_sanitizers.py runs
tests/dry_run_cases.py): every refusal, random batches -- layouts, depths, sample types, DC bands -- and the frame layer with
a geometry change, so that AddressSanitizer, UndefinedBehaviorSanitizer and ThreadSanitizer see the job tables, the DC
records and the table rebuild.  Nothing is computed.

Not collected by a plain `pytest tests/` (the name): the product library has no dry mode."""
import ctypes as C
import os

import numpy as np
import pytest

import quant_cases as QC
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

if "dry" not in os.path.basename(os.environ.get("SCHRO_HIP_LIB", "")):
    pytest.skip("dry-run cases need SCHRO_HIP_LIB = a libschro_hip_dry_*.so", allow_module_level=True)


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def test_refusals(ctx):
    assert QC.refusal_cases(ctx) >= 10


def test_60_random_batches(ctx):
    rng = np.random.default_rng(2222)
    for rnd in range(60):
        dtype = (np.int16, np.int32)[int(rng.integers(0, 2))]
        b = np.dtype(dtype).itemsize
        jobs, keep = [], []
        for n in range(int(rng.integers(1, 5))):
            depth = int(rng.integers(1, 5))
            unit = 1 << depth
            w, h = unit * int(rng.integers(1, 40)), unit * int(rng.integers(1, 30))
            pitch = w + int(rng.integers(0, 4))
            hc = [int(rng.integers(1, 4)) for _ in range(depth + 1)]
            vc = [int(rng.integers(1, 4)) for _ in range(depth + 1)]
            recs = [r for r in QC.layout(w, h, depth, hc, vc, pitch * b, b)]
            intra = int(rng.integers(0, 2))
            ndc = hc[0] * vc[0]
            # (the public call refuses empty records: the layouts of bands narrower than their codeblock count are left out)
            if any(r[2] == 0 or r[3] == 0 for r in recs):
                continue
            for r in recs:
                r[4] = int(rng.integers(0, 61))
            co, qu = ctx.plane(h, pitch, dtype, stride=pitch * b), ctx.plane(h, pitch, dtype, stride=pitch * b)
            keep += [co, qu]
            jobs.append((co, qu, QC.table(recs), intra, (ndc, w >> depth, h >> depth) if intra else None))
        if jobs:
            keep += ctx.quantise_batch(jobs)
            ctx.synchronize()
        [p.free() for p in keep]


def test_frame_layer(ctx):
    lib = ctx.lib
    for (dtype, w, h, depth, hc, vc, intra) in ((np.int16, 64, 48, 2, [1, 2, 3], [1, 2, 2], 1), (np.int32, 64, 48, 2, [2, 1, 4], [1, 1, 3], 0),
                                                (np.int16, 16, 16, 3, [2, 2, 2, 2], [2, 2, 2, 2], 1),      # (empty codeblocks: a 1 x 1 chroma LL)
                                                (np.int16, 64, 48, 2, [1, 2, 3], [1, 2, 2], 0)):
        fmt = frames.frame_format(dtype, 1, 1)
        iwt, quant = frames.DeviceFrame(ctx, fmt, w, h), frames.DeviceFrame(ctx, fmt, w, h)
        params = frames.make_params(transform_depth=depth, num_refs=0 if intra else 1, iwt_luma_width=w, iwt_luma_height=h,
                                    iwt_chroma_width=w // 2, iwt_chroma_height=h // 2)
        for l in range(depth + 1):
            params.horiz_codeblocks[l], params.vert_codeblocks[l] = hc[l], vc[l]
        idx, summ = [], []
        for k in range(3):
            cw, ch = (w, h) if k == 0 else (w // 2, h // 2)
            n = len(QC.layout(cw, ch, depth, hc, vc, iwt.c.components[k].stride, np.dtype(dtype).itemsize))
            idx.append((C.c_int * n)(*[(3 * c + k) % 61 for c in range(n)]))
            summ.append((_lib.CodeblockSummary * n)())
        qi = (C.POINTER(C.c_int) * 3)(*[C.cast(a, C.POINTER(C.c_int)) for a in idx])
        sp = (C.POINTER(_lib.CodeblockSummary) * 3)(*[C.cast(a, C.POINTER(_lib.CodeblockSummary)) for a in summ])
        sa.check(lib.schro_hipframe_quantise(quant.ptr(), iwt.ptr(), C.byref(params), qi, sp))
        # refusals of the frame layer: a quant index out of range, frames of unlike depth, a host frame
        idx[1][0] = 61
        assert lib.schro_hipframe_quantise(quant.ptr(), iwt.ptr(), C.byref(params), qi, sp) == QC.EINVAL
        assert b"component 1, codeblock 0" in lib.schro_hip_last_error()
        idx[1][0] = 0
        other = frames.DeviceFrame(ctx, frames.frame_format(np.int32 if dtype == np.int16 else np.int16, 1, 1), w, h)
        assert lib.schro_hipframe_quantise(other.ptr(), iwt.ptr(), C.byref(params), qi, sp) == QC.EINVAL
        assert lib.schro_hipframe_quantise(quant.ptr(), None, C.byref(params), qi, sp) == QC.EINVAL
        if dtype == np.int16:
            sa.check(lib.schro_hipframe_subtract(iwt.ptr(), quant.ptr()))
            assert lib.schro_hipframe_subtract(iwt.ptr(), other.ptr()) == QC.EINVAL
        for f in (iwt, quant, other):
            f.unref()
