"""GPU: schro_rough_me_heirarchical_scan_nohint_hip (the frame layer) and Context.rough_scan_nohint against
tests/analysis_ref.py's rough_scan_nohint, record for record: partial blocks, blocks wholly outside the picture, skipped
blocks of the coarser levels, both references; and the search finds the vector the reference picture was shifted by."""
import ctypes as C

import numpy as np
import pytest

import analysis_ref as A
import schroedinger_amd as sa
from schroedinger_amd import frames

pytestmark = pytest.mark.gpu

SHIFT_VECTOR = (3, -2)          # the reference picture is the frame moved by this many samples (dx, dy)

CASES = [  # (w, h, xbsep, x_num_blocks, y_num_blocks)
    (176, 144, 8, 24, 20),      # x_num_blocks * xbsep = 192 > 176: partial and empty blocks
    (176, 144, 12, 16, 12),
    (40, 24, 8, 8, 8),          # whole blocks outside the picture
]


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


_made = {}


def scene(w, h):
    """(frame, ref): ref (x, y) = frame (x - 3, y + 2) plus noise of +-2, so the best vector of an interior block is (3, -2)."""
    if (w, h) not in _made:
        rng = np.random.default_rng(w * 1000 + h)
        big = rng.integers(0, 256, (h + 16, w + 16), dtype=np.uint8)
        frame = big[8:8 + h, 8:8 + w]
        dx, dy = SHIFT_VECTOR
        ref = big[8 - dy:8 - dy + h, 8 - dx:8 - dx + w].astype(np.int32) + rng.integers(-2, 3, (h, w))
        _made[(w, h)] = (np.ascontiguousarray(frame), np.clip(ref, 0, 255).astype(np.uint8))
    return _made[(w, h)]


_wanted = {}


def differing(got, want):
    """The first few records that differ."""
    bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 20) != want.view(np.uint8).reshape(-1, 20)).any(axis=1))[:8]
    return [(int(n), got[n], want[n]) for n in bad]


def wanted(case, shift, distance, ref_index):
    key = (case, shift, distance, ref_index)
    if key not in _wanted:
        w, h, sep, nbx, nby = case
        frame, ref = scene(w, h)
        P = dict(x_num_blocks=nbx, y_num_blocks=nby, xbsep_luma=sep, ybsep_luma=sep)
        _wanted[key] = A.rough_scan_nohint(frame, ref, P, shift, distance, ref_index)
        _wanted[key].setflags(write=False)
    return _wanted[key]


@pytest.mark.parametrize("ref_index", [0, 1])
@pytest.mark.parametrize("shift,distance", [(0, 12), (0, 4), (2, 12), (2, 4), (4, 12), (4, 4)])
@pytest.mark.parametrize("case", CASES)
def test_context_rough_scan_nohint(ctx, case, shift, distance, ref_index):
    w, h, sep, nbx, nby = case
    frame, ref = scene(w, h)
    df, dr = ctx.upload(frame), ctx.upload(ref)
    P = dict(x_num_blocks=nbx, y_num_blocks=nby, xbsep_luma=sep, ybsep_luma=sep)
    got = ctx.rough_scan_nohint(df, dr, P, shift, distance, ref_index)
    want = wanted(case, shift, distance, ref_index)
    assert got.tobytes() == want.tobytes(), differing(got, want)
    if shift == 0:
        # interior blocks recover the vector the reference was shifted by
        grid = got.reshape(nby, nbx)
        dx, dy = SHIFT_VECTOR
        inner = grid[2:(h // sep) - 2, 2:(w // sep) - 2]
        if inner.size:
            assert (inner["v"][..., ref_index] == dx).all() and (inner["v"][..., 2 + ref_index] == dy).all()
            assert (inner["v"][..., 1 - ref_index] == 0).all() and (inner["metric"] < 3 * sep * sep).all()
    [p.free() for p in (df, dr)]


@pytest.mark.parametrize("ref_index", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_frame_layer_rough_scan_nohint(ctx, case, ref_index):
    w, h, sep, nbx, nby = case
    frame, ref = scene(w, h)

    def device_frame(luma, seed):
        comps = [luma, A.picture((w + 1) // 2, (h + 1) // 2, seed), A.picture((w + 1) // 2, (h + 1) // 2, seed + 1)]
        return frames.DeviceFrame(ctx, sa.FORMAT_U8_420, w, h).upload(frames.HostFrame(comps, 1, 1))

    fa, fb = device_frame(frame, 1), device_frame(ref, 3)
    P = frames.make_params(x_num_blocks=nbx, y_num_blocks=nby, xbsep_luma=sep, ybsep_luma=sep)
    for shift, distance in ((0, 12), (2, 4)):
        got = np.zeros(nbx * nby, sa.MV_DTYPE)
        got["metric"] = 12345       # (every record is set by the call)
        sa.check(ctx.lib.schro_rough_me_heirarchical_scan_nohint_hip(fa.ptr(), fb.ptr(), C.byref(P), shift, distance, ref_index,
                                                                     got.ctypes.data_as(C.c_void_p)))
        want = wanted(case, shift, distance, ref_index)
        assert got.tobytes() == want.tobytes(), differing(got, want)
    fa.unref(), fb.unref()


def test_an_apron_widens_the_windows_at_the_edges(ctx):
    """frame->extension is the reference frame's apron: with 32 samples of it the corner blocks search outside the picture."""
    w, h = 176, 144
    frame, ref = scene(w, h)
    ext = 32
    pf, pr = ctx.upload(A.edgeextend(frame, ext)), ctx.upload(A.edgeextend(ref, ext))
    P = dict(x_num_blocks=24, y_num_blocks=20, xbsep_luma=8, ybsep_luma=8)
    got = ctx.rough_scan_nohint(pf, pr, P, 0, 12, 0, extension=ext)
    want = A.rough_scan_nohint(frame, ref, P, 0, 12, 0, extension=ext)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != wanted(CASES[0], 0, 12, 0).tobytes()
    [p.free() for p in (pf, pr)]
