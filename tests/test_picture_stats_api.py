"""CPU: the picture statistics are declared, exported, bound and wrapped; the host-only schro_hip_plane_sums_check,
schro_hip_lowpass2_check and schro_hip_ssim_check refuse what the batch calls refuse (SCHRO_HIP_EINVAL, the message naming
the call and the entry) without a context or a device, and pass the good entry the refusals were made from;
schro_hip_lowpass2_coeff is the restatement's generate_coeff bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import picture_stats_cases as K
import picture_stats_ref as R
import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
EINVAL = -1
NAMES = ("schro_hip_picture_stats_geometry", "schro_hip_plane_sums_batch", "schro_hip_plane_sums_check", "schro_hip_lowpass2_coeff", "schro_hip_lowpass2_batch",
         "schro_hip_lowpass2_check", "schro_hip_ssim_scratch_bytes", "schro_hip_ssim_batch", "schro_hip_ssim_check",
         "schro_hipframe_calculate_average_luma", "schro_hipframe_mean_squared_error", "schro_hipframe_ssim",
         "schro_hipframe_filter_lowpass2", "schro_engine_get_scene_change_score_hip")


def test_header_declares_and_the_library_exports():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s \(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name)
    for name in ("plane_sums_batch", "lowpass2_batch", "ssim_batch", "average_luma", "mean_squared_error", "ssim", "filter_lowpass2",
                 "scene_change_score"):
        assert callable(getattr(sa.Context, name)), name
    assert callable(sa.lowpass2_coeff)
    # the structs on LP64, member for member
    assert C.sizeof(_lib.SumsJob) == 56 and _lib.SumsJob.b.offset == 24 and _lib.SumsJob.result.offset == 48
    assert C.sizeof(_lib.Lowpass2Plane) == 96 and _lib.Lowpass2Plane.h_coeff.offset == 24 and _lib.Lowpass2Plane.out_of_range.offset == 88
    assert C.sizeof(_lib.SsimResult) == 32 == sa.SSIM_RESULT_DTYPE.itemsize
    assert C.sizeof(_lib.SsimPicture) == 88 and _lib.SsimPicture.scratch.offset == 48 and _lib.SsimPicture.map_stride.offset == 80


def test_struct_layouts_match_the_header(tmp_path):
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "schro_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(SchroHipSumsJob), offsetof(SchroHipSumsJob, result),
         sizeof(SchroHipLowpass2Plane), offsetof(SchroHipLowpass2Plane, out_of_range), sizeof(SchroHipSsimResult),
         sizeof(SchroHipSsimPicture), offsetof(SchroHipSsimPicture, result), offsetof(SchroHipSsimPicture, map_stride));
  return 0;
}''')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(_lib.SumsJob), _lib.SumsJob.result.offset, C.sizeof(_lib.Lowpass2Plane), _lib.Lowpass2Plane.out_of_range.offset,
                   C.sizeof(_lib.SsimResult), C.sizeof(_lib.SsimPicture), _lib.SsimPicture.result.offset, _lib.SsimPicture.map_stride.offset]


def test_the_tile_lengths_come_from_the_library():
    g = sa.picture_stats_geometry()
    assert tuple(g) == sa.PICTURE_STATS_GEOMETRY and all(v > 0 for v in g.values())
    assert g["lowpass_rows"] % 64 == 0 and g["lowpass_cols"] % 64 == 0          # a lane a row, then a column: whole waves
    assert (K.LOWPASS_ROWS, K.LOWPASS_CHUNK, K.SSIM_TILE_COLS) == (g["lowpass_rows"], g["lowpass_chunk"], g["ssim_tile_cols"])


@pytest.mark.parametrize("sigma", K.SIGMAS + (0.1, 2.4999, 2.5, 100.0))
def test_lowpass2_coeff_is_generate_coeff(sigma):
    assert sa.lowpass2_coeff(sigma) == R.generate_coeff(sigma)


# ---- refusals: no pointer below is ever dereferenced (the checks are host only) ----

BASE = 0x10000


def sums_job(**kw):
    j = _lib.SumsJob(a=BASE, a_stride=64, bytes_per_sample=1, width=48, height=8, b=BASE + 0x1000, b_stride=64, b_width=48, b_height=8,
                     result=BASE + 0x2000)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def lowpass_plane(**kw):
    p = _lib.Lowpass2Plane(data=BASE, stride=128, bytes_per_sample=2, width=48, height=8, out_of_range=BASE + 0x2000)
    p.h_coeff[:] = R.generate_coeff(1.5)
    p.v_coeff[:] = R.generate_coeff(0.75)
    for k, v in kw.items():
        if k in ("h_coeff", "v_coeff"):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def ssim_picture(**kw):
    p = _lib.SsimPicture(a=BASE, a_stride=64, width=48, height=8, b=BASE + 0x1000, b_stride=64, b_width=48, b_height=8,
                         scratch=BASE + 0x10000, scratch_bytes=sa.ssim_scratch_bytes(48, 8), result=BASE + 0x2000,
                         map=BASE + 0x4000, map_stride=48 * 8)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def run(check, entry, n=1):
    lib = _lib.load()
    rc = check(C.byref(entry) if entry is not None else None, n)
    return rc, lib.schro_hip_last_error().decode()


SUMS_REFUSALS = [
    ("width 0", dict(width=0, b_width=0), "is not positive"),
    ("height -1", dict(height=-1, b_height=-1), "is not positive"),
    ("too wide", dict(width=65537, b_width=65537, a_stride=1 << 17, b_stride=1 << 17), "is too large"),
    ("a stride", dict(a_stride=47), "of a shorter than a row"),
    ("s16 stride", dict(bytes_per_sample=2, b=None, a_stride=94), "of a shorter than a row"),
    ("b stride", dict(b_stride=47), "of b shorter than a row"),
    ("a NULL", dict(a=None), "NULL pointer"),
    ("result NULL", dict(result=None), "NULL pointer"),
    ("result misaligned", dict(result=BASE + 0x2004), "not 8-byte aligned"),
    ("sample size 4", dict(bytes_per_sample=4), "neither 1 nor 2"),
    ("sample size 0", dict(bytes_per_sample=0), "neither 1 nor 2"),
    ("b narrower", dict(b_width=47), "a is 48x8, b is 47x8"),
    ("b taller", dict(b_height=9), "a is 48x8, b is 48x9"),
    ("s16 against b", dict(bytes_per_sample=2, a_stride=128), "two u8 planes"),
    ("s16 at an odd address", dict(bytes_per_sample=2, a_stride=128, b=None, a=BASE + 1), "odd address or stride"),
]
LOWPASS_REFUSALS = [
    ("width 0", dict(width=0), "is not positive"),
    ("height 0", dict(height=0), "is not positive"),
    ("too tall", dict(height=65537), "is too large"),
    ("stride", dict(stride=94), "shorter than a row"),
    ("data NULL", dict(data=None), "NULL pointer"),
    ("counter NULL", dict(out_of_range=None), "NULL pointer"),
    ("counter misaligned", dict(out_of_range=BASE + 0x2002), "not 4-byte aligned"),
    ("sample size 4", dict(bytes_per_sample=4), "neither 1 nor 2"),
    ("odd stride", dict(stride=129), "odd address or stride"),
    ("h nan", dict(h_coeff=(2, float("nan"))), "not finite"),
    ("v inf", dict(v_coeff=(0, float("inf"))), "not finite"),
    ("v -inf", dict(v_coeff=(3, float("-inf"))), "not finite"),
]
SSIM_REFUSALS = [
    ("width 0", dict(width=0, b_width=0), "is not positive"),
    ("height 0", dict(height=0, b_height=0), "is not positive"),
    ("too wide", dict(width=16385, b_width=16385), "is too large"),
    ("a stride", dict(a_stride=47), "stride shorter than a row"),
    ("b stride", dict(b_stride=40), "stride shorter than a row"),
    ("a NULL", dict(a=None), "NULL pointer"),
    ("b NULL", dict(b=None), "NULL pointer"),
    ("scratch NULL", dict(scratch=None), "NULL pointer"),
    ("result NULL", dict(result=None), "NULL pointer"),
    ("result misaligned", dict(result=BASE + 0x2004), "result is not 8-byte aligned"),
    ("scratch misaligned", dict(scratch=BASE + 0x10008), "scratch is not 16-byte aligned"),
    ("scratch short", dict(scratch_bytes=sa.ssim_scratch_bytes(48, 8) - 1), "bytes of scratch"),
    ("b smaller", dict(b_width=47), "a is 48x8, b is 47x8"),
    ("map misaligned", dict(map=BASE + 0x4004), "map is not 8-byte aligned"),
    ("map stride", dict(map_stride=47 * 8), "of the map shorter than a row"),
]


def walk(check, make, prefix, change, message):
    assert run(check, make()) == (0, run(check, make())[1])
    rc, text = run(check, make(**change))
    assert rc == EINVAL and message in text and text.startswith(prefix), (rc, text)


@pytest.mark.parametrize("name,change,message", SUMS_REFUSALS, ids=[r[0] for r in SUMS_REFUSALS])
def test_plane_sums_refusals(name, change, message):
    walk(_lib.load().schro_hip_plane_sums_check, sums_job, "plane_sums_batch:", change, message)


@pytest.mark.parametrize("name,change,message", LOWPASS_REFUSALS, ids=[r[0] for r in LOWPASS_REFUSALS])
def test_lowpass2_refusals(name, change, message):
    walk(_lib.load().schro_hip_lowpass2_check, lowpass_plane, "lowpass2_batch:", change, message)


@pytest.mark.parametrize("name,change,message", SSIM_REFUSALS, ids=[r[0] for r in SSIM_REFUSALS])
def test_ssim_refusals(name, change, message):
    walk(_lib.load().schro_hip_ssim_check, ssim_picture, "ssim_batch:", change, message)


def test_whole_call_refusals_and_the_batch_calls_refuse_alike():
    lib = _lib.load()
    for check, batch, make, T in ((lib.schro_hip_plane_sums_check, lib.schro_hip_plane_sums_batch, sums_job, _lib.SumsJob),
                                  (lib.schro_hip_lowpass2_check, lib.schro_hip_lowpass2_batch, lowpass_plane, _lib.Lowpass2Plane),
                                  (lib.schro_hip_ssim_check, lib.schro_hip_ssim_batch, ssim_picture, _lib.SsimPicture)):
        assert run(check, None)[0] == EINVAL
        assert run(check, make(), 0)[0] == EINVAL
        assert check((T * 300)(), 300) == EINVAL
        # no context: refused before anything else, nothing launched
        assert batch(None, C.byref(make()), 1) == EINVAL
    # two entries that share what each must own
    two = (_lib.SumsJob * 2)(sums_job(), sums_job(a=BASE + 0x8000))
    assert lib.schro_hip_plane_sums_check(two, 2) == EINVAL and "share a result" in lib.schro_hip_last_error().decode()
    two = (_lib.Lowpass2Plane * 2)(lowpass_plane(), lowpass_plane(data=BASE + 64))
    assert lib.schro_hip_lowpass2_check(two, 2) == EINVAL and "overlap" in lib.schro_hip_last_error().decode()
    two = (_lib.Lowpass2Plane * 2)(lowpass_plane(), lowpass_plane(data=BASE + 0x8000))
    assert lib.schro_hip_lowpass2_check(two, 2) == 0         # (one counter for both is fine)
    assert sa.ssim_scratch_bytes(0, 8) == 0 and sa.ssim_scratch_bytes(48, 16385) == 0
    # rows of a_lowpass, b_lowpass (64-byte pitch), ab, a^2, b^2 (128-byte pitch), one tile's partial sum
    assert sa.ssim_scratch_bytes(48, 8) == 8 * (2 * 64 + 3 * 128) + 64


def test_the_python_wrappers_raise_the_refusals():
    class P:
        def __init__(self, ptr, stride, width, height, dtype):
            self.ptr, self.stride, self.width, self.height, self.dtype = ptr, stride, width, height, np.dtype(dtype)
    a, b, r = P(BASE, 64, 48, 8, np.uint8), P(BASE + 0x1000, 64, 48, 8, np.uint8), P(BASE + 0x2000, 16, 2, 1, np.int64)
    sa.plane_sums_check([(a, b, r), (a, None, P(BASE + 0x3000, 16, 2, 1, np.int64))])
    with pytest.raises(sa.SchroHipError, match="a is 48x8, b is 40x8"):
        sa.plane_sums_check([(a, P(BASE + 0x1000, 64, 40, 8, np.uint8), r)])
    s = P(BASE, 128, 48, 8, np.int16)
    sa.lowpass2_check([(s, 1.5, R.generate_coeff(5), P(BASE + 0x2000, 4, 1, 1, np.uint32))])
    with pytest.raises(sa.SchroHipError, match="not finite"):
        sa.lowpass2_check([(s, 1.5, [1.0, float("nan"), 0, 0], P(BASE + 0x2000, 4, 1, 1, np.uint32))])
    scratch = P(BASE + 0x10000, 0, sa.ssim_scratch_bytes(48, 8), 1, np.uint8)
    sa.ssim_check([(a, b, None, scratch, r)])
    with pytest.raises(sa.SchroHipError, match="bytes of scratch"):
        sa.ssim_check([(a, b, None, P(BASE + 0x10000, 0, 100, 1, np.uint8), r)])


def test_overlaps_are_judged_by_rectangles():
    lib = _lib.load()

    def lowpass(*planes):
        arr = (_lib.Lowpass2Plane * len(planes))(*planes)
        return lib.schro_hip_lowpass2_check(arr, len(planes)), lib.schro_hip_last_error().decode()
    # two windows of one buffer side by side: rows of 256 bytes, s16 columns 0 .. 47 and 48 .. 95 (then 47 .. 94: one shared)
    left = lowpass_plane(stride=256)
    assert lowpass(left, lowpass_plane(stride=256, data=BASE + 96))[0] == 0
    assert lowpass(lowpass_plane(stride=256, data=BASE + 96), left)[0] == 0
    rc, text = lowpass(left, lowpass_plane(stride=256, data=BASE + 94))
    assert rc == EINVAL and "planes 0 and 1 overlap" in text
    # a window that wraps into the next row's first columns, and windows of unlike strides whose extents meet
    assert lowpass(left, lowpass_plane(stride=256, data=BASE + 200))[0] == EINVAL
    assert lowpass(left, lowpass_plane(stride=512, data=BASE + 96))[0] == EINVAL
    # the same plane one row down
    assert lowpass(left, lowpass_plane(stride=256, data=BASE + 256))[0] == EINVAL

    def ssim(*pics):
        arr = (_lib.SsimPicture * len(pics))(*pics)
        return lib.schro_hip_ssim_check(arr, len(pics)), lib.schro_hip_last_error().decode()
    assert ssim(ssim_picture())[0] == 0
    assert ssim(ssim_picture(b=BASE))[0] == 0                   # a against itself
    rc, text = ssim(ssim_picture(result=BASE + 0x10040))
    assert rc == EINVAL and "scratch of picture 0 overlaps a result of picture 0" in text
    rc, text = ssim(ssim_picture(map=BASE + 0x10100))
    assert rc == EINVAL and "scratch of picture 0 overlaps a map of picture 0" in text
    rc, text = ssim(ssim_picture(map=BASE + 0x1000))
    assert rc == EINVAL and "a map of picture 0 overlaps plane b of picture 0" in text
    other = dict(a=BASE + 0x40000, b=BASE + 0x41000, result=BASE + 0x42000, map=BASE + 0x44000, scratch=BASE + 0x50000)
    assert ssim(ssim_picture(), ssim_picture(**other))[0] == 0
    assert ssim(ssim_picture(), ssim_picture(**dict(other, a=BASE, b=BASE + 0x1000)))[0] == 0          # shared inputs
    rc, text = ssim(ssim_picture(), ssim_picture(**dict(other, map=BASE + 0x10000)))
    assert rc == EINVAL and "a map of picture 1 overlaps scratch of picture 0" in text
    rc, text = ssim(ssim_picture(), ssim_picture(**dict(other, a=BASE + 0x2000)))
    assert rc == EINVAL and "a result of picture 0 overlaps plane a of picture 1" in text
    rc, text = ssim(ssim_picture(), ssim_picture(**dict(other, scratch=BASE + 0x10040)))
    assert rc == EINVAL and "pictures 0 and 1 share scratch" in text
