"""CPU: upsample / edge-extend / convert oracle.  Checks the oracle's literal restatement
of schroframe.c against the closed-form half-pel plane spec, the
"aprons == coordinate clamp" equivalence the GPU path relies on, and the convert
arithmetic against the reference's compiled kernels."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import synth

TAPS = np.array([-1, 3, -7, 21, 21, -7, 3, -1])


def filt8(src, axis):
    n = src.shape[axis]
    idx = np.clip(np.arange(n)[:, None] + np.arange(8)[None, :] - 3, 0, n - 1)
    s = src.astype(np.int64)
    if axis == 0:
        acc = (s[idx, :] * TAPS[None, :, None]).sum(1)
    else:
        acc = (s[:, idx] * TAPS[None, None, :]).sum(2)
    return np.clip((acc + 16) >> 5, 0, 255).astype(np.uint8)


def planes_spec(p0):
    h, w = p0.shape
    p2 = filt8(p0, 0)
    p2[h - 1] = p0[h - 1]
    p1 = filt8(p0, 1)
    p1[:, w - 1] = p0[:, w - 1]
    p3 = filt8(p2, 1)
    p3[:, w - 1] = p2[:, w - 1]
    p3[h - 1] = p1[h - 1]
    return [p0, p1, p2, p3]


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (7, 9), (8, 8), (9, 8), (20, 20), (24, 40), (64, 96)])
def test_planes_and_aprons(h, w):
    pic = synth.picture_u8(h, w, seed=h * 13 + w, blur=False)
    up = O.UpComp(pic)
    spec = planes_spec(pic)
    for i in range(4):
        assert np.array_equal(up.plane(i), spec[i]), i
    # every apron sample equals the in-picture sample at the clamped half-pel coordinate
    for i in range(4):
        for y in list(range(-32, 3)) + list(range(h - 3, h + 32)):
            for x in list(range(-32, 3)) + list(range(w - 3, w + 32)):
                X = min(max(2 * x + (i & 1), 0), 2 * w - 2)
                Y = min(max(2 * y + (i >> 1), 0), 2 * h - 2)
                want = spec[((Y & 1) << 1) | (X & 1)][Y >> 1, X >> 1]
                assert up.get(i, x, y) == want, (i, x, y)


def test_convert_matches_reference_kernels():
    s16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)

    def ref_s16():
        d = np.zeros(65536, np.uint8)
        O.reforc().orc_offsetconvert_u8_s16(d.ctypes.data_as(C.c_void_p), s16.ctypes.data_as(C.c_void_p), C.c_int(65536))
        return d
    O.assert_reference("offsetconvert_u8_s16", O.convert_u8(s16.reshape(256, 256), 256, 256).ravel(), ref_s16)
    # s32: the shipped C fallback (schroorc-dist.c:4296-4303, convsuslw) and the Orc source the
    # JIT path runs (schroorc.orc:513-521, convssslw) disagree for sample + 128 > 32767 (fallback
    # -> 0, Orc -> 255); both agree everywhere below, which covers every legal sample.  The oracle
    # and the GPU follow the Orc source.
    s32 = np.concatenate([np.arange(-70000, 32640, 7), [-2**31, -40000, 32639, 0, -129]]).astype(np.int32)
    s32 = np.resize(s32, (100, 200)).copy()

    def ref_s32():
        d = np.zeros(s32.size, np.uint8)
        O.reforc().orc_offsetconvert_u8_s32(d.ctypes.data_as(C.c_void_p), s32.ctypes.data_as(C.c_void_p), C.c_int(s32.size))
        return d
    O.assert_reference("offsetconvert_u8_s32", O.convert_u8(s32, 200, 100).ravel(), ref_s32)
    big = np.array([[32640, 40000, 70000, 2**31 - 1]], np.int32)
    assert O.convert_u8(big, 4, 1).tolist() == [[255, 255, 255, 0]]     # addl wraps first


def test_convert_crop():
    src = synth.full_range(48, 64, np.int16, seed=2)
    out = O.convert_u8(src, 61, 45)
    assert out.shape == (45, 61)
    want = np.clip((src[:45, :61].astype(np.int32) + 128 + 32768) % 65536 - 32768, 0, 255)
    assert np.array_equal(out, want.astype(np.uint8))
