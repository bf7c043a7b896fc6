"""CPU: the motion-data encoder is declared, exported, bound and wrapped; schro_hip_motion_encode_check walks the refusal
table of tests/motion_enc_cases.py (SCHRO_HIP_EINVAL, the message naming the picture) and accepts the other side of every
limit; schro_hip_motion_encode_bound is the hand computation."""
import ctypes as C
import os
import re

import pytest

import motion_enc_cases as MC
import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
EINVAL = -1
KEYS = ("motion", "nbx", "nby", "num_refs", "hg", "out", "capacity", "result")


def test_header_declares_and_the_library_exports():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in ("schro_hip_motion_encode_bound", "schro_hip_motion_encode_batch", "schro_hip_motion_encode_check",
                 "schro_hip_encode_motion_data_noarith"):
        assert re.search(r"\b%s \(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name)
    assert "#define SCHRO_HIP_MOTION_SECTIONS %d" % _lib.MOTION_SECTIONS in text
    assert "SCHRO_HIP_SIZE (SchroHipMotionEncodeResult, %d);" % C.sizeof(_lib.MotionEncodeResult) in text
    assert "SCHRO_HIP_SIZE (SchroHipMotionEncodePicture, %d);" % C.sizeof(_lib.MotionEncodePicture) in text
    assert C.sizeof(_lib.MotionEncodeResult) == 4 * (2 + 9 + 9 + 3) and C.sizeof(_lib.MotionEncodePicture) == 8 + 16 + 8 + 8 + 8
    for member, offset in (("section_units", 44), ("first_unverified", 88)):
        assert getattr(_lib.MotionEncodeResult, member).offset == offset
        assert "SCHRO_HIP_LAYOUT (SchroHipMotionEncodeResult, %s, %d);" % (member, offset) in text
    for member, offset in (("num_refs", 16), ("out", 24), ("result", 40)):
        assert getattr(_lib.MotionEncodePicture, member).offset == offset
        assert "SCHRO_HIP_LAYOUT (SchroHipMotionEncodePicture, %s, %d);" % (member, offset) in text
    for name in ("motion_encode_batch", "encode_motion_data_noarith"):
        assert callable(getattr(sa.Context, name))
    assert callable(sa.motion_encode_check) and callable(sa.motion_encode_bound)


def check(d):
    pictures = [tuple(p[k] or None if k in ("motion", "out", "result") else p[k] for k in KEYS) for p in d]
    try:
        sa.motion_encode_check(pictures)
    except sa.SchroHipError as e:
        return e.code, _lib.load().schro_hip_last_error().decode()
    return 0, ""


@pytest.mark.parametrize("name,change,message", MC.REFUSALS, ids=[r[0] for r in MC.REFUSALS])
def test_refusals(name, change, message):
    d = MC.describe()
    assert check(d)[0] == 0
    change(d)
    rc, text = check(d)
    assert rc == EINVAL and message in text and text.startswith("motion_encode_batch:"), (rc, text)


@pytest.mark.parametrize("name,change", MC.ACCEPTED, ids=[r[0] for r in MC.ACCEPTED])
def test_the_other_side_of_the_limits_passes(name, change):
    d = MC.describe()
    change(d)
    rc, text = check(d)
    assert rc == 0, text


def test_the_bound_is_the_hand_computation():
    # 4 x 4 blocks, one reference, no global motion: 16 blocks of 102 + 1 bits and one superblock of 3: 1651 bits, 207
    # bytes; 7 sections of 9 bytes: 270
    assert sa.motion_encode_bound(4, 4, 1, 0) == 207 + 63 == 270
    # 240 x 136 blocks (a 2160p picture at 16-pixel separation), two references, global motion: 32640 blocks of 136 + 3 bits
    # and 2040 superblocks of 3: 4543080 bits, 567885 bytes; 9 sections of 9 bytes: 567966
    assert sa.motion_encode_bound(240, 136, 2, 1) == 567885 + 81 == 567966
    for args in ((4, 4, 1, 0), (240, 136, 2, 1), (12, 8, 2, 0), (20, 12, 1, 1)):
        assert sa.motion_encode_bound(*args) == MC.bound(*args)
    for args, message in (((6, 4, 1, 0), "6 x 4 blocks"), ((4, 4, 3, 0), "num_refs 3")):
        with pytest.raises(sa.SchroHipError, match=message) as e:
            sa.motion_encode_bound(*args)
        assert e.value.code == EINVAL


def test_empty_and_oversized_calls():
    lib = _lib.load()
    pic = sa.motion_encode_pictures([tuple(MC.describe()[0][k] for k in KEYS)])
    assert lib.schro_hip_motion_encode_check(None, 1) == EINVAL
    assert lib.schro_hip_motion_encode_check(pic, 0) == EINVAL
    assert lib.schro_hip_motion_encode_check(pic, 1) == 0
    assert lib.schro_hip_motion_encode_batch(None, pic, 1) == EINVAL
    assert lib.schro_hip_encode_motion_data_noarith(None, None, None, None, 0, None, None, None) == EINVAL
    many = sa.motion_encode_pictures([tuple(MC.describe()[0][k] for k in KEYS)] * 257)
    assert lib.schro_hip_motion_encode_check(many, 257) == EINVAL
