"""CPU: the motion-data decoder is declared, exported, bound and wrapped; schro_hip_motion_decode_check walks the refusal
table of tests/motion_dec_cases.py (SCHRO_HIP_EINVAL, the message naming the picture) and accepts the other side of every
limit, with addresses only; schro_hip_motion_decode_scratch_words is the hand count."""
import ctypes as C
import os
import re

import pytest

import motion_dec_cases as DC
import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
EINVAL = -1
KEYS = ("data", "data_bytes", "word", "nbx", "nby", "num_refs", "hg", "motion", "result")


def test_header_declares_and_the_library_exports():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in ("schro_hip_motion_decode_batch", "schro_hip_motion_decode_check", "schro_hip_motion_decode_scratch_words",
                 "schro_hip_decode_motion_data_noarith"):
        assert re.search(r"\b%s \(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name)
    assert C.sizeof(_lib.MotionDecodeResult) == 4 * (1 + 3 * 9 + 4 + 2) == DC.RESULT_BYTES
    assert C.sizeof(_lib.MotionDecodePicture) == 8 + 8 + 8 + 16 + 8 + 8
    assert "SCHRO_HIP_SIZE (SchroHipMotionDecodeResult, %d);" % C.sizeof(_lib.MotionDecodeResult) in text
    assert "SCHRO_HIP_SIZE (SchroHipMotionDecodePicture, %d);" % C.sizeof(_lib.MotionDecodePicture) in text
    for member, offset in (("section_bits", 76), ("truncated", 112), ("first_unverified", 132)):
        assert getattr(_lib.MotionDecodeResult, member).offset == offset
        assert "SCHRO_HIP_LAYOUT (SchroHipMotionDecodeResult, %s, %d);" % (member, offset) in text
    for member, offset in (("bytes_on_device", 16), ("num_refs", 32), ("motion", 40), ("result", 48)):
        assert getattr(_lib.MotionDecodePicture, member).offset == offset
        assert "SCHRO_HIP_LAYOUT (SchroHipMotionDecodePicture, %s, %d);" % (member, offset) in text
    for name in ("motion_decode_batch", "decode_motion_data_noarith"):
        assert callable(getattr(sa.Context, name))
    for name in ("motion_decode_pictures", "motion_decode_check", "motion_decode_scratch_words", "motion_decode_result"):
        assert callable(getattr(sa, name))


def test_the_result_dict_names_every_word():
    words = list(range(100, 134))
    r = sa.motion_decode_result(words)
    assert r["bytes"] == 100 and r["section_bytes"] == words[1:10] and r["section_units"] == words[10:19]
    assert r["section_bits"] == words[19:28]
    assert [r[k] for k in ("truncated", "overran", "not_consumed", "long_codes", "unverified", "first_unverified")] == words[28:]
    assert sa.motion_decode_result(words[:33] + [0xffffffff])["first_unverified"] == -1


def pictures_of(d):
    return [tuple(p[k] or None if k in ("data", "word", "motion", "result") else p[k] for k in KEYS) for p in d]


def check(d):
    try:
        sa.motion_decode_check(pictures_of(d))
    except sa.SchroHipError as e:
        return e.code, _lib.load().schro_hip_last_error().decode()
    return 0, ""


@pytest.mark.parametrize("name,change,message", DC.REFUSALS, ids=[r[0] for r in DC.REFUSALS])
def test_refusals(name, change, message):
    d = DC.describe()
    assert check(d)[0] == 0
    change(d)
    rc, text = check(d)
    assert rc == EINVAL and message in text and text.startswith("motion_decode_batch:"), (rc, text)
    with pytest.raises(sa.SchroHipError) as e:
        sa.motion_decode_scratch_words(pictures_of(d))
    assert e.value.code == EINVAL


@pytest.mark.parametrize("name,change", DC.ACCEPTED, ids=[r[0] for r in DC.ACCEPTED])
def test_the_other_side_of_the_limits_passes(name, change):
    d = DC.describe()
    change(d)
    rc, text = check(d)
    assert rc == 0, text
    assert sa.motion_decode_scratch_words(pictures_of(d)) == DC.scratch_words(d)


def test_the_scratch_is_the_hand_count():
    # 4 x 4 blocks and no bytes: 72 words of sections, 8 chunk slots of 4 words, 3 words of one superblock padded to 4, 160
    # words of 16 blocks
    d = DC.describe()
    d[0].update(nbx=4, nby=4, data_bytes=0)
    assert sa.motion_decode_scratch_words(pictures_of(d)) == 72 + 32 + 4 + 160 == 268
    # 240 x 136 blocks (a 2160p picture at 16-pixel separation) and 100001 bytes: 12501 + 8 slots, 2040 superblocks
    d[0].update(nbx=240, nby=136, data_bytes=100001)
    assert sa.motion_decode_scratch_words(pictures_of(d)) == 72 + 4 * 12509 + 6120 + 326400 == 382628
    # pictures add up
    DC._second(nbx=12, nby=4, data_bytes=17)(d)
    assert sa.motion_decode_scratch_words(pictures_of(d)) == 382628 + 72 + 4 * 11 + 10 + 480


def test_empty_and_oversized_calls():
    lib = _lib.load()
    pic = sa.motion_decode_pictures(pictures_of(DC.describe()))
    assert lib.schro_hip_motion_decode_check(None, 1) == EINVAL
    assert lib.schro_hip_motion_decode_check(pic, 0) == EINVAL
    assert lib.schro_hip_motion_decode_check(pic, 1) == 0
    assert lib.schro_hip_motion_decode_batch(None, pic, 1) == EINVAL
    assert lib.schro_hip_decode_motion_data_noarith(None, None, 0, None, None, None) == EINVAL
    many = sa.motion_decode_pictures(pictures_of(DC.describe()) * 257)
    assert lib.schro_hip_motion_decode_check(many, 257) == EINVAL
