"""CPU: the arithmetic motion-data decoder is declared, exported, bound and wrapped; schro_hip_motion_arith_decode_check
walks the refusal table of tests/motion_arith_dec_cases.py -- the VLC call's, in the same words -- and accepts the other
side of every limit, with addresses only; schro_hip_motion_arith_decode_scratch_words is the hand count."""
import ctypes as C
import os
import re

import pytest

import motion_arith_dec_cases as AC
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
    for name in ("schro_hip_motion_arith_decode_batch", "schro_hip_motion_arith_decode_check", "schro_hip_motion_arith_decode_scratch_words",
                 "schro_hip_decode_motion_data_arith"):
        assert re.search(r"\b%s \(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name)
    assert C.sizeof(_lib.MotionArithDecodeResult) == 4 * (1 + 4 * 9 + 4 + 2) == AC.RESULT_BYTES
    assert C.sizeof(_lib.MotionArithDecodePicture) == C.sizeof(_lib.MotionDecodePicture) == 56
    assert "SCHRO_HIP_SIZE (SchroHipMotionArithDecodeResult, %d);" % C.sizeof(_lib.MotionArithDecodeResult) in text
    assert "SCHRO_HIP_SIZE (SchroHipMotionArithDecodePicture, %d);" % C.sizeof(_lib.MotionArithDecodePicture) in text
    for member, offset in (("section_offset", 76), ("section_bins", 112), ("truncated", 148), ("first_unverified", 168)):
        assert getattr(_lib.MotionArithDecodeResult, member).offset == offset
        assert "SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodeResult, %s, %d);" % (member, offset) in text
    for member, offset in (("bytes_on_device", 16), ("num_refs", 32), ("motion", 40), ("result", 48)):
        assert getattr(_lib.MotionArithDecodePicture, member).offset == offset
        assert "SCHRO_HIP_LAYOUT (SchroHipMotionArithDecodePicture, %s, %d);" % (member, offset) in text
    for name in ("motion_arith_decode_batch", "decode_motion_data_arith"):
        assert callable(getattr(sa.Context, name))
    for name in ("motion_arith_decode_pictures", "motion_arith_decode_check", "motion_arith_decode_scratch_words", "motion_arith_decode_result"):
        assert callable(getattr(sa, name))


def test_the_result_dict_names_every_word():
    words = list(range(100, 143))
    r = sa.motion_arith_decode_result(words)
    assert r["bytes"] == 100 and r["section_bytes"] == words[1:10] and r["section_units"] == words[10:19]
    assert r["section_offset"] == words[19:28] and r["section_bins"] == words[28:37]
    assert [r[k] for k in ("truncated", "overran", "not_consumed", "long_codes", "unverified", "first_unverified")] == words[37:]
    assert sa.motion_arith_decode_result(words[:42] + [0xffffffff])["first_unverified"] == -1
    assert len(r) == 11


def pictures_of(d):
    return [tuple(p[k] or None if k in ("data", "word", "motion", "result") else p[k] for k in KEYS) for p in d]


def check(d):
    try:
        sa.motion_arith_decode_check(pictures_of(d))
    except sa.SchroHipError as e:
        return e.code, _lib.load().schro_hip_last_error().decode()
    return 0, ""


@pytest.mark.parametrize("name,change,message", AC.REFUSALS, ids=[r[0] for r in AC.REFUSALS])
def test_refusals(name, change, message):
    d = AC.describe_picture()
    assert check(d)[0] == 0
    change(d)
    rc, text = check(d)
    assert rc == EINVAL and message in text and text.startswith("motion_arith_decode_batch:"), (rc, text)
    with pytest.raises(sa.SchroHipError) as e:
        sa.motion_arith_decode_scratch_words(pictures_of(d))
    assert e.value.code == EINVAL


@pytest.mark.parametrize("name,change,message", [r for r in DC.REFUSALS if r in AC.REFUSALS], ids=[r[0] for r in DC.REFUSALS if r in AC.REFUSALS])
def test_refusals_in_the_vlc_calls_words(name, change, message):
    """Behind the call's name the message is the VLC call's, letter for letter."""
    texts = []
    for checker in (sa.motion_decode_check, sa.motion_arith_decode_check):
        d = DC.describe()
        change(d)
        with pytest.raises(sa.SchroHipError):
            checker(pictures_of(d))
        texts.append(_lib.load().schro_hip_last_error().decode().split(":", 1)[1])
    assert texts[0] == texts[1]


@pytest.mark.parametrize("name,change", AC.ACCEPTED, ids=[r[0] for r in AC.ACCEPTED])
def test_the_other_side_of_the_limits_passes(name, change):
    d = AC.describe_picture()
    change(d)
    rc, text = check(d)
    assert rc == 0, text
    assert sa.motion_arith_decode_scratch_words(pictures_of(d)) == AC.scratch_words(d)


def test_the_scratch_is_the_hand_count():
    # 4 x 4 blocks: 36 words of sections, 3 words of one superblock padded to 4, 11 words for each of 16 blocks; the bytes
    # take no scratch
    d = AC.describe_picture()
    d[0].update(nbx=4, nby=4, data_bytes=0)
    assert sa.motion_arith_decode_scratch_words(pictures_of(d)) == 36 + 4 + 176 == 216
    d[0].update(data_bytes=100001)
    assert sa.motion_arith_decode_scratch_words(pictures_of(d)) == 216
    # 240 x 136 blocks (a 2160p picture at 16-pixel separation): 2040 superblocks, 32640 blocks
    d[0].update(nbx=240, nby=136)
    assert sa.motion_arith_decode_scratch_words(pictures_of(d)) == 36 + 6120 + 359040 == 365196
    # pictures add up
    DC._second(nbx=12, nby=4, data_bytes=17)(d)
    assert sa.motion_arith_decode_scratch_words(pictures_of(d)) == 365196 + 36 + 10 + 528


def test_empty_and_oversized_calls():
    lib = _lib.load()
    pic = sa.motion_arith_decode_pictures(pictures_of(AC.describe_picture()))
    assert lib.schro_hip_motion_arith_decode_check(None, 1) == EINVAL
    assert lib.schro_hip_motion_arith_decode_check(pic, 0) == EINVAL
    assert lib.schro_hip_motion_arith_decode_check(pic, 1) == 0
    assert lib.schro_hip_motion_arith_decode_batch(None, pic, 1) == EINVAL
    assert lib.schro_hip_decode_motion_data_arith(None, None, 0, None, None, None) == EINVAL
    many = sa.motion_arith_decode_pictures(pictures_of(AC.describe_picture()) * 257)
    assert lib.schro_hip_motion_arith_decode_check(many, 257) == EINVAL
