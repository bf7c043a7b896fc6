"""CPU: the noarith transform-data decoder is declared, exported, bound and wrapped; schro_hip_noarith_decode_check walks
the refusal table of tests/noarith_dec_cases.py (SCHRO_HIP_EINVAL, the message naming picture and component) and accepts
the other side of every limit; every case's geometry passes; the scratch the call takes follows the stated formula."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noarith_dec_cases as DC
import noarith_enc_ref as enc
import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
EINVAL = -1


def test_header_declares_and_the_library_exports():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in ("schro_hip_noarith_decode_batch", "schro_hip_noarith_decode_check", "schro_hip_noarith_decode_scratch_words",
                 "schro_hipframe_decode_transform_data_noarith"):
        assert re.search(r"\b%s \(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name)
    # the structs: member for member (sizes on LP64)
    assert C.sizeof(_lib.NoarithDecodeResult) == 4 * 9 + 4 * 3 * 19 + 3 * 19 + 3
    assert C.sizeof(_lib.NoarithDecodePicture) == 8 + 8 + 8 + 24 + 24 + 12 + 4 + 24 + 12 + 12 + 4 + 28 + 28 + 4 + 4 + 4 + 8
    for member in ("data", "data_bytes", "bytes_on_device", "coeffs", "bytes", "stride", "quant", "iwt_width", "iwt_height",
                   "transform_depth", "horiz_codeblocks", "vert_codeblocks", "codeblock_mode_index", "is_intra",
                   "compat_quant_offset", "result"):
        assert hasattr(_lib.NoarithDecodePicture, member) and re.search(r"\b%s\b" % member, text), member
    for name in ("noarith_decode_batch", "decode_transform_data_noarith"):
        assert callable(getattr(sa.Context, name))
    assert callable(sa.noarith_decode_check) and callable(sa.noarith_decode_result) and callable(sa.noarith_decode_pictures)


def check(d):
    lib = _lib.load()
    pic = DC.c_picture(d, _lib)
    rc = lib.schro_hip_noarith_decode_check(C.byref(pic), 1, d["bpp"])
    return rc, lib.schro_hip_last_error().decode()


@pytest.mark.parametrize("name,change,message", DC.REFUSALS, ids=[r[0] for r in DC.REFUSALS])
def test_refusals(name, change, message):
    d = DC.describe()
    assert check(d)[0] == 0
    change(d)
    rc, text = check(d)
    assert rc == EINVAL and message in text and text.startswith("noarith_decode_batch:"), (rc, text)


@pytest.mark.parametrize("name,change", DC.ACCEPTED, ids=[r[0] for r in DC.ACCEPTED])
def test_the_other_side_of_the_limits_passes(name, change):
    for bpp in (2, 4):
        d = DC.describe(bpp=bpp)
        change(d)
        rc, text = check(d)
        assert rc == 0, text


def test_empty_and_oversized_calls():
    lib = _lib.load()
    pic = DC.c_picture(DC.describe(), _lib)
    assert lib.schro_hip_noarith_decode_check(None, 1, 2) == EINVAL
    assert lib.schro_hip_noarith_decode_check(C.byref(pic), 0, 2) == EINVAL
    assert lib.schro_hip_noarith_decode_batch(None, C.byref(pic), 1, 2) == EINVAL
    assert lib.schro_hip_noarith_decode_scratch_words(None, 1, 2) == EINVAL
    assert lib.schro_hipframe_decode_transform_data_noarith(None, None, 0, None, None, None) == EINVAL
    assert b"hipframe_decode_transform_data_noarith" in lib.schro_hip_last_error()
    many = (_lib.NoarithDecodePicture * 257)(*([pic] * 257))
    assert lib.schro_hip_noarith_decode_check(many, 257, 2) == EINVAL


class FakePlane:
    def __init__(self, ptr, w, h, b):
        self.ptr, self.width, self.height, self.stride = ptr, w, h, (w * b + 63) // 64 * 64


def fake_picture(case, n=0):
    b = case.dtype.itemsize
    coeffs = [FakePlane((1 + 2 * k + 16 * n) << 24, w, h, b) for k, (w, h) in enumerate(case.sizes)]
    quant = [FakePlane((2 + 2 * k + 16 * n) << 24, w, h, b) for k, (w, h) in enumerate(case.sizes)]
    return ((9 + 16 * n) << 24, case.data_bytes, None, coeffs, quant, case.depth, case.hc, case.vc, case.mode, case.is_intra,
            case.compat, (10 + 16 * n) << 24)


def test_wrappers_fill_the_structure():
    case = DC.BY_NAME["s32-compat-fires-c1"]
    arr = sa.noarith_decode_pictures([fake_picture(case), fake_picture(case, 1)])
    a = arr[1]
    assert (a.data, a.data_bytes, a.bytes_on_device, a.result) == (25 << 24, len(case.data), None, 26 << 24)
    assert [a.coeffs[k] for k in range(3)] == [(17 + 2 * k) << 24 for k in range(3)]
    assert [a.quant[k] for k in range(3)] == [(18 + 2 * k) << 24 for k in range(3)]
    assert [(a.iwt_width[k], a.iwt_height[k]) for k in range(3)] == case.sizes
    assert [a.stride[k] for k in range(3)] == [(w * 4 + 63) // 64 * 64 for w, h in case.sizes]
    assert list(a.horiz_codeblocks)[:case.depth + 1] == case.hc[:case.depth + 1] and list(a.vert_codeblocks)[:case.depth + 1] == case.vc[:case.depth + 1]
    assert (a.transform_depth, a.codeblock_mode_index, a.is_intra, a.compat_quant_offset) == (case.depth, case.mode, 0, 0)
    sa.noarith_decode_check([fake_picture(case), fake_picture(case, 1)], 4)
    with pytest.raises(sa.SchroHipError, match="bytes_per_sample must be 2 or 4"):
        sa.noarith_decode_check([fake_picture(case)], 3)
    pic = list(fake_picture(case))
    pic[4] = None
    assert all(sa.noarith_decode_pictures([tuple(pic)])[0].quant[k] is None for k in range(3))


def test_pictures_of_one_call_may_not_write_into_each_other():
    """What one picture writes (planes, result) may not overlap what another reads or writes; shared input is fine."""
    lib = _lib.load()
    case = DC.BY_NAME["s16-all-two-m1-c0"]

    def check2(change):
        pics = [list(fake_picture(case)), list(fake_picture(case, 1))]
        change(pics)
        arr = sa.noarith_decode_pictures([tuple(p) for p in pics])
        return lib.schro_hip_noarith_decode_check(arr, 2, 2), lib.schro_hip_last_error().decode()

    assert check2(lambda p: None)[0] == 0
    assert check2(lambda p: p[1].__setitem__(0, p[0][0]))[0] == 0               # the same data twice
    rc, text = check2(lambda p: p[1].__setitem__(11, p[0][0] + 8))              # a result inside the other's data
    assert rc == EINVAL and "picture 1: its result overlaps the data of picture 0" in text, text
    rc, text = check2(lambda p: p[1].__setitem__(3, p[0][3]))                   # the same coefficient planes
    assert rc == EINVAL and "picture 1: its coeffs overlaps the coeffs of picture 0" in text, text
    rc, text = check2(lambda p: p[0].__setitem__(11, p[1][11]))                 # one result for both
    assert rc == EINVAL and "picture 1: its result overlaps the result of picture 0" in text, text
    rc, text = check2(lambda p: p[0].__setitem__(2, p[1][4][2].ptr + 4))        # a length word inside the other's quant plane
    assert rc == EINVAL and "picture 1: its quant overlaps the bytes_on_device of picture 0" in text, text


def test_result_words_unpack():
    r = _lib.NoarithDecodeResult()
    r.bytes_read, r.error, r.first_error, r.compat_quant_offset, r.truncated = 1000, 1, 44, 1, 2
    r.not_consumed, r.overran, r.long_codes, r.clamped_quant = 3, 4, 5, 6
    r.subband_length[2][18], r.subband_length[0][1] = 77, 1 << 31
    r.subband_quant_index[0][0], r.subband_quant_index[2][18], r.subband_quant_index[1][3] = 60, 9, 200
    for form in (r, np.frombuffer(bytes(r), np.uint32)):
        d = sa.noarith_decode_result(form)
        assert [d[k] for k in ("bytes_read", "error", "first_error", "compat_quant_offset", "truncated", "not_consumed", "overran",
                               "long_codes", "clamped_quant")] == [1000, 1, 44, 1, 2, 3, 4, 5, 6]
        assert d["subband_length"][2, 18] == 77 and d["subband_length"][0, 1] == 1 << 31 and d["subband_length"].sum() == 77 + (1 << 31)
        assert d["subband_quant_index"][0, 0] == 60 and d["subband_quant_index"][2, 18] == 9 and d["subband_quant_index"][1, 3] == 200
        assert d["subband_quant_index"].sum() == 269


def test_every_case_passes_and_takes_the_stated_scratch():
    """5 words per chunk slot (data_bytes / 8 + sub-bands + 1 per picture), 3 per codeblock, 8 per sub-band, 2 per picture."""
    lib = _lib.load()
    for case in DC.CASES + DC.HOSTILE:
        arr = sa.noarith_decode_pictures([fake_picture(case)])
        b = case.dtype.itemsize
        assert lib.schro_hip_noarith_decode_check(arr, 1, b) == 0, (case.name, lib.schro_hip_last_error())
        nsb = 3 * case.nsub
        ncb = 3 * sum(case.counts(i)[0] * case.counts(i)[1] for i in range(case.nsub))
        slots = case.data_bytes // 8 + nsb + 1
        assert lib.schro_hip_noarith_decode_scratch_words(arr, 1, b) == 5 * slots + 3 * ncb + 8 * nsb + 2, case.name
        # the slots suffice: a payload of n bytes takes (n + 7) / 8 chunks
        lengths = case.expected()[2]["subband_length"]
        assert sum(-(-min(int(v), case.data_bytes) // 8) for v in lengths.ravel()) <= slots or case.expected()[2]["truncated"]
    two = sa.noarith_decode_pictures([fake_picture(DC.CASES[0]), fake_picture(DC.CASES[2], 1)])
    one = [lib.schro_hip_noarith_decode_scratch_words(sa.noarith_decode_pictures([fake_picture(c)]), 1, 2) for c in (DC.CASES[0], DC.CASES[2])]
    assert lib.schro_hip_noarith_decode_scratch_words(two, 2, 2) == sum(one)


def test_kernels_are_in_the_library():
    """The kernels are in the gfx950 code object (a missing kernel is an error, not a fall-back)."""
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"nd_header_kernel", b"nd_summary_kernel", b"nd_chain_kernel", b"nd_decode_kernel", b"nd_fill_kernel"):
        assert kernel in blob, kernel
