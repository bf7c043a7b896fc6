"""CPU: the noarith transform-data encoder is declared, exported, bound and wrapped; schro_hip_noarith_encode_check walks
the refusal table of tests/noarith_enc_cases.py (SCHRO_HIP_EINVAL, the message naming picture, component and sub-band or
record) and accepts the other side of every limit; the records of schro_hip_codeblock_layout pass for every case and
draw; schro_hip_noarith_encode_bound covers what the restatement writes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noarith_enc_cases as NC
import noarith_enc_draws as ND
import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
EINVAL = -1


def test_header_declares_and_the_library_exports():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in ("schro_hip_noarith_encode_bound", "schro_hip_noarith_encode_batch", "schro_hip_noarith_encode_check",
                 "schro_hip_encode_transform_data_noarith"):
        assert re.search(r"\b%s \(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name)
    assert "#define SCHRO_HIP_NOARITH_MAX_SUBBANDS %d" % _lib.NOARITH_MAX_SUBBANDS in text
    # the structs: member for member (sizes on LP64)
    assert C.sizeof(_lib.NoarithResult) == 4 * (4 + 3 * 19)
    assert C.sizeof(_lib.NoarithPicture) == 24 + 24 + 12 + 12 + 12 + 4 + 24 + 12 + 4 + 28 + 28 + 4 + 4 + 8 + 8 + 8
    for member in ("quant", "bytes", "stride", "iwt_width", "iwt_height", "codeblocks", "ncodeblocks", "transform_depth",
                   "horiz_codeblocks", "vert_codeblocks", "codeblock_mode_index", "out", "capacity", "result"):
        assert hasattr(_lib.NoarithPicture, member)
    for name in ("noarith_encode_batch", "encode_transform_data_noarith"):
        assert callable(getattr(sa.Context, name))
    assert callable(sa.noarith_encode_check) and callable(sa.noarith_encode_bound)


def check(d):
    lib = _lib.load()
    pic, keep = NC.c_picture(d, _lib, C)
    rc = lib.schro_hip_noarith_encode_check(C.byref(pic), 1, d["bpp"])
    return rc, lib.schro_hip_last_error().decode()


@pytest.mark.parametrize("name,change,message", NC.REFUSALS, ids=[r[0] for r in NC.REFUSALS])
def test_refusals(name, change, message):
    d = NC.describe()
    assert check(d)[0] == 0
    change(d)
    rc, text = check(d)
    assert rc == EINVAL and message in text and text.startswith("noarith_encode_batch:"), (rc, text)


@pytest.mark.parametrize("name,change", NC.ACCEPTED, ids=[r[0] for r in NC.ACCEPTED])
def test_the_other_side_of_the_limits_passes(name, change):
    d = NC.describe()
    change(d)
    rc, text = check(d)
    assert rc == 0, text


def test_the_bound_limit_on_s32():
    for change, want in ((NC.REFUSALS[-1][1], EINVAL), (NC.ACCEPTED[-1][1], 0)):
        d = NC.describe(bpp=4)
        change(d)
        rc, text = check(d)
        assert rc == want, text


def test_empty_and_oversized_calls():
    lib = _lib.load()
    pic, keep = NC.c_picture(NC.describe(), _lib, C)
    assert lib.schro_hip_noarith_encode_check(None, 1, 2) == EINVAL
    assert lib.schro_hip_noarith_encode_check(C.byref(pic), 0, 2) == EINVAL
    assert lib.schro_hip_noarith_encode_batch(None, C.byref(pic), 1, 2) == EINVAL
    assert lib.schro_hip_noarith_encode_bound(None, 2) == EINVAL
    assert lib.schro_hip_encode_transform_data_noarith(None, None, None, None, 0, None, None, None) == EINVAL
    assert b"encode_transform_data_noarith" in lib.schro_hip_last_error()
    many = (_lib.NoarithPicture * 257)(*([pic] * 257))
    assert lib.schro_hip_noarith_encode_check(many, 257, 2) == EINVAL


def test_layout_records_pass_for_every_case_and_draw():
    """The check holds the records against closed forms (xmin = x bw / hc); schro_hip_codeblock_layout accumulates as the
    decoder does.  They agree on every geometry of the suite, at two pitches."""
    lib = _lib.load()
    for case in NC.CASES + ND.DRAWS:
        b = case.dtype.itemsize
        for pad in (0, 3):
            d = {"bpp": b, "depth": case.depth, "mode": case.mode, "sizes": case.sizes, "hc": case.hc, "vc": case.vc}
            d["stride"] = [(w * b + 63) // 64 * 64 + pad * b for w, h in case.sizes]
            d["bytes"] = [s * h for s, (w, h) in zip(d["stride"], case.sizes)]
            d["records"] = []
            for k, (w, h) in enumerate(case.sizes):
                hc, vc = (C.c_int * 7)(*case.hc), (C.c_int * 7)(*case.vc)
                n = lib.schro_hip_codeblock_layout(w, h, case.depth, hc, vc, d["stride"][k], b, None, 0)
                tab = (_lib.Codeblock * n)()
                lib.schro_hip_codeblock_layout(w, h, case.depth, hc, vc, d["stride"][k], b, tab, n)
                recs = [[t.dst_offset, t.dst_stride, t.width, t.height, -1, 0, q] for t, q in zip(tab, case.record_indices(k))]
                assert [r[:4] for r in recs] == [r[:4] for r in NC.layout_records(w, h, case.depth, case.hc, case.vc, d["stride"][k], b)]
                d["records"].append(recs)
            d["quant"], d["out"], d["capacity"], d["result"] = [1 << 28, 2 << 28, 3 << 28], 4 << 28, 1 << 20, 5 << 28
            rc, text = check(d)
            assert rc == 0, (case.name, text)


def test_bound_covers_the_restatement():
    for case in NC.CASES + ND.DRAWS:
        b = case.dtype.itemsize
        bound = sa.noarith_encode_bound(case.sizes, case.depth, case.hc, case.vc, b)
        want = 0
        for k, (w, h) in enumerate(case.sizes):
            for i in range(case.nsub):
                hc, vc = case.counts(i)
                bh, bw = case.band(k, i).shape
                want += bw * bh * 2 * b + (2 * hc * vc + 7) // 8 + 10
        assert bound == want and len(case.expected()[0]) <= bound, case.name
    # the longest codes fill 4 / 8 bytes per sample exactly
    for name in ("s16-window-64", "s32-window-65"):
        case = NC.BY_NAME[name]
        samples = sum(w * h for w, h in case.sizes)
        assert len(case.expected()[0]) > samples * 2 * case.dtype.itemsize - samples // 2
    with pytest.raises(sa.SchroHipError, match="transform_depth 7"):
        sa.noarith_encode_bound([(128, 128)] * 3, 7, [1] * 7, [1] * 7, 2)


def test_kernels_are_in_the_library_without_scratch():
    """The four kernels are in the gfx950 code object (a missing kernel is an error, not a fall-back)."""
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"na_count_kernel", b"na_layout_kernel", b"na_clear_kernel", b"na_pack_kernel"):
        assert kernel in blob, kernel
