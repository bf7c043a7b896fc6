"""CPU: the > 8-bit packed finish (schro_hip_iiwt_pack_wide_batch, schro_hip_wide_routes, the frame layer's
schro_frame_inverse_iwt_transform_shift_convert_hip) is declared, exported, bound and wrapped -- include/schro_hip.h's
route constants, struct and prototypes, the library's symbols, _lib's argtypes and struct layout, the Context wrappers."""
import ctypes as C
import os
import re

import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")


def test_header_declares_the_routes_and_the_calls():
    text = open(HEADER).read()
    want = {"SCHRO_HIP_WIDE_ROUTE_LEVEL": 0, "SCHRO_HIP_WIDE_ROUTE_TWO_PASS": 1, "SCHRO_HIP_WIDE_ROUTES": 2}
    for name, value in want.items():
        assert re.search(r"^#define %s %d\b" % (name, value), text, re.M), name
    assert re.search(r"int schro_hip_wide_routes \(SchroHipContext \* ctx, long long counts\[SCHRO_HIP_WIDE_ROUTES\], "
                     r"int reset\);", text)
    assert re.search(r"int schro_hip_iiwt_pack_wide_batch \(SchroHipContext \* ctx, const SchroHipIwtPackWidePicture \* pictures, "
                     r"int npictures, int depth,\s+int filter, int bytes_per_sample\);", text)
    assert re.search(r"int schro_frame_inverse_iwt_transform_shift_convert_hip \(SchroHipFrame \* packed, SchroHipFrame \* "
                     r"transform_frame,\s+SchroHipParams \* params, int shift\);", text)


def test_the_struct_is_the_headers():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} SchroHipIwtPackWidePicture;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s\*]|\[\d+\]", "", n) for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    assert names == [f[0] for f in _lib.IwtPackWidePicture._fields_]
    # the layout of SchroHipIwtPackPicture plus format and shift
    assert names[:-2] == [f[0] for f in _lib.IwtPackPicture._fields_]
    # LP64: 3 pointers + 3 ints + 4 ints (+ pad) + pointer + 5 ints (+ pad)
    assert C.sizeof(_lib.IwtPackWidePicture) == 24 + 12 + 16 + 4 + 8 + 20 + 4


def test_library_exports_and_binds_them():
    lib = _lib.load()
    for name in ("schro_hip_wide_routes", "schro_hip_iiwt_pack_wide_batch", "schro_frame_inverse_iwt_transform_shift_convert_hip"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int
    assert lib.schro_hip_wide_routes.argtypes == [C.c_void_p, C.POINTER(C.c_longlong), C.c_int]
    assert lib.schro_hip_iiwt_pack_wide_batch.argtypes == [C.c_void_p, C.POINTER(_lib.IwtPackWidePicture), C.c_int, C.c_int, C.c_int, C.c_int]
    assert lib.schro_frame_inverse_iwt_transform_shift_convert_hip.argtypes == [C.POINTER(_lib.Frame), C.POINTER(_lib.Frame),
                                                                                C.POINTER(_lib.Params), C.c_int]


def test_context_wraps_them():
    assert callable(getattr(sa.Context, "wide_routes", None))
    assert callable(getattr(sa.Context, "iiwt_pack_wide_batch", None))
    assert sa.Context.WIDE_ROUTES == ("level", "two_pass")


def test_a_null_context_is_refused():
    lib = _lib.load()
    counts = (C.c_longlong * 2)(7, 7)
    assert lib.schro_hip_wide_routes(None, counts, 0) != 0
    assert list(counts) == [7, 7]
    pic = (_lib.IwtPackWidePicture * 1)()
    assert lib.schro_hip_iiwt_pack_wide_batch(None, pic, 1, 3, 0, 4) != 0
    assert lib.schro_frame_inverse_iwt_transform_shift_convert_hip(None, None, None, 0) != 0
