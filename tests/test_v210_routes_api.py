"""CPU: the v210 route report (schro_hip_v210_routes) is declared, exported, bound and wrapped -- include/schro_hip.h's
route constants and prototype, the library's symbol, _lib's argtypes and Context.v210_routes."""
import ctypes as C
import os
import re

import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")


def test_header_declares_the_routes_and_the_call():
    text = open(HEADER).read()
    want = {"SCHRO_HIP_V210_ROUTE_HAAR3": 0, "SCHRO_HIP_V210_ROUTE_LEVEL": 1, "SCHRO_HIP_V210_ROUTE_TWO_PASS": 2,
            "SCHRO_HIP_V210_ROUTES": 3}
    for name, value in want.items():
        assert re.search(r"^#define %s %d\b" % (name, value), text, re.M), name
    assert re.search(r"int schro_hip_v210_routes \(SchroHipContext \* ctx, long long counts\[SCHRO_HIP_V210_ROUTES\], "
                     r"int reset\);", text)


def test_library_exports_and_binds_it():
    assert "schro_hip_v210_routes" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    f = lib.schro_hip_v210_routes
    assert f.argtypes == [C.c_void_p, C.POINTER(C.c_longlong), C.c_int]
    assert f.restype == C.c_int


def test_context_wraps_it():
    assert callable(getattr(sa.Context, "v210_routes", None))
    assert sa.Context.V210_ROUTES == ("haar3", "level", "two_pass")


def test_a_null_context_is_refused():
    lib = _lib.load()
    counts = (C.c_longlong * 3)(7, 7, 7)
    assert lib.schro_hip_v210_routes(None, counts, 0) != 0
    assert list(counts) == [7, 7, 7]
