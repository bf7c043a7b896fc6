"""CPU: schro_hip_iiwt_pack_v210_batch refuses what schro_hip_iiwt_batch refuses -- a component that is not a multiple of
2^depth (chroma: width / 2) or a src_stride that does not hold the component's row -- whichever route would take the
picture, and counts nothing for a refused call.  Run without a device against the sanitizers' device-free build
(libschro_hip_dry_asan.so, schroedinger_amd/csrc/schro_hip_dry.h: launches are dropped, the host code runs) in a child
process with the AddressSanitizer runtime preloaded, as tests/test_sanitizers.py does."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")

CHILD = r'''
import numpy as np
import schroedinger_amd as sa

ctx = sa.Context(0)

def call(w, h, depth, dtype=np.int32, luma_stride=None, filt=0):
    bpp = np.dtype(dtype).itemsize
    co = [ctx.plane(h, w, dtype, stride=luma_stride), ctx.plane(h, w // 2, dtype), ctx.plane(h, w // 2, dtype)]
    dst = ctx.plane(h, 16 * (-(-w // 6)), np.uint8, stride=(16 * (-(-w // 6)) + 15) // 16 * 16)
    ctx.v210_routes(reset=True)
    try:
        ctx.iiwt_pack_v210_batch([(co, 1, 0, dst, w, h)], depth, filt)
        ok = True
    except sa.SchroHipError:
        ok = False
    routes = ctx.v210_routes(reset=True)
    [p.free() for p in co + [dst]]
    return ok, routes

NONE = {"haar3": 0, "level": 0, "two_pass": 0}
refused = [
    (42, 8, 1, None),           # chroma 21 columns at depth 1
    (48, 9, 1, None),           # 9 rows at depth 1
    (48, 8, 1, 96),             # a luma stride of 96 bytes for 48 s32 samples
    (96, 16, 2, 192),           # a luma stride of 192 bytes for 96 s32 samples
    (96, 17, 2, None),          # 17 rows at depth 2
    (40, 16, 3, None),          # 40 columns at depth 3
]
for (w, h, depth, stride) in refused:
    ok, routes = call(w, h, depth, luma_stride=stride)
    assert not ok and routes == NONE, ("accepted", w, h, depth, stride, routes)
    ok, routes = call(w, h, depth, luma_stride=stride, filt=3)
    assert not ok and routes == NONE, ("accepted (Haar)", w, h, depth, stride, routes)
# the same sizes made legal are taken
for (w, h, depth) in [(44, 8, 1), (48, 10, 1), (48, 8, 1), (96, 16, 2), (96, 20, 2), (48, 16, 3)]:
    for dtype in (np.int16, np.int32):
        ok, routes = call(w, h, depth, dtype)
        assert ok and routes == dict(NONE, level=1), ("refused", w, h, depth, routes)
ctx.close()
print("V210_VALIDATION_OK")
'''


def clang_runtime(name):
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.%s-x86_64.so" % name))
    return hits[-1] if hits else None


@pytest.mark.timeout(1500)
def test_iiwt_pack_v210_refuses_what_the_transform_refuses():
    rt = clang_runtime("asan")
    if not rt:
        pytest.skip("no AddressSanitizer runtime in this image")
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", "dry_asan"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, SCHRO_HIP_LIB=os.path.join(ROOT, "schroedinger_amd", "libschro_hip_dry_asan.so"), LD_PRELOAD=rt,
               ASAN_OPTIONS="detect_leaks=0:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0",
               PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "V210_VALIDATION_OK" in text, text[-4000:]
    assert "runtime error:" not in text and "AddressSanitizer" not in text, text[-4000:]
