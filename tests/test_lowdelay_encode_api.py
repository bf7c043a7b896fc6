"""CPU: the low-delay slice encoder is declared, exported, bound and wrapped; its struct has the header's layout; its three
kernels are in both libraries without scratch memory or spills; the departures from the reference are stated in the header."""
import ctypes as C
import os
import re
import subprocess

import pytest

import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
KERNELS = ("ldenc_estimate_kernel", "ldenc_choose_kernel", "ldenc_pack_kernel")


def test_header_declares_and_states_the_departures():
    text = open(HEADER).read()
    assert "int schro_hip_lowdelay_encode_batch (SchroHipContext * ctx," in text
    assert "int schro_hip_encode_lowdelay_transform_data (const SchroHipFrame * iwt_frame" in text
    at = text.index("} SchroHipLowDelayEncodePicture;")
    above = text[text.rindex("/* ----", 0, at):at]
    for word in ("departure", "untouched", "const", "schro_hip_lowdelay_batch", "asserts", "s32", "chroma LL"):
        assert word in above, word


def test_struct_layout_matches_the_header(tmp_path):
    cls = _lib.LowDelayEncodePicture
    fields = [f[0] for f in cls._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(SchroHipLowDelayEncodePicture));\n'
                   + "".join('  printf("%%zu\\n", offsetof(SchroHipLowDelayEncodePicture, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


def test_library_exports_and_binds_them():
    lib = _lib.load()
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    for name in ("schro_hip_lowdelay_encode_batch", "schro_hip_encode_lowdelay_transform_data"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name).restype == C.c_int and hasattr(exp, name)
    for name in ("lowdelay_encode_batch", "encode_lowdelay"):
        assert callable(getattr(sa.Context, name, None)), name
    pics = (_lib.LowDelayEncodePicture * 1)()
    assert lib.schro_hip_lowdelay_encode_batch(None, pics, 1, None, 2) == -1
    assert b"lowdelay_encode_batch" in lib.schro_hip_last_error()
    assert lib.schro_hip_encode_lowdelay_transform_data(None, None, 0, None, None, None) == -1
    assert b"encode_lowdelay_transform_data" in lib.schro_hip_last_error()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "lowdelay_enc.hip" in srcs and "plane_lowdelay_enc.cpp" in srcs


@pytest.mark.parametrize("lib", ["libschro_hip.so", "libschro_hip_exp.so"])
def test_the_three_kernels_are_built_without_scratch_or_spills(lib, tmp_path):
    from test_iwt_forward_api import LLVM, kernel_notes
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    for k in KERNELS:
        mine = [v for n, v in notes.items() if k in n]
        assert len(mine) == 1, k
        v = mine[0]
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (k, v)


def test_committed_resource_usage_lists_the_kernels_without_scratch():
    text = open(os.path.join(ROOT, "profiles", "r15_lowdelay_encode_resource_usage.txt")).read()
    for k in KERNELS:
        block = text[text.index("Function Name: " + k):]
        block = block[:block.index("LDS Size")]
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", block) and re.search(r"SGPRs Spill: 0\b", block) \
            and re.search(r"VGPRs Spill: 0\b", block), k

