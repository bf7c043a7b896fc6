"""CPU: the encoder's quantisation and the frame subtract are declared, exported, bound and wrapped; the kernel's tables
are the reference's numbers; the kernels are in both libraries without scratch memory; the host code -- every refusal
(SCHRO_HIP_EINVAL, the message naming plane and record), random batches, the frame layer with its table rebuild:
tests/dry_run_quant_cases.py -- runs clean on the device-free sanitizer libraries in child processes, the way
tests/test_sanitizers.py runs tests/dry_run_cases.py."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import pytest

import quant_ref as Q
import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
REPORT = re.compile(r"(ThreadSanitizer|AddressSanitizer|LeakSanitizer|UndefinedBehaviorSanitizer|runtime error:)")


def struct_members(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s\*]", "", n) for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    return names


def test_header_declares_the_structs_and_the_calls():
    text = open(HEADER).read()
    for decl in (r"int schro_hip_quantise_batch \(SchroHipContext \* ctx, const SchroHipQuantPlane \* planes, int nplanes, int bytes_per_sample\);",
                 r"int schro_hip_subtract_batch \(SchroHipContext \* ctx, const SchroHipConvertPlane \* planes, int nplanes, int src_is_u8\);",
                 r"int schro_hipframe_subtract \(SchroHipFrame \* dest, SchroHipFrame \* src\);",
                 r"int schro_hipframe_quantise \(SchroHipFrame \* quant_frame, SchroHipFrame \* iwt_frame, const SchroHipParams \* params,"):
        assert re.search(decl, text), decl
    assert struct_members(text, "SchroHipQuantPlane") == [f[0] for f in _lib.QuantPlane._fields_]
    assert struct_members(text, "SchroHipCodeblockSummary") == [f[0] for f in _lib.CodeblockSummary._fields_] == ["nonzero", "max_abs"]
    assert int(re.search(r"#define SCHRO_HIP_QUANTISE_DC_THREADS (\d+)", text).group(1)) == sa.QUANTISE_DC_THREADS
    # the deliberate departure from the reference's zero test is stated where the summary is declared
    assert "schro_frame_data_is_zero" in text and "65536" in text


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(SchroHipQuantPlane), offsetof(SchroHipQuantPlane, bytes),\n'
                   '         offsetof(SchroHipQuantPlane, ncodeblocks), offsetof(SchroHipQuantPlane, dc_height),\n'
                   '         offsetof(SchroHipQuantPlane, summary), sizeof(SchroHipCodeblockSummary));\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    P = _lib.QuantPlane
    assert got == [C.sizeof(P), P.bytes.offset, P.ncodeblocks.offset, P.dc_height.offset, P.summary.offset, C.sizeof(_lib.CodeblockSummary)]


def test_library_exports_and_binds_them():
    lib = _lib.load()
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    for name in ("schro_hip_quantise_batch", "schro_hip_subtract_batch", "schro_hipframe_subtract", "schro_hipframe_quantise"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int and hasattr(exp, name)
    assert lib.schro_hip_quantise_batch.argtypes == [C.c_void_p, C.POINTER(_lib.QuantPlane), C.c_int, C.c_int]
    assert callable(getattr(sa.Context, "quantise_batch", None)) and callable(getattr(sa.Context, "subtract_batch", None))
    assert sa.Context.KERNEL_CLASSES[8:] == ("quantise", "quantise_dc")
    assert int(re.search(r"#define SCHRO_HIP_KERNEL_CLASSES (\d+)", open(HEADER).read()).group(1)) == len(sa.Context.KERNEL_CLASSES)


def test_a_null_context_is_refused_with_a_message():
    lib = _lib.load()
    planes = (_lib.QuantPlane * 1)()
    assert lib.schro_hip_quantise_batch(None, planes, 1, 2) == -1
    assert b"quantise_batch" in lib.schro_hip_last_error()
    assert lib.schro_hip_subtract_batch(None, None, 1, 0) == -1
    assert b"subtract_batch" in lib.schro_hip_last_error()
    assert lib.schro_hipframe_quantise(None, None, None, None, None) == -1
    assert b"hipframe_quantise" in lib.schro_hip_last_error()
    assert lib.schro_hipframe_subtract(None, None) == -1
    assert b"hipframe_subtract" in lib.schro_hip_last_error()


def test_the_kernel_source_holds_the_reference_inverse_table():
    """schro_table_inverse_quant has no closed form: quant.hip carries its 61 numbers, and they are the reference's."""
    text = open(os.path.join(CSRC, "quant.hip")).read()
    body = re.search(r"constexpr uint16_t inv\[61\] = \{(.*?)\};", text, re.S).group(1)
    assert [int(v) for v in re.findall(r"\d+", body)] == Q.tables()["schro_table_inverse_quant"]


def test_sources_are_in_every_build_and_keep_to_the_allowed_guards():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "quant.hip" in srcs and "plane_quant.cpp" in srcs
    allowed = re.compile(r"^\s*#\s*(ifdef|ifndef|if)\s+(defined\s*\(?\s*)?(SCHRO_HIP_EXPERIMENTS|SCHRO_HIP_DRY|__HIPCC__|__cplusplus)\b")
    for name in ("quant.hip", "plane_quant.cpp"):
        bad = [line for line in open(os.path.join(CSRC, name)) if re.match(r"^\s*#\s*(ifdef|ifndef|if)\b", line) and not allowed.match(line)]
        assert not bad, (name, bad)


@pytest.mark.parametrize("lib", ["libschro_hip.so", "libschro_hip_exp.so"])
def test_every_quantise_kernel_is_built_without_scratch(lib, tmp_path):
    from test_iwt_forward_api import LLVM, kernel_notes
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    mine = {n: v for n, v in notes.items() if re.search(r"quantise_(dc_)?kernelI[si]E", n)}
    assert {re.search(r"quantise_(?:dc_)?kernelI[si]E", n).group(0) for n in mine} == {
        "quantise_kernelIsE", "quantise_kernelIiE", "quantise_dc_kernelIsE", "quantise_dc_kernelIiE"}
    for n, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)


def run_dry(target, rt_name, env):
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.%s-x86_64.so" % rt_name))
    if not hits:
        pytest.skip("no %s runtime in this image" % rt_name)
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", target], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, SCHRO_HIP_LIB=os.path.join(ROOT, "schroedinger_amd", "libschro_hip_%s.so" % target), LD_PRELOAD=hits[-1], **env)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "tests/dry_run_quant_cases.py", "-m", "not gpu"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found, "sanitizer report:\n" + text[max(0, found.start() - 200):found.start() + 4000]
    assert r.returncode == 0, text[-4000:]
    # the refusals, the random batches, the frame layer
    assert re.search(r"3 passed", text), text[-2000:]


@pytest.mark.timeout(1500)
def test_refusals_and_host_code_under_address_and_undefined_behaviour_sanitizers():
    run_dry("dry_asan", "asan", {"ASAN_OPTIONS": "detect_leaks=0:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=0"})


@pytest.mark.timeout(1500)
def test_refusals_and_host_code_under_thread_sanitizer():
    run_dry("dry_tsan", "tsan", {"TSAN_OPTIONS": "report_signal_unsafe=0:exitcode=66:halt_on_error=0"})
