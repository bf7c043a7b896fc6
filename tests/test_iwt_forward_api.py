"""CPU: the forward wavelet (schro_hip_iwt_batch, the frame layer's schro_hipframe_iwt_transform) is declared, exported,
bound and wrapped; its level kernels are in both libraries for every sample type and filter without scratch memory; its
host code -- 100 random batches, every refusal (SCHRO_HIP_EINVAL with a message), the frame layer: tests/dry_run_fwd_cases.py
-- runs clean on the device-free sanitizer libraries (ThreadSanitizer; AddressSanitizer + UndefinedBehaviorSanitizer) in
child processes, the way tests/test_sanitizers.py runs tests/dry_run_cases.py."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
LLVM = "/opt/rocm/llvm/bin"
REPORT = re.compile(r"(ThreadSanitizer|AddressSanitizer|LeakSanitizer|UndefinedBehaviorSanitizer|runtime error:)")


def test_header_declares_the_struct_and_the_calls():
    text = open(HEADER).read()
    assert re.search(r"int schro_hip_iwt_batch \(SchroHipContext \* ctx, const SchroHipIwtFwdPlane \* planes, int nplanes, "
                     r"int depth, int filter,\s+int bytes_per_sample\);", text)
    assert re.search(r"int schro_hipframe_iwt_transform \(SchroHipContext \* ctx, SchroHipFrame \* frame, "
                     r"const SchroHipParams \* params\);", text)
    body = re.search(r"typedef struct \{([^}]*)\} SchroHipIwtFwdPlane;", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s\*]", "", n) for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    assert names == [f[0] for f in _lib.IwtFwdPlane._fields_] == ["src", "src_stride", "dst", "dst_stride", "width", "height"]
    # LP64: (pointer + int + pad) twice + 2 ints
    assert C.sizeof(_lib.IwtFwdPlane) == 40


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(SchroHipIwtFwdPlane), offsetof(SchroHipIwtFwdPlane, dst),\n'
                   '         offsetof(SchroHipIwtFwdPlane, dst_stride), offsetof(SchroHipIwtFwdPlane, width));\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    P = _lib.IwtFwdPlane
    assert got == [C.sizeof(P), P.dst.offset, P.dst_stride.offset, P.width.offset]


def test_library_exports_and_binds_them():
    lib = _lib.load()
    for name in ("schro_hip_iwt_batch", "schro_hipframe_iwt_transform"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int
    assert lib.schro_hip_iwt_batch.argtypes == [C.c_void_p, C.POINTER(_lib.IwtFwdPlane), C.c_int, C.c_int, C.c_int, C.c_int]
    assert lib.schro_hipframe_iwt_transform.argtypes == [C.c_void_p, C.POINTER(_lib.Frame), C.POINTER(_lib.Params)]
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    assert hasattr(exp, "schro_hip_iwt_batch") and hasattr(exp, "schro_hipframe_iwt_transform")
    assert callable(getattr(sa.Context, "iwt_batch", None))


def test_a_null_context_is_refused_with_a_message():
    lib = _lib.load()
    planes = (_lib.IwtFwdPlane * 1)()
    assert lib.schro_hip_iwt_batch(None, planes, 1, 3, 0, 2) == -1
    assert b"iwt_batch" in lib.schro_hip_last_error()
    assert lib.schro_hipframe_iwt_transform(None, None, None) == -1
    assert b"hipframe_iwt_transform" in lib.schro_hip_last_error()


def test_the_product_keeps_to_the_two_allowed_preprocessor_guards():
    """tests/test_abi.py's rule, on the files of the forward transform by name: every preprocessor conditional is the
    experiments guard, the device-free build's, or the shared header's include / __HIPCC__ / __cplusplus plumbing."""
    allowed = re.compile(r"^\s*#\s*(ifdef|ifndef|if)\s+(defined\s*\(?\s*)?(SCHRO_HIP_EXPERIMENTS|SCHRO_HIP_DRY|__HIPCC__|__cplusplus)\b")
    for name in ("iwt_fwd.hip", "plane_iwt.cpp", "frame.cpp", "schro_hip_internal.h", "iiwt_steps.h"):
        path = os.path.join(CSRC, name)
        assert os.path.exists(path), name
        bad = [line for line in open(path) if re.match(r"^\s*#\s*(ifdef|ifndef|if)\b", line) and not allowed.match(line)]
        assert not bad, (name, bad)
    # ... and the Makefile compiles the new sources into every library (the dry rules take the same list)
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "iwt_fwd.hip" in srcs and "plane_iwt.cpp" in srcs


def kernel_notes(lib, tmp_path):
    """{kernel name: {metadata key: int}} of every gfx950 code object bundled in `lib`."""
    work = tmp_path / os.path.basename(lib)
    work.mkdir()
    shutil.copy(lib, work)      # (the bundles are extracted next to the file)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(lib)], cwd=work, check=True, stdout=subprocess.DEVNULL)
    out = {}
    for co in sorted(glob.glob(str(work / "*gfx950*"))):
        text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, stdout=subprocess.PIPE).stdout.decode()
        for block in text.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            out[name] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count|"
                                                          r"group_segment_fixed_size|vgpr_count):\s+(\d+)", block)}
    return out


@pytest.mark.parametrize("lib", ["libschro_hip.so", "libschro_hip_exp.so"])
def test_every_forward_kernel_is_built_without_scratch(lib, tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", "all"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    fwd = {n: v for n, v in notes.items() if "iwt_fwd_level_kernel" in n}
    # T in {s16, s32} x filters 0 - 6
    want = {"iwt_fwd_level_kernelI%sLi%dE" % (t, f) for t in "si" for f in range(7)}
    assert {re.search(r"iwt_fwd_level_kernelI[si]Li\dE", n).group(0) for n in fwd} == want
    for n, v in fwd.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] <= 65536, (n, v)


def test_committed_resource_usage_lists_every_instantiation_without_scratch():
    text = open(os.path.join(ROOT, "profiles", "r11_iwt_fwd_resource_usage.txt")).read()
    rows = re.findall(r"^iwt_fwd_level_kernel<(s16|s32),(\d)> VGPRs (\d+) SGPRs (\d+) LDS (\d+) scratch (\d+) spillV (\d+)", text, re.M)
    assert sorted((t, int(f)) for t, f, *_ in rows) == [(t, f) for t in ("s16", "s32") for f in range(7)]
    assert all(int(r[5]) == 0 and int(r[6]) == 0 for r in rows)


def run_dry(target, rt_name, env):
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.%s-x86_64.so" % rt_name))
    if not hits:
        pytest.skip("no %s runtime in this image" % rt_name)
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", target], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, SCHRO_HIP_LIB=os.path.join(ROOT, "schroedinger_amd", "libschro_hip_%s.so" % target), LD_PRELOAD=hits[-1], **env)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "tests/dry_run_fwd_cases.py", "-m", "not gpu"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found, "sanitizer report:\n" + text[max(0, found.start() - 200):found.start() + 4000]
    assert r.returncode == 0, text[-4000:]
    # the random batches, the refusals, the frame layer
    assert re.search(r"3 passed", text), text[-2000:]


@pytest.mark.timeout(1500)
def test_forward_host_code_and_refusals_under_address_and_undefined_behaviour_sanitizers():
    run_dry("dry_asan", "asan", {"ASAN_OPTIONS": "detect_leaks=0:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=0"})


@pytest.mark.timeout(1500)
def test_forward_host_code_and_refusals_under_thread_sanitizer():
    run_dry("dry_tsan", "tsan", {"TSAN_OPTIONS": "report_signal_unsafe=0:exitcode=66:halt_on_error=0"})
