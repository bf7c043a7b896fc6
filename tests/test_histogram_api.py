"""CPU: the sub-band histograms are declared, exported, bound and wrapped; SchroHipHistogram has SchroHistogram's layout;
the kernels are in both libraries without scratch memory or spills; the kernel classes are what they were; the host code --
every refusal (SCHRO_HIP_EINVAL, the message naming plane and band), random batches, the frame layer with its table
rebuild and both queues: tests/dry_run_hist_cases.py -- runs clean on the device-free sanitizer libraries in child
processes, the way tests/test_quantise_api.py runs tests/dry_run_quant_cases.py."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import pytest

import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
REPORT = re.compile(r"(ThreadSanitizer|AddressSanitizer|LeakSanitizer|UndefinedBehaviorSanitizer|runtime error:)")
STRUCTS = {"SchroHipHistogramCounts": _lib.HistogramCounts, "SchroHipHistogramBand": _lib.HistogramBand,
           "SchroHipHistogramPlane": _lib.HistogramPlane, "SchroHipHistogram": _lib.Histogram}


def struct_members(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s\*]|\[.*\]", "", n) for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    return names


def test_header_declares_the_structs_and_the_calls():
    text = open(HEADER).read()
    for decl in (r"int schro_hip_histogram_batch \(SchroHipContext \* ctx, const SchroHipHistogramPlane \* planes, int nplanes, int bytes_per_sample\);",
                 r"int schro_hipframe_subband_histograms \(SchroHipFrame \* iwt_frame, const SchroHipParams \* params,"):
        assert re.search(decl, text), decl
    for name, cls in STRUCTS.items():
        assert struct_members(text, name) == [f[0] for f in cls._fields_], name
    assert int(re.search(r"#define SCHRO_HIP_HISTOGRAM_BINS (\d+)", text).group(1)) == _lib.HISTOGRAM_BINS == 104
    # the deliberate departure from the reference's unbounded index is stated where the counts are declared
    at = text.index("#define SCHRO_HIP_HISTOGRAM_BINS")
    above = text[text.rindex("/* ----", 0, at):at]
    assert "overflow" in above and "-32768" in above and "index 104" in above and "111" in above and "departure" in above


def test_struct_layout_matches_the_header(tmp_path):
    fields = [(n, f[0]) for n, cls in STRUCTS.items() for f in cls._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n'
                   + "".join('  printf("%%zu\\n", sizeof(%s));\n' % n for n in STRUCTS)
                   + "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % nf for nf in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(cls) for cls in STRUCTS.values()] + [getattr(STRUCTS[n], f).offset for n, f in fields]
    # SchroHistogram (schrohistogram.h:16-20): int n; double bins[104]
    assert C.sizeof(_lib.Histogram) == 840 and _lib.Histogram.bins.offset == 8 and _lib.Histogram.n.offset == 0
    assert C.sizeof(_lib.HistogramCounts) == 4 * 105 and _lib.HistogramCounts.overflow.offset == 4 * 104


def test_library_exports_and_binds_them():
    lib = _lib.load()
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    for name in ("schro_hip_histogram_batch", "schro_hipframe_subband_histograms"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int and hasattr(exp, name)
    assert lib.schro_hip_histogram_batch.argtypes == [C.c_void_p, C.POINTER(_lib.HistogramPlane), C.c_int, C.c_int]
    assert lib.schro_hipframe_subband_histograms.argtypes == [C.POINTER(_lib.Frame), C.POINTER(_lib.Params), C.POINTER(_lib.Histogram),
                                                              C.POINTER(C.c_uint32)]
    for name in ("histogram_batch", "histogram_planes", "subband_histograms"):
        assert callable(getattr(sa.Context, name, None)), name


def test_the_kernel_classes_are_what_they_were():
    assert sa.Context.KERNEL_CLASSES == ("iiwt_finest", "iiwt_coarse", "upsample", "obmc", "convert", "slices", "dc_predict",
                                         "dequant", "quantise", "quantise_dc")
    assert int(re.search(r"#define SCHRO_HIP_KERNEL_CLASSES (\d+)", open(HEADER).read()).group(1)) == 10


def test_a_null_context_is_refused_with_a_message():
    lib = _lib.load()
    planes = (_lib.HistogramPlane * 1)()
    assert lib.schro_hip_histogram_batch(None, planes, 1, 2) == -1
    assert b"histogram_batch" in lib.schro_hip_last_error()
    assert lib.schro_hipframe_subband_histograms(None, None, None, None) == -1
    assert b"hipframe_subband_histograms" in lib.schro_hip_last_error()


def test_sources_are_in_every_build_and_keep_to_the_allowed_guards():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "hist.hip" in srcs and "plane_hist.cpp" in srcs
    # the experiments and the dry libraries are built from SRCS
    assert re.search(r"^OBJS = \$\(addsuffix \.o,\$\(basename \$\(SRCS\)\)\)$", mk, re.M) and "$(OBJS)" in re.search(r"^EXPOBJS = (.*)$", mk, re.M).group(1)
    assert "$(OBJS)" in re.search(r"^DRYOBJS = (.*)$", mk, re.M).group(1)
    allowed = re.compile(r"^\s*#\s*(ifdef|ifndef|if)\s+(defined\s*\(?\s*)?(SCHRO_HIP_EXPERIMENTS|SCHRO_HIP_DRY|__HIPCC__|__cplusplus)\b")
    for name in ("hist.hip", "plane_hist.cpp"):
        bad = [line for line in open(os.path.join(CSRC, name)) if re.match(r"^\s*#\s*(ifdef|ifndef|if)\b", line) and not allowed.match(line)]
        assert not bad, (name, bad)


@pytest.mark.parametrize("lib", ["libschro_hip.so", "libschro_hip_exp.so"])
def test_every_histogram_kernel_is_built_without_scratch_or_spills(lib, tmp_path):
    from test_iwt_forward_api import LLVM, kernel_notes
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    mine = {n: v for n, v in notes.items() if "histogram_kernel" in n}
    names = {re.search(r"histogram_kernelI[si]Li\dE", n).group(0) for n in mine}
    # s16 and s32, the four lowest bins in registers; the experiments library: also none of them, and eight
    want = {"histogram_kernelI%sLi4E" % t for t in "si"}
    if "exp" in lib:
        want |= {"histogram_kernelI%sLi%dE" % (t, h) for t in "si" for h in (0, 8)}
    assert names == want
    for n, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] == 4 * 4 * 105, (n, v)     # a histogram per wave: 104 bins + overflow


def test_committed_resource_usage_lists_both_kernels_without_scratch():
    text = open(os.path.join(ROOT, "profiles", "r14_histogram_resource_usage.txt")).read()
    rows = re.findall(r"^histogram_kernel<(s16|s32),(\d)> VGPRs (\d+) SGPRs (\d+) LDS (\d+) scratch (\d+) spillS (\d+) spillV (\d+)", text, re.M)
    assert {(t, int(h)) for t, h, *_ in rows} >= {("s16", 4), ("s32", 4)}
    assert all(int(r[5]) == 0 and int(r[6]) == 0 and int(r[7]) == 0 for r in rows)


def run_dry(target, rt_name, env):
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.%s-x86_64.so" % rt_name))
    if not hits:
        pytest.skip("no %s runtime in this image" % rt_name)
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", target], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, SCHRO_HIP_LIB=os.path.join(ROOT, "schroedinger_amd", "libschro_hip_%s.so" % target), LD_PRELOAD=hits[-1], **env)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "tests/dry_run_hist_cases.py", "-m", "not gpu"],
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
