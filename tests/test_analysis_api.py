"""CPU: the encoder-analysis entry points (schro_hip_downsample_batch, schro_hip_metric_scan_setup,
schro_hip_metric_scan_batch, schro_hipframe_downsample, schro_rough_me_heirarchical_scan_nohint_hip) are declared,
exported, bound and wrapped; their structs lie as the header says; schro_hip_metric_scan_setup agrees with
tests/analysis_ref.py on 10 000 seeded inputs; the two kernels are in both libraries without scratch memory; and the host
code -- 100 random batches, every refusal, the frame layer: tests/dry_run_analysis_cases.py -- runs clean on the device-free
sanitizer libraries in child processes, the way tests/test_iwt_forward_api.py runs tests/dry_run_fwd_cases.py."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import analysis_ref as A
import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
LLVM = "/opt/rocm/llvm/bin"
REPORT = re.compile(r"(ThreadSanitizer|AddressSanitizer|LeakSanitizer|UndefinedBehaviorSanitizer|runtime error:)")
CALLS = ("schro_hip_downsample_batch", "schro_hip_metric_scan_setup", "schro_hip_metric_scan_batch", "schro_hipframe_downsample",
         "schro_rough_me_heirarchical_scan_nohint_hip")
STRUCTS = {"SchroHipDownsamplePlane": _lib.DownsamplePlane, "SchroHipMetricScan": _lib.MetricScan,
           "SchroHipMetricScanResult": _lib.MetricScanResult, "SchroHipMetricScanPicture": _lib.MetricScanPicture}


def header_members(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s\*]", "", n) for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    return names


def test_header_declares_the_structs_and_the_calls():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int schro_hip_downsample_batch (SchroHipContext * ctx, const SchroHipDownsamplePlane * planes, int nplanes);",
                 "int schro_hip_metric_scan_setup (SchroHipMetricScan * scan, int frame_width, int frame_height, int extension, "
                 "int dx, int dy, int dist);",
                 "int schro_hip_metric_scan_batch (SchroHipContext * ctx, const SchroHipMetricScanPicture * pictures, int npictures);",
                 "int schro_hipframe_downsample (SchroHipFrame * dest, SchroHipFrame * src);",
                 "int schro_rough_me_heirarchical_scan_nohint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame, "
                 "const SchroHipParams * params, int shift, int distance, int ref, void *motion_vectors);"):
        assert decl in flat, decl
    for name, cls in STRUCTS.items():
        assert header_members(text, name) == [f[0] for f in cls._fields_], name
    assert C.sizeof(_lib.MetricScan) == 48 == sa.SCAN_DTYPE.itemsize
    assert C.sizeof(_lib.MetricScanResult) == 16 == sa.SCAN_RESULT_DTYPE.itemsize
    assert [n for n in sa.SCAN_DTYPE.names] == [f[0] for f in _lib.MetricScan._fields_]
    assert re.search(r"#define SCHRO_HIP_LIMIT_METRIC_SCAN 42\b", text) and sa.LIMIT_METRIC_SCAN == 42


def test_struct_layouts_match_the_header(tmp_path):
    lines = []
    for name, cls in STRUCTS.items():
        lines.append('  printf("%%zu", sizeof(%s));' % name)
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (name, f[0]) for f in cls._fields_]
        lines.append('  printf("\\n");')
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [list(map(int, line.split())) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    want = [[C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_] for cls in STRUCTS.values()]
    assert got == want


def test_library_exports_and_binds_them():
    lib = _lib.load()
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    for name in CALLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int
        assert hasattr(exp, name)
    assert lib.schro_hip_downsample_batch.argtypes == [C.c_void_p, C.POINTER(_lib.DownsamplePlane), C.c_int]
    assert lib.schro_hip_metric_scan_batch.argtypes == [C.c_void_p, C.POINTER(_lib.MetricScanPicture), C.c_int]
    assert lib.schro_hip_metric_scan_setup.argtypes == [C.POINTER(_lib.MetricScan)] + [C.c_int] * 6
    assert lib.schro_hipframe_downsample.argtypes == [C.POINTER(_lib.Frame), C.POINTER(_lib.Frame)]
    for name in ("downsample_batch", "metric_scan_batch", "rough_scan_nohint"):
        assert callable(getattr(sa.Context, name, None)), name
    assert callable(sa.metric_scan_setup)


def test_null_arguments_are_refused_with_a_message():
    lib = _lib.load()
    assert lib.schro_hip_downsample_batch(None, (_lib.DownsamplePlane * 1)(), 1) == -1
    assert b"downsample_batch" in lib.schro_hip_last_error()
    assert lib.schro_hip_metric_scan_batch(None, (_lib.MetricScanPicture * 1)(), 1) == -1
    assert b"metric_scan_batch" in lib.schro_hip_last_error()
    assert lib.schro_hipframe_downsample(None, None) == -1
    assert b"hipframe_downsample" in lib.schro_hip_last_error()
    assert lib.schro_rough_me_heirarchical_scan_nohint_hip(None, None, None, 0, 4, 0, None) == -1
    assert b"rough_me_heirarchical_scan_nohint_hip" in lib.schro_hip_last_error()
    assert lib.schro_hip_metric_scan_setup(None, 8, 8, 0, 0, 0, 4) == -1
    assert b"metric_scan_setup" in lib.schro_hip_last_error()


def test_metric_scan_setup_is_the_restatement_on_10000_inputs():
    """Pictures from 1 x 1, blocks from -4 (a block column right of the picture) to 64, positions on both sides of every
    edge, extensions 0 .. 32, vectors and distances that give windows of <= 0, of 1 and of over 42 positions."""
    lib = _lib.load()
    rng = np.random.default_rng(4242)
    seen = {"empty": 0, "over": 0, "ok": 0}
    for n in range(10000):
        w, h = (int(v) for v in rng.integers(1, 301, 2))
        ext = int(rng.choice([0, 1, 8, 32]))
        bw, bh = (int(v) for v in rng.integers(-4, 65, 2))
        x, y = int(rng.integers(-40, w + 41)), int(rng.integers(-40, h + 41))
        dx, dy = (int(v) for v in rng.integers(-40, 41, 2))
        dist = int(rng.integers(1, 26))
        want = A.scan_setup(x, y, bw, bh, w, h, ext, dx, dy, dist)
        s = _lib.MetricScan(x=x, y=y, block_width=bw, block_height=bh, gravity_x=11, gravity_y=-12, dx=13, dy=-14)
        rc = lib.schro_hip_metric_scan_setup(C.byref(s), w, h, ext, dx, dy, dist)
        over = want[2] > 42 or want[3] > 42
        assert rc == (-1 if over else 0), (n, rc, want)
        # (the reference sets the members before it asserts the limit)
        assert (s.ref_x, s.ref_y, s.scan_width, s.scan_height) == want, n
        assert (s.x, s.y, s.block_width, s.block_height, s.gravity_x, s.gravity_y, s.dx, s.dy) == (x, y, bw, bh, 11, -12, 13, -14)
        if not over:
            assert sa.metric_scan_setup(x, y, bw, bh, w, h, ext, dx, dy, dist) == want
        seen["over" if over else "empty" if want[2] <= 0 or want[3] <= 0 else "ok"] += 1
    assert min(seen.values()) > 100, seen
    s = _lib.MetricScan(x=4, y=4, block_width=8, block_height=8)
    for dist in (0, -3):
        assert lib.schro_hip_metric_scan_setup(C.byref(s), 64, 64, 8, 0, 0, dist) == -1


def test_the_product_keeps_to_the_two_allowed_preprocessor_guards():
    allowed = re.compile(r"^\s*#\s*(ifdef|ifndef|if)\s+(defined\s*\(?\s*)?(SCHRO_HIP_EXPERIMENTS|SCHRO_HIP_DRY|__HIPCC__|__cplusplus)\b")
    for name in ("analysis.hip", "plane_analysis.cpp", "frame.cpp", "schro_hip_internal.h"):
        path = os.path.join(CSRC, name)
        assert os.path.exists(path), name
        bad = [line for line in open(path) if re.match(r"^\s*#\s*(ifdef|ifndef|if)\b", line) and not allowed.match(line)]
        assert not bad, (name, bad)
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "analysis.hip" in srcs and "plane_analysis.cpp" in srcs


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
def test_both_kernels_are_built_without_scratch(lib, tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", "all"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    mine = {n: v for n, v in notes.items() if "downsample_kernel" in n or "metric_scan_kernel" in n}
    assert len(mine) == 2, sorted(mine)
    for n, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] == 0, (n, v)       # (the scan's LDS is sized by the launch)
        assert v["vgpr_count"] <= 128, (n, v)


def test_committed_resource_usage_lists_both_kernels_without_scratch():
    text = open(os.path.join(ROOT, "profiles", "r12_analysis_resource_usage.txt")).read()
    rows = re.findall(r"^(downsample_kernel|metric_scan_kernel) VGPRs (\d+) SGPRs (\d+) LDS (\d+) scratch (\d+) spillV (\d+)", text, re.M)
    assert sorted(r[0] for r in rows) == ["downsample_kernel", "metric_scan_kernel"]
    assert all(int(r[4]) == 0 and int(r[5]) == 0 for r in rows)


def run_dry(target, rt_name, env):
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.%s-x86_64.so" % rt_name))
    if not hits:
        pytest.skip("no %s runtime in this image" % rt_name)
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", target], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, SCHRO_HIP_LIB=os.path.join(ROOT, "schroedinger_amd", "libschro_hip_%s.so" % target), LD_PRELOAD=hits[-1], **env)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "tests/dry_run_analysis_cases.py", "-m", "not gpu"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found, "sanitizer report:\n" + text[max(0, found.start() - 200):found.start() + 4000]
    assert r.returncode == 0, text[-4000:]
    # the random batches, the refusals, the frame layer
    assert re.search(r"3 passed", text), text[-2000:]


@pytest.mark.timeout(1500)
def test_analysis_host_code_and_refusals_under_address_and_undefined_behaviour_sanitizers():
    run_dry("dry_asan", "asan", {"ASAN_OPTIONS": "detect_leaks=0:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=0"})


@pytest.mark.timeout(1500)
def test_analysis_host_code_and_refusals_under_thread_sanitizer():
    run_dry("dry_tsan", "tsan", {"TSAN_OPTIONS": "report_signal_unsafe=0:exitcode=66:halt_on_error=0"})
