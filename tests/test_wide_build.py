"""CPU, no device: the v216 / ARGB / AY64 level kernels are in both libraries for every sample type, filter and kernel family
and none of them uses scratch memory (the code objects' own metadata), and the new host code runs clean on the device-free
sanitizer twins (tests/dry_run_wide_cases.py in a child process under AddressSanitizer + UndefinedBehaviorSanitizer)."""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
LLVM = "/opt/rocm/llvm/bin"
REPORT = re.compile(r"(AddressSanitizer|LeakSanitizer|UndefinedBehaviorSanitizer|runtime error:)")


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
def test_every_wide_kernel_is_built_without_scratch(lib, tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", "all"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    wide = {n: v for n, v in notes.items() if "iiwt_wide_kernel" in n}
    # T in {s16, s32} x filters 0 - 6 x {v216, ARGB / AY64}
    want = {"iiwt_wide_kernelI%sLi%dELi%dE" % (t, f, v) for t in "si" for f in range(7) for v in (0, 1)}
    assert {re.search(r"iiwt_wide_kernelI[si]Li\dELi\dE", n).group(0) for n in wide} == want
    for n, v in wide.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] <= 65536, (n, v)


@pytest.mark.timeout(1500)
def test_host_code_on_the_dry_sanitizer_twins():
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    if not hits:
        pytest.skip("no AddressSanitizer runtime in this image")
    subprocess.run(["make", "-C", CSRC, "-j8", "-s", "dry_tsan", "dry_asan"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, SCHRO_HIP_LIB=os.path.join(ROOT, "schroedinger_amd", "libschro_hip_dry_asan.so"), LD_PRELOAD=hits[-1],
               ASAN_OPTIONS="detect_leaks=0:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "tests/dry_run_wide_cases.py", "-m", "not gpu"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found, "sanitizer report:\n" + text[max(0, found.start() - 200):found.start() + 4000]
    assert r.returncode == 0, text[-4000:]
    assert re.search(r"3 passed", text), text[-2000:]
