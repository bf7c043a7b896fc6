"""CPU: the host code of the picture statistics (plane_stats.cpp, the frame layer's five calls) under AddressSanitizer +
UndefinedBehaviorSanitizer, from a stand-alone program (tests/c/picture_stats_walk.cpp: its own main, compiled with the
sanitizer, linked against the device-free sanitizer objects of the library; nothing is preloaded and no Python is in the
process).  The program walks every refusal through the _check twin and the batch call, each batch call in a small,
larger, small order on two queues, the most entries a call takes, and the frame layer's calls on u8 and s16 frames; a
sanitizer report or a non-zero exit fails the test with the text.  Leak detection is on."""
import os
import subprocess

import pytest

from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def test_the_picture_stats_host_code_under_asan_and_ubsan():
    if not clang_runtime("asan"):
        pytest.skip("no asan runtime in this image")
    make = subprocess.run(["make", "-C", CDIR, "-f", "picture_stats_walk.mk", "-j8", "-s", "picture_stats_walk_asan"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([os.path.join(CDIR, "_build", "picture_stats_walk_asan")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found and r.returncode == 0, text[-6000:]
    assert "picture_stats_walk: 34 refusals, 29 calls, ok" in text
