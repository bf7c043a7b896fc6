"""CPU: the host code of the whole mode decision -- plane_mode.cpp and the refusals of plane_split2.cpp under it -- under
AddressSanitizer + UndefinedBehaviorSanitizer, from a stand-alone program (tests/c/mode_walk.cpp: its own main, compiled
with the sanitizer, linked against the device-free sanitizer objects of the library; nothing is preloaded and no Python is
in the process).  The program walks every refusal and the three batch calls over pictures of every geometry class, then on
contexts of their own the frame-layer runs of the motion stages in small, large, small order (they size the queue's scratch
themselves and copy to and from host fields of the exact size); a sanitizer report or a non-zero exit fails the test with
the text.  Leak detection is on."""
import os
import subprocess

import pytest

from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def test_the_mode_decision_host_code_under_asan_and_ubsan():
    if not clang_runtime("asan"):
        pytest.skip("no asan runtime in this image")
    make = subprocess.run(["make", "-C", CDIR, "-f", "mode_walk.mk", "-j8", "-s", "mode_walk_asan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([os.path.join(CDIR, "_build", "mode_walk_asan")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found and r.returncode == 0, text[-6000:]
    assert "mode_walk: 8 pictures, ok" in text
    assert "mode_walk: frame layer small, large, small: 3 pictures on each queue, ok" in text
