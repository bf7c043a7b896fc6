"""CPU: the host code of the encoder's way in (plane_unpack.cpp, the packed level 0 of plane_iwt.cpp, the frame layer's two
calls) under AddressSanitizer + UndefinedBehaviorSanitizer, from a stand-alone program (tests/c/unpack_walk.cpp: its own
main, compiled with the sanitizer, linked against the device-free sanitizer objects of the library; nothing is preloaded
and no Python is in the process).  The program walks every accepted format and depth, every refusal with the line of the
reference its message names, and the forward transform's calls from packed bytes in a small, large, small order on two
queues (the routes counted, the queue's blocks grown and kept); a sanitizer report or a non-zero exit fails the test with
the text.  Leak detection is on."""
import os
import subprocess

import pytest

from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def test_the_unpack_host_code_under_asan_and_ubsan():
    if not clang_runtime("asan"):
        pytest.skip("no asan runtime in this image")
    make = subprocess.run(["make", "-C", CDIR, "-f", "unpack_walk.mk", "-j8", "-s", "unpack_walk_asan"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    # (the device-free build is an experiments build: every combination that allows it on the FUSED route, so that the
    # program's route counts do not depend on the measured table)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0",
               SCHRO_HIP_UNPACK_FUSED="1")
    env.pop("SCHRO_HIP_UNPACK_TWO_PASS", None)
    r = subprocess.run([os.path.join(CDIR, "_build", "unpack_walk_asan")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found and r.returncode == 0, text[-6000:]
    assert "unpack_walk: 37 accepted, 26 refusals, 72 transform calls, ok" in text
