"""CPU: the host code of the quantiser choice (plane_quant_choose.cpp) and of the two consumers that take their indices from
the device (schro_hip_quantise_chosen_batch, schro_hip_noarith_encode_chosen_batch and its check) under AddressSanitizer +
UndefinedBehaviorSanitizer, from a stand-alone program (tests/c/quant_choose_walk.cpp: its own main, compiled with the
sanitizer, linked against the device-free sanitizer objects of the library; nothing is preloaded and no Python is in the
process).  The program walks the tables' replacement, every refusal of the check, batches of one, nine and one unlike
pictures on two queues (the scratch small, large, small) and the consumers' tables and refusals; a sanitizer report or a
non-zero exit fails the test with the text.  Leak detection is on."""
import os
import subprocess

import pytest

from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def test_the_quantiser_choice_host_code_under_asan_and_ubsan():
    if not clang_runtime("asan"):
        pytest.skip("no asan runtime in this image")
    make = subprocess.run(["make", "-C", CDIR, "-f", "quant_choose_walk.mk", "-j8", "-s", "quant_choose_walk_asan"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([os.path.join(CDIR, "_build", "quant_choose_walk_asan")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found and r.returncode == 0, text[-6000:]
    assert "quant_choose_walk: 12 refusals, 6 batches, the chosen consumers, ok" in text
