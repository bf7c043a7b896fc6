"""CPU: the encoder-side host code -- plane_analysis, plane_rough, plane_iwt, plane_quant, plane_hist, plane_lowdelay_enc and
the encoder half of frame.cpp -- under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer, from a
stand-alone program (tests/c/encoder_walk.cpp: its own main, compiled with the sanitizer, linked against the device-free
sanitizer objects of the library; nothing is preloaded and no Python is in the process).

tests/encoder_walk_cases.py writes the program's case file from the case modules the device tests share; this file
asserts that the file is not vacuous -- every entry point, every class of geometry, every refusal -- builds the program
(make -C tests/c encoder_walk_asan / encoder_walk_tsan) and runs it as a child.  A sanitizer report or a non-zero exit
fails the test with the text.  Leak detection is on: a leak in the library's close path is the library's.

Build and walk take seconds (about two minutes where the device-free library has to be built first) and run under the
suite's own per-test limit.  Both runs walk the whole file: no draw is thinned out (encoder_walk_cases.build (k) can keep every k-th random draw should
the ThreadSanitizer walk -- three threads at once beside a scheduler -- ever become the long one).  Wall times: DESIGN.md,
"The encoder's host code under the sanitizers"."""
import os
import re
import subprocess

import pytest

import encoder_walk_cases as W
import hist_cases as HC
import lowdelay_enc_cases as LK
import quant_cases as QC
import rough_hint_cases as RK
from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")
TSAN_THIN = 1                   # every draw


def assert_not_vacuous(lines, classes):
    calls = {line.split()[0] for line in lines}
    assert calls == set(W.ENTRY_POINTS), set(W.ENTRY_POINTS) ^ calls
    for name in W.CLASSES:
        assert classes[name] >= 1, name
    # the thresholds are the case modules': both spill cases and the three-picture batch leave LDS, the rough cases hold
    # the largest block at the largest distance, a padded stride, odd block counts
    assert all(LK.leaves_lds(LK.CASES[n][0]) for n in ("spill_2x2", "spill_3x5_420", LK.SPILL_BATCH[0])) and len(LK.SPILL_BATCH[1]) >= 3
    assert classes["spill"] >= 3
    big = RK.CASES["block_64x64_distance_20"]
    assert (big["xb"], big["yb"], big["dist"]) == (W.MAX_BLOCK, W.MAX_BLOCK, W.MAX_DISTANCE)
    assert RK.CASES["padded_strides"]["pad"] > 0 and RK.CASES["shift3_odd"]["nbx"] % 2 == RK.CASES["shift3_odd"]["nby"] % 2 == 1
    for name in ("long_diagonal", "one_block", "beyond_the_picture"):
        assert name in RK.CASES
    # every refusal status these calls return, and the refusals by call
    refused = {"rough_hint": len(RK.REFUSED_MEMBERS) + len(RK.REFUSED_ALIASES), "quantise": len(QC.refusal_table(64)[1]),
               "histogram": len(HC.refusal_table(64)[1]), "lowdelay_encode": 1 + len(LK.refused_params(LK.CASES[LK.REFUSED_CASE][0]))}
    for call, n in refused.items():     # (every refusal of the module's table is a line of the file)
        assert classes["refused_" + call] == n, (call, classes["refused_" + call], n)
    assert classes["status_%d" % W.EINVAL] >= sum(refused.values()) and classes["status_%d" % W.EUNSUPPORTED] >= 1
    for word in ("chroma_LL", "LL_bands", "LL_rectangles"):
        assert classes["refused_" + word] >= 1, word
    for call in W.ENTRY_POINTS:
        if call not in ("downsample", "metric_scan"):       # (their refusals are tests/dry_run_analysis_cases.py's)
            assert classes["refused_" + call] >= 1, call


def test_the_case_file_is_not_vacuous():
    full, thin = W.build(), W.build(3)
    assert_not_vacuous(*full)
    assert_not_vacuous(*thin)           # (thinning drops draws, never a named case, a refusal or the spill path)
    assert len(thin[0]) < len(full[0])


def run_walk(tmp_path, sanitizer, runtime, thin, env, limit):
    if not clang_runtime(runtime):
        pytest.skip("no %s runtime in this image" % runtime)
    lines, classes = W.build(thin)
    assert_not_vacuous(lines, classes)
    cases = tmp_path / "encoder_walk_cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    make = subprocess.run(["make", "-C", CDIR, "-j8", "-s", "encoder_walk_" + sanitizer], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    env = dict(os.environ, **env)
    r = subprocess.run([os.path.join(CDIR, "_build", "encoder_walk_" + sanitizer), sanitizer, str(cases)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=limit)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found, "sanitizer report:\n" + text[max(0, found.start() - 400):found.start() + 4000]
    assert r.returncode == 0, text[-4000:]
    assert re.search(r"encoder_walk %s: %d lines, ok" % (sanitizer, len(lines)), text), text[-2000:]


def test_encoder_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    run_walk(tmp_path, "asan", "asan", 1, {"ASAN_OPTIONS": "detect_leaks=1:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=0"},
             limit=300)


def test_encoder_host_code_under_thread_sanitizer(tmp_path):
    run_walk(tmp_path, "tsan", "tsan", TSAN_THIN, {"TSAN_OPTIONS": "exitcode=66:halt_on_error=0"}, limit=300)
