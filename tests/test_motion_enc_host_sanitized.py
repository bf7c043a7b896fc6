"""CPU: the host code of the motion-data encoder -- plane_motion_enc.cpp and the frame layer's entry -- under
AddressSanitizer + UndefinedBehaviorSanitizer, from a stand-alone program (tests/c/motion_enc_walk.cpp: its own main,
compiled with the sanitizer, linked against the device-free sanitizer objects of the library; nothing is preloaded and no
Python is in the process).  The program walks the case module's geometries and the refusal table; a sanitizer report or
a non-zero exit fails the test with the text.  Leak detection is on."""
import os
import subprocess

import pytest

import motion_enc_cases as MC
from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")
KEYS = ("motion", "nbx", "nby", "num_refs", "hg", "out", "capacity", "result")


def geometries():
    return sorted({c[2:6] for c in MC.all_cases()})


def table_lines():
    out = ["G %dx%d-r%d-g%d %d %d %d %d" % (g + g) for g in geometries()]
    for refused, table in ((1, MC.REFUSALS), (0, [(n, c, "") for n, c in MC.ACCEPTED])):
        for name, change, message in table:
            d = MC.describe()
            change(d)
            out.append("D %s %d %d" % (name.replace(" ", "_"), refused, len(d)))
            out += ["p " + " ".join(str(int(p[k])) for k in KEYS) for p in d]
            out.append("M " + (message or "-"))
    return out


def test_the_motion_encoder_host_code_under_asan_and_ubsan(tmp_path):
    if not clang_runtime("asan"):
        pytest.skip("no asan runtime in this image")
    make = subprocess.run(["make", "-C", CDIR, "-f", "motion_enc_walk.mk", "-j8", "-s", "motion_enc_walk_asan"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    table = tmp_path / "motion_enc_walk.txt"
    table.write_text("\n".join(table_lines()) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([os.path.join(CDIR, "_build", "motion_enc_walk_asan"), str(table)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found and r.returncode == 0, text[-6000:]
    assert "motion_enc_walk: %d geometries, %d descriptions, ok" % (len(geometries()), len(MC.REFUSALS) + len(MC.ACCEPTED)) in text
