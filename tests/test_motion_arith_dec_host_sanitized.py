"""CPU: the host code of the arithmetic motion-data decoder -- plane_motion_arith_dec.cpp and the frame layer's entry -- under
AddressSanitizer + UndefinedBehaviorSanitizer, from a stand-alone program (tests/c/motion_arith_dec_walk.cpp: its own main,
compiled with the sanitizer, linked against the device-free sanitizer objects of the library; nothing is preloaded and no
Python is in the process).  The program walks the refusal and accepted tables, every geometry of the case list and the
scratch formula against the hand count; a sanitizer report or a non-zero exit fails the test with the text.  Leak
detection is on."""
import os
import subprocess

import pytest

import motion_arith_dec_cases as DC
from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")
KEYS = ("data", "data_bytes", "word", "nbx", "nby", "num_refs", "hg", "motion", "result")


def geometries():
    """Every geometry of the case list, with the length of its longest stream."""
    longest = {}
    for c in DC.all_cases()[0] + DC.all_cases()[1] + DC.all_cases()[2]:
        longest[c[2:6]] = max(longest.get(c[2:6], 0), len(c[1]))
    return sorted(g + (n,) for g, n in longest.items())


def table_lines():
    out = []
    for nbx, nby, num_refs, hg, n in geometries():
        words = DC.scratch_words([dict(nbx=nbx, nby=nby, data_bytes=n)])
        out.append("G %dx%d-r%d-g%d %d %d %d %d %d %d" % (nbx, nby, num_refs, hg, nbx, nby, num_refs, hg, n, words))
    for refused, table in ((1, DC.REFUSALS), (0, [(n, c, "") for n, c in DC.ACCEPTED])):
        for name, change, message in table:
            d = DC.describe_picture()
            change(d)
            out.append("D %s %d %d %d" % (name.replace(" ", "_"), refused, len(d), 0 if refused else DC.scratch_words(d)))
            out += ["p " + " ".join(str(int(p[k] or 0)) for k in KEYS) for p in d]
            out.append("M " + (message or "-"))
    return out


def test_the_arithmetic_motion_decoder_host_code_under_asan_and_ubsan(tmp_path):
    if not clang_runtime("asan"):
        pytest.skip("no asan runtime in this image")
    make = subprocess.run(["make", "-C", CDIR, "-f", "motion_arith_dec_walk.mk", "-j8", "-s", "motion_arith_dec_walk_asan"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    table = tmp_path / "motion_arith_dec_walk.txt"
    table.write_text("\n".join(table_lines()) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([os.path.join(CDIR, "_build", "motion_arith_dec_walk_asan"), str(table)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found and r.returncode == 0, text[-6000:]
    assert len(geometries()) >= 20
    assert "motion_arith_dec_walk: %d geometries, %d descriptions, ok" % (len(geometries()), len(DC.REFUSALS) + len(DC.ACCEPTED)) in text
