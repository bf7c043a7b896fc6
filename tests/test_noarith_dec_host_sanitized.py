"""CPU: the host code of the noarith transform-data decoder -- plane_noarith_dec.cpp and the frame layer's entry -- under
AddressSanitizer + UndefinedBehaviorSanitizer, from a stand-alone program (tests/c/noarith_dec_walk.cpp: its own main,
compiled with the sanitizer, linked against the device-free sanitizer objects of the library; nothing is preloaded and no
Python is in the process).  The program walks the case module's geometries with the scratch formula and the refusal
table; a sanitizer report or a non-zero exit fails the test with the text.  Leak detection is on."""
import os
import subprocess

import pytest

import noarith_dec_cases as DC
import noarith_dec_draws as DD
from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


# ---- the table tests/c/noarith_dec_walk.cpp reads ----------------------------------------------------------------------

def _shape(bpp, depth, mode, sizes, hc, vc):
    pad = lambda v: list(v)[:7] + [1] * (7 - len(v))
    return [bpp, depth, mode] + [v for s in sizes for v in s] + pad(hc) + pad(vc)


def scratch_words(case):
    """5 words per chunk slot (data_bytes / 8 + sub-bands + 1), 3 per codeblock, 8 per sub-band, 2 per picture."""
    nsb = 3 * case.nsub
    ncb = 3 * sum(case.counts(i)[0] * case.counts(i)[1] for i in range(case.nsub))
    return 5 * (case.data_bytes // 8 + nsb + 1) + 3 * ncb + 8 * nsb + 2


# the named cases, and the drawn and scale ones: depths to 6, sizes the transform rounds up, inputs cut short
GEOMETRIES = DC.CASES + DC.HOSTILE + DD.DRAWS + DD.SCALE


def table_lines():
    out = []
    for case in GEOMETRIES:
        row = ["G", case.name] + _shape(case.dtype.itemsize, case.depth, case.mode, case.sizes, case.hc, case.vc)
        out.append(" ".join(str(v) for v in row + [case.data_bytes, scratch_words(case)]))
    for refused, table in ((1, DC.REFUSALS), (0, [(n, c, "") for n, c in DC.ACCEPTED])):
        for name, change, message in table:
            d = DC.describe()
            change(d)
            row = ["D", name, refused] + _shape(d["bpp"], d["depth"], d["mode"], d["sizes"], d["hc"], d["vc"])
            row += d["stride"] + d["bytes"] + d["coeffs"] + (d["quant"] or [0, 0, 0])
            row += [d["data"], d["data_bytes"], d["bytes_on_device"], d["result"]]
            out.append(" ".join(str(v) for v in row))
            out.append("M " + (message or "-"))
    return out


def test_the_noarith_decoder_host_code_under_asan_and_ubsan(tmp_path):
    if not clang_runtime("asan"):
        pytest.skip("no asan runtime in this image")
    make = subprocess.run(["make", "-C", CDIR, "-f", "noarith_dec_walk.mk", "-j8", "-s", "noarith_dec_walk_asan"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    table = tmp_path / "noarith_dec_walk.txt"
    table.write_text("\n".join(table_lines()) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([os.path.join(CDIR, "_build", "noarith_dec_walk_asan"), str(table)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found and r.returncode == 0, text[-6000:]
    assert "noarith_dec_walk: %d geometries, %d descriptions, ok" % (len(GEOMETRIES), len(DC.REFUSALS) + len(DC.ACCEPTED)) in text
