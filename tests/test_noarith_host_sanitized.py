"""CPU: the host code of the noarith transform-data encoder -- plane_noarith_enc.cpp and the frame layer's entry -- under
AddressSanitizer + UndefinedBehaviorSanitizer, from a stand-alone program (tests/c/noarith_walk.cpp: its own main,
compiled with the sanitizer, linked against the device-free sanitizer objects of the library; nothing is preloaded and no
Python is in the process).  The program walks the case module's geometries, the random draws and the refusal table; a
sanitizer report or a non-zero exit fails the test with the text.  Leak detection is on."""
import os
import subprocess

import pytest

import noarith_enc_cases as NC
import noarith_enc_draws as ND
from test_sanitizers import REPORT, clang_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


# ---- the table tests/c/noarith_walk.cpp reads --------------------------------------------------------------------------

def _shape(bpp, depth, mode, sizes, hc, vc):
    pad = lambda v: list(v) + [1] * (7 - len(v))
    return [bpp, depth, mode] + [v for s in sizes for v in s] + pad(hc) + pad(vc)


def table_lines():
    out = []
    for case in NC.CASES + ND.DRAWS:
        out.append(" ".join(["G", case.name] + [str(v) for v in _shape(case.dtype.itemsize, case.depth, case.mode, case.sizes, case.hc, case.vc)]))
    for refused, table in ((1, NC.REFUSALS), (0, [(n, c, "") for n, c in NC.ACCEPTED])):
        for name, change, message in table:
            d = NC.describe()
            change(d)
            row = ["D", name, refused] + _shape(d["bpp"], d["depth"], d["mode"], d["sizes"], d["hc"], d["vc"])
            row += d["stride"] + d["bytes"] + d["quant"] + [d["out"], d["capacity"], d["result"]] + [len(r) for r in d["records"]]
            out.append(" ".join(str(v) for v in row))
            for recs in d["records"]:
                out += ["r %d %d %d %d %d" % (r[0], r[1], r[2], r[3], r[6]) for r in recs]
            out.append("M " + (message or "-"))
    return out


def test_the_noarith_encoder_host_code_under_asan_and_ubsan(tmp_path):
    if not clang_runtime("asan"):
        pytest.skip("no asan runtime in this image")
    make = subprocess.run(["make", "-C", CDIR, "-f", "noarith_walk.mk", "-j8", "-s", "noarith_walk_asan"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT)
    assert make.returncode == 0, make.stdout.decode(errors="replace")[-4000:]
    table = tmp_path / "noarith_walk.txt"
    table.write_text("\n".join(table_lines()) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([os.path.join(CDIR, "_build", "noarith_walk_asan"), str(table)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    found = REPORT.search(text)
    assert not found and r.returncode == 0, text[-6000:]
    assert "noarith_walk: %d geometries, %d descriptions, ok" % (len(NC.CASES) + len(ND.DRAWS), len(NC.REFUSALS) + len(NC.ACCEPTED)) in text
