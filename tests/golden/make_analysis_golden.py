"""Writes tests/golden/analysis_ref.npz: what the reference's compiled kernels (oracle/_ref/libschroorc_ref.so:
orc_downsample_vert_u8, orc_downsample_horiz_u8, orc_sad_*) give for the cases of tests/analysis_ref.py, driven in the
reference's own row schedule (analysis_ref.downsample_orc, do_scan_orc).  Data only; needs oracle/_ref.

    python tests/golden/make_analysis_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import analysis_ref as A        # noqa: E402
import oracle_lib as O          # noqa: E402


def main():
    assert O.ref_available(), "build oracle/_ref first"
    out = {}
    for (w, h) in A.GOLDEN_SIZES:
        out["down_random_%dx%d" % (w, h)] = A.downsample_orc(A.picture(w, h, 100 + w + 7 * h))
        out["down_checker_%dx%d" % (w, h)] = A.downsample_orc(A.checkerboard(w, h))
    for n, (frame, ref, s, ext) in enumerate(A.golden_scans()):
        out["scan_%02d" % n] = A.do_scan_orc(frame, ref, s, ext)
    path = os.path.join(HERE, "analysis_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
