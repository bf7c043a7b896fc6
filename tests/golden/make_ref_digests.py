#!/usr/bin/env python3
"""Regenerates tests/golden/ref_kernel_digests.json.

For every case in which the oracle tests pin a formula on the REFERENCE's compiled kernels
(oracle/_ref/libschroorc_ref.so, libschro_refdrv.so: built by `make -C oracle` where the reference
sources are present), the digest of what those kernels computed (oracle_lib.digest: sha256 of dtype,
shape and bytes).  The tests compare against these digests on a box without oracle/_ref, and against
both the kernels and the digests where it is built.  Runs those tests with
SCHRO_REF_DIGESTS_RECORD=1 (oracle_lib.assert_reference then records instead of looking up).

Data only: digests of outputs, no reference source.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402

TESTS = ["test_oracle_wavelet.py", "test_oracle_frame.py", "test_oracle_motion.py", "test_oracle_pack.py",
         "test_oracle_lowdelay.py", "test_oracle_dequant.py"]


def main():
    O.build_oracle()
    if not O.ref_available():
        sys.exit("oracle/_ref is not built: the reference sources are needed to record its results")
    if os.path.exists(O.REF_DIGESTS):
        os.remove(O.REF_DIGESTS)
    subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:xdist", "-p", "no:cacheprovider"]
                   + [os.path.join(ROOT, "tests", t) for t in TESTS],
                   cwd=ROOT, env=dict(os.environ, SCHRO_REF_DIGESTS_RECORD="1"), check=True)
    print(O.REF_DIGESTS, os.path.getsize(O.REF_DIGESTS))


if __name__ == "__main__":
    main()
