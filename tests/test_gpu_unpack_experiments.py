"""GPU: the packed level 0 of the forward wavelet for the combinations that the product library sends to the two passes,
and the two passes of those it sends to the packed level 0.

schro_hip_unpack_iwt_batch takes FUSED only for the format x filter x sample type combinations that did not measure slower
than the chain (include/schro_hip.h, unpack_fused_combination in plane_unpack.cpp); iwt_fwd_packed_kernel is built for every
combination all the same.  The experiments library with SCHRO_HIP_UNPACK_FUSED=1 lets every combination take it, with
SCHRO_HIP_UNPACK_TWO_PASS=1 none: tests/test_gpu_unpack_iwt.py, run again in a fresh child process with each switch, then
expects that route for every picture that allows it and compares the same coefficients."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so")


def rerun(switch):
    assert os.path.exists(EXP), "build the experiments library first (__graft_entry__.build ())"
    e = dict(os.environ, SCHRO_HIP_LIB=EXP)
    e.pop("SCHRO_HIP_UNPACK_FUSED", None)
    e.pop("SCHRO_HIP_UNPACK_TWO_PASS", None)
    e[switch] = "1"
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_unpack_iwt.py")]
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]


def test_every_combination_on_the_fused_route():
    rerun("SCHRO_HIP_UNPACK_FUSED")


def test_every_picture_on_the_two_passes():
    rerun("SCHRO_HIP_UNPACK_TWO_PASS")
