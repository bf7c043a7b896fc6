"""GPU: the packed 8-bit level kernels of the filters that the product library sends to the two passes.

schro_hip_iiwt_pack_u8_batch keeps the two passes for the filters whose level route did not measure faster (include/schro_hip.h);
iiwt_pack8_kernel is built for every filter all the same.  The experiments library with SCHRO_HIP_PACK8_LEVEL=1 lets every
filter take it: tests/test_gpu_pack8_fused.py, run again in a child process with that switch, then expects the LEVEL route
for every filter and compares the same bytes."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so")


def test_every_filter_on_the_level_route():
    assert os.path.exists(EXP), "build the experiments library first (__graft_entry__.build ())"
    e = dict(os.environ, SCHRO_HIP_LIB=EXP, SCHRO_HIP_PACK8_LEVEL="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_pack8_fused.py")]
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
