"""CPU: schro_hip_quant_choose_check refuses, before any launch and without a context, what
schro_hip_quant_choose_batch refuses, and names the picture and the field; the numpy record and the ctypes struct of
SchroHipQuantChoice agree with the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import schroedinger_amd as sa
from schroedinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def good(depth=2):
    nb = 1 + 3 * depth
    return dict(counts=[0x1000, 0x2000, 0x3000], skip=[1] * nb, depth=depth, is_intra=1, is_noarith=1, engine=sa.QUANT_ENGINE_BIT_ALLOCATION,
                weight=[1.5] * nb, ratio=[[1.0] * nb] * 3, scales=(10.0, 0.1, 0.5), target=4000.0, result=0x4000)


def test_a_good_batch_passes():
    sa.quant_choose_check([good(0), good(6), dict(good(3), is_noarith=0)])
    sa.quant_choose_check([good()], have_bit_tables=False)


@pytest.mark.parametrize("change,message", [
    (dict(depth=7, skip=[1] * 19, weight=[1.0] * 19, ratio=[[1.0] * 19] * 3), r"picture 1: a transform_depth of 7"),
    (dict(depth=-1), r"picture 1: a transform_depth of -1"),
    (dict(skip=[1, 2, 3, 1, 1, 1, 1]), r"picture 1: skip\[2\] is 3 \(a power of two"),
    (dict(skip=[1, 0, 1, 1, 1, 1, 1]), r"picture 1: skip\[1\] is 0"),
    (dict(skip=[1, 1, 1, 1, 1, 1, 2048]), r"picture 1: skip\[6\] is 2048"),
    (dict(weight=[1, 1, 1, 0.0, 1, 1, 1]), r"picture 1: subband_weight\[3\] is 0 "),
    (dict(weight=[1, 1, 1, 1, -2.0, 1, 1]), r"picture 1: subband_weight\[4\] is -2 "),
    (dict(weight=[float("inf")] + [1] * 6), r"picture 1: subband_weight\[0\] is inf"),
    (dict(weight=[1] * 6 + [float("nan")]), r"picture 1: subband_weight\[6\] is nan"),
    (dict(ratio=[[1.0] * 7, [1.0] * 5 + [float("nan"), 1.0], [1.0] * 7]), r"picture 1: context_ratio\[1\]\[5\] is nan"),
    (dict(scales=(float("inf"), 1, 1)), r"picture 1: subband0_lambda_scale is inf"),
    (dict(scales=(1, float("nan"), 1)), r"picture 1: chroma_lambda_scale is nan"),
    (dict(scales=(1, 1, float("-inf"))), r"picture 1: diagonal_lambda_scale is -inf"),
    (dict(target=float("nan")), r"picture 1: target is nan"),
    (dict(target=float("inf")), r"picture 1: target is inf"),
    (dict(engine=3), r"picture 1: engine 3 is unknown"),
    (dict(engine=-1), r"picture 1: engine -1 is unknown"),
    (dict(is_noarith=2), r"picture 1: is_intra 1, is_noarith 2"),
    (dict(counts=[0x1000, None, 0x3000]), r"picture 1: counts\[1\] is NULL"),
    (dict(counts=[0x1000, 0x2000, 0x3002]), r"picture 1: counts\[2\] is NULL or not 4-byte aligned"),
    (dict(result=None), r"picture 1: result is NULL"),
    (dict(result=0x4004), r"picture 1: result is NULL or not 8-byte aligned"),
    (dict(est_error=0x5004), r"picture 1: est_entropy / est_error not 8-byte aligned"),
])
def test_refusals(change, message):
    with pytest.raises(sa.SchroHipError, match=message):
        sa.quant_choose_check([good(), dict(good(), **change)])


def test_arith_form_without_bit_tables():
    with pytest.raises(sa.SchroHipError, match=r"picture 2: is_noarith 0 needs the one-bits and zero-bits tables"):
        sa.quant_choose_check([good(), good(), dict(good(), is_noarith=0)], have_bit_tables=False)


def test_entries_past_the_depth_are_not_looked_at():
    p = good(1)
    p["skip"] = [1, 1, 1, 1] + [3] * 15
    p["weight"] = [1.0] * 4 + [float("nan")] * 15
    sa.quant_choose_check([p])


def test_no_pictures():
    with pytest.raises(sa.SchroHipError, match="bad arguments"):
        sa.quant_choose_check([])


def test_choice_record_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "schro_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(SchroHipQuantChoice), offsetof(SchroHipQuantChoice, sum),
         offsetof(SchroHipQuantChoice, chosen_entropy), offsetof(SchroHipQuantChoice, chosen_error),
         offsetof(SchroHipQuantChoice, quant_index), offsetof(SchroHipQuantChoice, evaluations),
         offsetof(SchroHipQuantChoice, not_bracketed), sizeof(SchroHipQuantChoosePicture),
         offsetof(SchroHipQuantChoosePicture, subband_weight), offsetof(SchroHipQuantChoosePicture, target),
         offsetof(SchroHipQuantChoosePicture, est_error));
  return 0;
}''')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    f = sa.QUANT_CHOICE_DTYPE.fields
    assert got[:7] == [sa.QUANT_CHOICE_DTYPE.itemsize] + [f[n][1] for n in ("sum", "chosen_entropy", "chosen_error", "quant_index",
                                                                           "evaluations", "not_bracketed")]
    Q, P = _lib.QuantChoice, _lib.QuantChoosePicture
    assert got[:7] == [C.sizeof(Q), Q.sum.offset, Q.chosen_entropy.offset, Q.chosen_error.offset, Q.quant_index.offset,
                       Q.evaluations.offset, Q.not_bracketed.offset]
    assert got[7:] == [C.sizeof(P), P.subband_weight.offset, P.target.offset, P.est_error.offset]
    assert (sa.QUANT_ENGINE_LAMBDA, sa.QUANT_ENGINE_BIT_ALLOCATION, sa.QUANT_ENGINE_CONSTANT_ERROR) == (0, 1, 2)
    assert np.zeros(1, sa.QUANT_CHOICE_DTYPE)["quant_index"].shape == (1, 3, 19)
