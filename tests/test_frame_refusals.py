"""CPU: the frame layer's transform-data entry points (schroedinger_amd/csrc/frame.cpp) answer every accepted call and every
refusal of tests/c/frame_walk.cpp with the status and the message, byte for byte and in the order, that
tests/golden/frame_refusals.json records from the library as it was before those entry points shared one transform
geometry, one fused-picture fill and one synchronous round trip (tests/golden/make_frame_refusals.py).

The program is a stand-alone one (its own main, compiled with AddressSanitizer + UndefinedBehaviorSanitizer, linked against
the device-free sanitizer objects of the library; nothing is preloaded and no Python is in the process), so the same run
shows that the calls, their refusal paths and the contexts' close path leave no report and no leak."""
import json
import os
import sys

import pytest

from test_sanitizers import REPORT

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_frame_refusals as M    # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "frame_refusals.json")))
# the entry points that stand on the shared pieces, by the prefix of their calls' names
ENTRY_POINTS = {
    "schro_hipframe_iwt_transform": ("iwt_transform/",),
    "schro_frame_inverse_iwt_transform_hip / _combine_hip": ("inverse_iwt/",),
    "schro_frame_inverse_iwt_transform_combine_convert_hip: YUYV / UYVY / AYUV": ("convert_yuyv/",),
    "schro_frame_inverse_iwt_transform_combine_convert_hip: v216 / ARGB / AY64": ("convert_v216/",),
    "schro_frame_inverse_iwt_transform_combine_convert_hip: v210": ("convert_v210/",),
    "schro_hip_decode_lowdelay_transform_data": ("decode_lowdelay/",),
    "schro_hip_encode_lowdelay_transform_data": ("encode_lowdelay/",),
    "schro_hip_encode_transform_data_noarith": ("encode_noarith/",),
    "schro_hipframe_decode_transform_data_noarith": ("decode_noarith/",),
    "schro_hip_encode_motion_data_noarith": ("encode_motion/",),
    "schro_hip_decode_motion_data_noarith": ("decode_motion/",),
    "schro_hipframe_dequantise": ("dequantise/",),
    "schro_hipframe_add": ("add/",),
    "schro_hipframe_subtract": ("subtract/",),
    "schro_hipframe_quantise": ("quantise/",),
    "schro_hipframe_subband_histograms": ("histograms/",),
}


@pytest.fixture(scope="module")
def walk():
    return M.transcript()


def test_the_build_at_hand_prints_the_recorded_transcript(walk):
    calls, text = walk
    want = "".join("\t".join(c) + "\n" for c in GOLDEN)
    got = "".join("\t".join(c) + "\n" for c in calls)
    assert got == want, next(((a, b) for a, b in zip(calls, GOLDEN) if a != b), (len(calls), len(GOLDEN)))
    assert text == want         # (nothing else on either stream)


def test_the_walk_leaves_no_sanitizer_report(walk):
    found = REPORT.search(walk[1])      # (leak detection is on and the exit status was 0: make_frame_refusals.ENV)
    assert not found, "sanitizer report:\n" + walk[1][max(0, found.start() - 400):found.start() + 4000]
    assert "detect_leaks=1" in M.ENV["ASAN_OPTIONS"]


@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_every_entry_point_is_accepted_once_and_refused_once(entry):
    mine = [c for c in GOLDEN if c[0].startswith(ENTRY_POINTS[entry])]
    assert any(c[1] in ("0", "passed") for c in mine), "no accepted call"
    # a refusal of the entry point's own: SCHRO_HIP_EINVAL with a message
    assert any(c[1] == "-1" and c[2] for c in mine), "no refusal"
