"""CPU: every refusal of the five motion stages -- rough search, block matching, sub-pel refinement, split 2, mode decision
-- returns the code and the message, byte for byte, that tests/golden/motion_refusals.json records from the library as it
was before the stages shared one span check and one geometry check (tests/golden/make_motion_refusals.py).  The api tests
match substrings; this pins the wording and the order in which the refusals are tested."""
import json
import os
import re

import pytest

import motion_refusal_cases

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_refusals.json")))
CASES = motion_refusal_cases.cases()
STAGES = {"rough": ("rough_hint/", "rough_me/"), "hbm": ("hbm_level/", "hbm/"), "subpel": ("subpel/",), "split2": ("split2/",), "mode": ("mode/",)}


def test_the_fixture_and_the_cases_are_the_same_set():
    assert sorted(GOLDEN) == sorted(CASES)
    assert all(code == -1 and msg for code, msg in GOLDEN.values())     # SCHRO_HIP_EINVAL, with a message


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal_is_what_was_recorded(name):
    assert CASES[name]() == GOLDEN[name]


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_each_stage_has_every_kind_of_refusal(stage):
    msgs = [m for n, (code, m) in GOLDEN.items() if n.startswith(STAGES[stage])]
    assert any(re.search(r"\d+ x -?\d+ blocks|a block of", m) for m in msgs), "a geometry refusal"
    assert any("NULL pointer" in m or "aligned" in m for m in msgs), "a pointer or alignment refusal"
    # what is written against what is read, and against what another picture, entry or chain of the call writes
    written = r"the field|the motion field|the superblock table|the trial table|the statistics"
    read = r"a plane or hint field|the picture|the upsampled image|an upsampled image|the source field|a sub-pel field|a level-[12] field"
    assert any(re.search(r"(%s) overlaps (%s) of" % (written, read), m) or re.search(r"(%s) overlaps (%s) of" % (read, written), m) for m in msgs)
    two = [re.search(r"(?:picture|entry|chain) (\d+)(?: level \d+)?: (?:%s) overlaps (?:%s) of (?:picture|entry|chain) (\d+)" % (written, written), m)
           for m in msgs]
    assert any(t and t.group(1) != t.group(2) for t in two), "written over written across two owners"
