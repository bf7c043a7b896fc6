"""Writes tests/golden/motion_refusals.json: {case id: [return code, message]} for every refusal case of the five motion
stages (tests/motion_refusal_cases.py), as the library that is built answers them.  Recorded once from the commit in
front of the one that gave the stages one span check and one geometry check; run it again only when a refusal is meant
to change.  Data only; needs no device.

    python tests/golden/make_motion_refusals.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import motion_refusal_cases as cases    # noqa: E402


def main():
    out = {name: thunk() for name, thunk in cases.cases().items()}
    assert all(code != 0 and msg for code, msg in out.values()), "a case that is not refused"
    path = os.path.join(HERE, "motion_refusals.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "cases")


if __name__ == "__main__":
    main()
