"""Writes tests/golden/frame_refusals.json: the transcript of tests/c/frame_walk.cpp -- [call, status, last-error text] for
every accepted call and every refusal of the frame layer's transform-data entry points, in the order the source tests
them -- as the library that is built answers.  Recorded once from the commit in front of the one that put the transform
geometry, the fused-picture fill and the synchronous round trip of schroedinger_amd/csrc/frame.cpp in one place each
(that commit's sources in a scratch worktree, this program and its make target copied in); run it again only when a
refusal is meant to change.  Data only; needs no device.

    python tests/golden/make_frame_refusals.py
"""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CDIR = os.path.join(os.path.dirname(HERE), "c")
ENV = {"ASAN_OPTIONS": "detect_leaks=1:exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=0"}


def transcript():
    """(the calls as [name, status, text], everything the program printed)"""
    subprocess.run(["make", "-C", CDIR, "-j8", "-s", "frame_walk_asan"], check=True)
    r = subprocess.run([os.path.join(CDIR, "_build", "frame_walk_asan")], env=dict(os.environ, **ENV), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    return [line.split("\t") for line in text.splitlines()], text


def main():
    calls, _ = transcript()
    assert all(len(c) == 3 for c in calls), "a line that is not a call"
    path = os.path.join(HERE, "frame_refusals.json")
    with open(path, "w") as f:
        json.dump(calls, f, indent=0)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(calls), "calls")


if __name__ == "__main__":
    main()
