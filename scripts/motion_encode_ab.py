#!/usr/bin/env python3
"""First numbers for the motion-data encoder of noarith pictures (motion_enc.hip) beside what it replaces.

8 x 2160p pictures with two references per call, at 16-pixel block separation (240 x 136 blocks: 135 rows rounded up to
whole superblocks) and at 8-pixel separation (480 x 272).  The fields are seeded fields that look like a search result
(tests/motion_enc_cases.py search_like: smooth vectors, a few DC blocks, mixed splits) and satisfy schro_motion_verify.

In the same run, on the same fields:

  schro_hip_motion_encode_batch      the whole call (count, layout, clear, pack);
  its launches one at a time         (experiments library only: SCHRO_HIP_MOTENC_STAGES = 1 count, 2 layout, 4 clear, 8 pack;
                                     each runs on the tables the full call before it left);
  the device-to-host copy            of the eight fields into pinned memory: what the host's nine passes need today.

Before anything is timed the bytes of picture 0 are held against the restatement (tests/motion_enc_ref.py) and every
picture's result must report no assert and no unverified block.  Times: device events around `steps` calls
(Context.timer_begin / timer_end), per call; the median of `rounds` rounds after `warmup` calls, and the spread
(max - min) / median.  NOT shown: the host's nine passes and its packer, which are not built here; the copy is only the part
of today's path that this call makes unnecessary, the stream bytes still have to reach the host.

  SCHRO_HIP_LIB=schroedinger_amd/libschro_hip_exp.so python scripts/motion_encode_ab.py [--out profiles/motion_encode.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import motion_enc_cases as MC           # noqa: E402
import motion_enc_ref as ref            # noqa: E402
import schroedinger_amd as sa           # noqa: E402
from schroedinger_amd import _lib       # noqa: E402

NPIC, W, H, NUM_REFS = 8, 3840, 2160, 2


def timed(ctx, fn, a):
    rows = []
    for _ in range(a.rounds):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.timer_begin()
        for _ in range(a.steps):
            fn()
        rows.append(ctx.timer_end() / a.steps)
    med = statistics.median(rows)
    return med, (max(rows) - min(rows)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    experiments = "exp" in os.path.basename(_lib.LIB_PATH)
    lines = ["motion_encode_ab: %d x %dx%d pictures, %d references, no global motion, per call%s"
             % (NPIC, W, H, NUM_REFS, ", experiments library" if experiments else "")]
    words = C.sizeof(_lib.MotionEncodeResult) // 4
    for sep in (16, 8):
        nbx, nby = (W + sep - 1) // sep, (H + sep - 1) // sep
        nbx, nby = (nbx + 3) // 4 * 4, (nby + 3) // 4 * 4
        host = [MC.search_like(40 + p, nbx, nby, NUM_REFS) for p in range(2)]
        fields = [ctx.upload_bytes(host[p % 2]) for p in range(NPIC)]
        bound = sa.motion_encode_bound(nbx, nby, NUM_REFS, 0)
        outs = [ctx.plane(1, bound, np.uint8) for _ in range(NPIC)]
        ress = [ctx.plane(1, words, np.uint32) for _ in range(NPIC)]
        pinned = [ctx.host_array((1, host[0].nbytes), np.uint8) for _ in range(NPIC)]
        pics = [(fields[p], nbx, nby, NUM_REFS, 0, outs[p], bound, ress[p]) for p in range(NPIC)]
        field_mb = NPIC * host[0].nbytes / 1e6

        def encode():
            ctx.motion_encode_batch(pics)

        def copy_back():
            for p in range(NPIC):
                fields[p].download_async(pinned[p])

        encode()
        ctx.synchronize()
        results = [sa.motion_encode_result(r.download()) for r in ress]
        want, want_result = ref.encode(host[0], nbx, nby, NUM_REFS, 0)
        got = bytes(outs[0].download()[0, :results[0]["bytes"]])
        assert got == want and results[0]["section_bytes"] == want_result["section_bytes"], "picture 0 is not the restatement's"
        assert all(r["overrun"] == 0 and r["asserted"] == 0 and r["unverified"] == 0 for r in results)
        nbytes = sum(r["bytes"] for r in results)
        lines.append("%d-pixel separation: %d x %d blocks, %.2f MB of records and %.3f MB of stream for the call (%.1f bits per block); "
                     "capacity per picture %.2f MB; picture 0 checked against the restatement"
                     % (sep, nbx, nby, field_mb, nbytes / 1e6, 8.0 * nbytes / (NPIC * nbx * nby), bound / 1e6))
        t, spread = timed(ctx, encode, a)
        lines.append("  encode     %8.4f ms per call, %8.4f ms per picture, spread %.1f %%" % (t, t / NPIC, 100 * spread))
        if experiments:
            for bit, name in ((1, "count"), (2, "layout"), (4, "clear"), (8, "pack")):
                os.environ["SCHRO_HIP_MOTENC_STAGES"] = str(bit)
                ts, spread = timed(ctx, encode, a)
                lines.append("  launch %-10s %8.4f ms per call, spread %.1f %%" % (name, ts, 100 * spread))
            os.environ.pop("SCHRO_HIP_MOTENC_STAGES", None)
        tc, spread = timed(ctx, copy_back, a)
        lines.append("  copy back  %8.4f ms per call for the eight fields (%.1f GB/s), spread %.1f %%" % (tc, field_mb / tc, 100 * spread))
        lines.append("  ratio copy back / encode %.2f" % (tc / t))
        for p in fields + outs + ress:
            p.free()
    lines.append("not shown: the host's nine passes and its packer (not built here); the stream bytes still have to be copied to the host")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
