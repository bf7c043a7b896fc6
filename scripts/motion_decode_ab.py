#!/usr/bin/env python3
"""First numbers for the motion-data decoder of noarith pictures (motion_dec.hip) beside what it replaces.

The workload of scripts/motion_encode_ab.py: 8 x 2160p pictures with two references per call, at 16-pixel block separation
(240 x 136 blocks) and at 8-pixel separation (480 x 272), seeded fields that look like a search result
(tests/motion_enc_cases.py search_like).  The streams come from schro_hip_motion_encode_batch on those fields, and every
decoded field is held against motion_enc_ref.canonical of its source before anything is timed.

In the same run, on the same fields:

  schro_hip_motion_decode_batch      the whole call;
  its launches one at a time         (experiments library only: SCHRO_HIP_MOTDEC_STAGES = 1 header, 2 summary, 4 scan, 8
                                     extract, 16 split walk, 32 mode walk, 64 value walk; each runs on the tables the full
                                     call before it left), with the walks' time per diagonal;
  the host-to-device copy            of the eight fields from pinned memory: the parent's hand-over, what this call replaces;
  schro_hip_motion_encode_batch      on the same fields;
  the serial mode walk               one call of 8 pictures WITH global motion at 16-pixel separation (a drawn field, a
                                     third of the inter units global), whole call and mode walk alone.

Times: device events around `steps` calls (Context.timer_begin / timer_end), per call; the median of `rounds` rounds after
`warmup` calls, and the spread (max - min) / median.  NOT shown: the host's serial parse of the motion data, which this call
saves -- that parser is not built here and is unmeasured.

  SCHRO_HIP_LIB=schroedinger_amd/libschro_hip_exp.so python scripts/motion_decode_ab.py [--out profiles/motion_decode.txt]"""
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
STAGES = ((1, "header"), (2, "summary"), (4, "scan"), (8, "extract"), (16, "split walk"), (32, "mode walk"), (64, "value walk"))


def timed(ctx, fn, a, steps=None):
    rows, steps = [], steps or a.steps
    for _ in range(a.rounds):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.timer_begin()
        for _ in range(steps):
            fn()
        rows.append(ctx.timer_end() / steps)
    med = statistics.median(rows)
    return med, (max(rows) - min(rows)) / med


def geometry(sep):
    nbx, nby = (W + sep - 1) // sep, (H + sep - 1) // sep
    return (nbx + 3) // 4 * 4, (nby + 3) // 4 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    experiments = "exp" in os.path.basename(_lib.LIB_PATH)
    lines = ["motion_decode_ab: %d x %dx%d pictures, %d references, per call%s"
             % (NPIC, W, H, NUM_REFS, ", experiments library" if experiments else "")]
    ewords, dwords = C.sizeof(_lib.MotionEncodeResult) // 4, C.sizeof(_lib.MotionDecodeResult) // 4
    for sep, hg in ((16, 0), (8, 0), (16, 1)):
        nbx, nby = geometry(sep)
        if hg:
            host = [MC.draw(60 + p, nbx, nby, NUM_REFS, 1, modes=(1,) * 12 + (0,) + (3,) * 6 + (2,) * 3, smooth=True) for p in range(2)]
        else:
            host = [MC.search_like(40 + p, nbx, nby, NUM_REFS) for p in range(2)]
        canonical = [ref.canonical(h).tobytes() for h in host]
        fields = [ctx.upload_bytes(host[p % 2]) for p in range(NPIC)]
        bound = sa.motion_encode_bound(nbx, nby, NUM_REFS, hg)
        outs = [ctx.plane(1, bound, np.uint8) for _ in range(NPIC)]
        eress = [ctx.plane(1, ewords, np.uint32) for _ in range(NPIC)]
        decoded = [ctx.plane(1, host[0].nbytes, np.uint8) for _ in range(NPIC)]
        dress = [ctx.plane(1, dwords, np.uint32) for _ in range(NPIC)]
        pinned = [ctx.host_array((1, host[0].nbytes), np.uint8) for _ in range(NPIC)]
        for p in range(NPIC):
            pinned[p][:] = host[p % 2].view(np.uint8).reshape(1, -1)
        epics = [(fields[p], nbx, nby, NUM_REFS, hg, outs[p], bound, eress[p]) for p in range(NPIC)]
        ctx.motion_encode_batch(epics)
        ctx.synchronize()
        sizes = [sa.motion_encode_result(r.download())["bytes"] for r in eress]
        dpics = [(outs[p], sizes[p], None, nbx, nby, NUM_REFS, hg, decoded[p], dress[p]) for p in range(NPIC)]
        field_mb = NPIC * host[0].nbytes / 1e6

        def decode():
            ctx.motion_decode_batch(dpics)

        def encode():
            ctx.motion_encode_batch(epics)

        def copy_up():
            for p in range(NPIC):
                decoded[p].upload_async(pinned[p])

        decode()
        ctx.synchronize()
        for p in range(NPIC):
            r = sa.motion_decode_result(dress[p].download())
            assert decoded[p].download().tobytes() == canonical[p % 2], "picture %d is not canonical (its source)" % p
            assert r["bytes"] == sizes[p] and not (r["truncated"] or r["overran"] or r["not_consumed"] or r["long_codes"] or r["unverified"]), r
        diagonals = nbx + nby - 1
        lines.append("%d-pixel separation%s: %d x %d blocks, %.2f MB of records and %.3f MB of stream for the call; %d diagonals of blocks, %d "
                     "of superblocks; every decoded field is canonical (its source)"
                     % (sep, ", global motion" if hg else "", nbx, nby, field_mb, sum(sizes) / 1e6, diagonals, nbx // 4 + nby // 4 - 1))
        steps = 1 if hg else None
        t, spread = timed(ctx, decode, a, steps)
        lines.append("  decode     %8.4f ms per call, %8.4f ms per picture, spread %.1f %%" % (t, t / NPIC, 100 * spread))
        if experiments:
            for bit, name in STAGES:
                if hg and bit != 32:
                    continue
                os.environ["SCHRO_HIP_MOTDEC_STAGES"] = str(bit)
                ts, spread = timed(ctx, decode, a, steps)
                per = ""
                if bit >= 16 and not hg:
                    n = diagonals if bit > 16 else nbx // 4 + nby // 4 - 1
                    per = ", %.2f us per diagonal (walk and prefix sums together)" % (1000 * ts / n)
                lines.append("  launch %-10s %8.4f ms per call (%4.1f %% of the call), spread %.1f %%%s" % (name, ts, 100 * ts / t, 100 * spread, per))
            os.environ.pop("SCHRO_HIP_MOTDEC_STAGES", None)
            decode()                    # (whole tables again)
            ctx.synchronize()
        if not hg:
            tc, spread = timed(ctx, copy_up, a)
            lines.append("  copy up    %8.4f ms per call for the eight fields from pinned memory (%.1f GB/s), spread %.1f %%" % (tc, field_mb / tc, 100 * spread))
            te, spread = timed(ctx, encode, a)
            lines.append("  encode     %8.4f ms per call, spread %.1f %%" % (te, 100 * spread))
            lines.append("  ratio decode / copy up %.2f, decode / encode %.2f" % (t / tc, t / te))
        for p in fields + outs + eress + decoded + dress:
            p.free()
    lines.append("not shown: the host's serial parse of the motion data, which the call saves (that parser is not built here: unmeasured)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
