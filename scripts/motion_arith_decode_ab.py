#!/usr/bin/env python3
"""First numbers for the motion-data decoder of arithmetic-coded pictures (motion_arith_dec.hip) beside what it replaces.

Workload: the 96 inter pictures of tests/golden/test_stream.drc (320 x 240, 40 x 32 blocks), their motion data as the
stream carries it, at 1, 8 and 96 pictures per call; and one 2160p-sized field (240 x 136 blocks, two references,
tests/motion_enc_cases.py search_like) written with the tests' arithmetic writer.  Every decoded field is held against its
source -- the oracle's field, the canonical drawn field -- before anything is timed.

In the same run, on the same pictures:

  schro_hip_motion_arith_decode_batch   the whole call;
  its launches one at a time            (experiments library only: SCHRO_HIP_MOTARITH_STAGES = 1 header, 2 split chain, 4
                                        split walk, 8 mode chain, 16 mode walk, 32 value chains, 64 value walk; each runs on
                                        the tables the full call before it left);
  bins per section                      from the results; a chain launch lasts as long as its longest chain, so its time
                                        over that chain's bins is the ns per bin of a chain, launch overhead included;
  the host-to-device copy               of the fields from pinned memory: the hand-over the call replaces;
  schro_hip_motion_decode_batch         on the VLC twin of the same pictures (tests/noarith_twin.py);
  800 ns per bin                        what DESIGN 4.24 measured for a transform-data chain, quoted.

Times: device events around `steps` calls (Context.timer_begin / timer_end), per call; the median of `rounds` rounds after
`warmup` calls, and the spread (max - min) / median.  NOT shown: the reference's host decoder, which is not built by the
committed recipe -- unmeasured.

  SCHRO_HIP_LIB=schroedinger_amd/libschro_hip_exp.so python scripts/motion_arith_decode_ab.py [--out profiles/motion_arith_decode.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, d))

import numpy as np                      # noqa: E402
import motion_arith_dec_ref as A        # noqa: E402
import motion_enc_cases as MC           # noqa: E402
import motion_enc_ref as ref            # noqa: E402
import noarith_twin as T                # noqa: E402
import schroedinger_amd as sa           # noqa: E402
from schroedinger_amd import _lib       # noqa: E402

STAGES = ((1, "header", None), (2, "split chain", (0,)), (4, "split walk", None), (8, "mode chain", (1,)), (16, "mode walk", None),
          (32, "value chains", (2, 3, 4, 5, 6, 7, 8)), (64, "value walk", None))
DESIGN_4_24_NS_PER_BIN = 800


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


class Set:
    """Pictures on the device: (bytes, nbx, nby, num_refs, the field they must decode to) each."""

    def __init__(self, ctx, pictures):
        self.ctx, self.pictures = ctx, pictures
        words = C.sizeof(_lib.MotionArithDecodeResult) // 4
        self.data = [ctx.upload_bytes(np.frombuffer(p[0], np.uint8)) for p in pictures]
        self.field = [ctx.plane(1, len(p[4]), np.uint8) for p in pictures]
        self.res = [ctx.plane(1, words, np.uint32) for _ in pictures]
        self.entries = [(d, len(p[0]), None, p[1], p[2], p[3], 0, f, r) for p, d, f, r in zip(pictures, self.data, self.field, self.res)]

    def check(self):
        self.ctx.motion_arith_decode_batch(self.entries)
        self.ctx.synchronize()
        results = []
        for n, p in enumerate(self.pictures):
            assert self.field[n].download().tobytes() == p[4], "picture %d does not decode to its source" % n
            r = sa.motion_arith_decode_result(self.res[n].download())
            assert r["bytes"] == len(p[0]) and not (r["truncated"] or r["overran"] or r["long_codes"] or r["unverified"]), r
            results.append(r)
        return results

    def free(self):
        for p in self.data + self.field + self.res:
            p.free()


def report(ctx, a, lines, s, per_call, results, experiments):
    """The call at `per_call` pictures, and -- experiments library -- each launch with the ns per bin of its longest chain."""
    entries = s.entries[:per_call]
    call = lambda: ctx.motion_arith_decode_batch(entries)
    t, spread = timed(ctx, call, a)
    lines.append("  %3d per call: %8.4f ms per call, %8.4f ms per picture, spread %.1f %%" % (per_call, t, t / per_call, 100 * spread))
    if not experiments:
        return t
    for bit, name, sections in STAGES:
        os.environ["SCHRO_HIP_MOTARITH_STAGES"] = str(bit)
        ts, spread = timed(ctx, call, a)
        per = ""
        if sections:
            longest = max(r["section_bins"][k] for r in results[:per_call] for k in sections)
            per = ", longest chain %d bins: %.0f ns per bin" % (longest, 1e6 * ts / longest)
        lines.append("      launch %-12s %8.4f ms (%4.1f %% of the call), spread %.1f %%%s" % (name, ts, 100 * ts / t, 100 * spread, per))
    os.environ.pop("SCHRO_HIP_MOTARITH_STAGES", None)
    call()
    ctx.synchronize()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    experiments = "exp" in os.path.basename(_lib.LIB_PATH)
    lines = ["motion_arith_decode_ab%s; device events, median of %d rounds of %d calls" % (", experiments library" if experiments else "", a.rounds, a.steps)]

    # ---- the stream ----------------------------------------------------------------------------------------------------------
    recs = list(T.motion_pictures())
    stream = [(data, r["nbx"], r["nby"], r["num_refs"], r["mv"].tobytes()) for (pic, payload, data), r in zip(A.stream_pictures(), recs)]
    s = Set(ctx, stream)
    results = s.check()
    bins = np.array([r["section_bins"] for r in results])
    lines.append("the stream's %d inter pictures, %d x %d blocks, %d bytes of motion data (%d .. %d a picture); every field is the oracle's"
                 % (len(stream), recs[0]["nbx"], recs[0]["nby"], sum(len(p[0]) for p in stream), min(len(p[0]) for p in stream),
                    max(len(p[0]) for p in stream)))
    lines.append("  bins per section, mean over the pictures: %s; the longest chain of a picture %d .. %d bins"
                 % (" ".join("%.0f" % v for v in bins.mean(axis=0)), bins.max(axis=1).min(), bins.max(axis=1).max()))
    for per_call in (1, 8, 96):
        report(ctx, a, lines, s, per_call, results, experiments)
    # the hand-over the call replaces, and the VLC twin
    pinned = [ctx.host_array((1, len(p[4])), np.uint8) for p in stream]
    for h, p in zip(pinned, stream):
        h[:] = np.frombuffer(p[4], np.uint8).reshape(1, -1)
    for per_call in (1, 8, 96):
        def copy_up():
            for n in range(per_call):
                s.field[n].upload_async(pinned[n])
        tc, spread = timed(ctx, copy_up, a)
        lines.append("  copy up %3d fields from pinned memory: %8.4f ms (%.2f GB/s), spread %.1f %%"
                     % (per_call, tc, per_call * len(stream[0][4]) / 1e6 / tc, 100 * spread))
    vwords = C.sizeof(_lib.MotionDecodeResult) // 4
    vdata = [ctx.upload_bytes(np.frombuffer(r["motion"], np.uint8)) for r in recs]
    vres = [ctx.plane(1, vwords, np.uint32) for _ in recs]
    ventries = [(d, len(r["motion"]), None, r["nbx"], r["nby"], r["num_refs"], 0, f, v) for r, d, f, v in zip(recs, vdata, s.field, vres)]
    ctx.motion_decode_batch(ventries)
    ctx.synchronize()
    for n, p in enumerate(stream):
        assert s.field[n].download().tobytes() == p[4]
    for per_call in (1, 8, 96):
        tv, spread = timed(ctx, lambda: ctx.motion_decode_batch(ventries[:per_call]), a)
        lines.append("  motion_decode_batch on the VLC twin, %3d per call: %8.4f ms, spread %.1f %%" % (per_call, tv, 100 * spread))
    for p in vdata + vres:
        p.free()
    s.free()

    # ---- one 2160p-sized field -------------------------------------------------------------------------------------------------
    nbx, nby = 240, 136
    field = ref.canonical(MC.search_like(40, nbx, nby, 2))
    data = A.write_field(field, nbx, nby, 2, 0)
    s = Set(ctx, [(data, nbx, nby, 2, field.tobytes())])
    results = s.check()
    lines.append("one field of %d x %d blocks, two references (search_like, the tests' writer): %d bytes; decodes to its source"
                 % (nbx, nby, len(data)))
    lines.append("  bins per section: %s" % " ".join(str(v) for v in results[0]["section_bins"]))
    report(ctx, a, lines, s, 1, results, experiments)
    h = ctx.host_array((1, field.nbytes), np.uint8)
    h[:] = field.view(np.uint8).reshape(1, -1)
    tc, spread = timed(ctx, lambda: s.field[0].upload_async(h), a)
    lines.append("  copy up the field from pinned memory: %8.4f ms (%.2f GB/s), spread %.1f %%" % (tc, field.nbytes / 1e6 / tc, 100 * spread))
    vbytes = ref.encode(field, nbx, nby, 2, 0)[0]
    vd, vr = ctx.upload_bytes(np.frombuffer(vbytes, np.uint8)), ctx.plane(1, vwords, np.uint32)
    tv, spread = timed(ctx, lambda: ctx.motion_decode_batch([(vd, len(vbytes), None, nbx, nby, 2, 0, s.field[0], vr)]), a)
    lines.append("  motion_decode_batch on the same field's VLC bytes (%d): %8.4f ms, spread %.1f %%" % (len(vbytes), tv, 100 * spread))
    s.free()
    lines.append("beside: DESIGN 4.24 measured %d ns per bin for a transform-data chain" % DESIGN_4_24_NS_PER_BIN)
    lines.append("not shown: the reference's host decoder of the motion data (not built by the committed recipe: unmeasured)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
