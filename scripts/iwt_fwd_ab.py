#!/usr/bin/env python3
"""The forward wavelet (schro_hip_iwt_batch, iwt_fwd.hip's LDS tile kernel) against the inverse on the same planes.

8 x 2160p 4:2:0 pictures per call (24 planes; eight pictures: the working set exceeds the 256 MiB Infinity Cache), depth 3, every
filter, s16 and s32.  Three forms in one process, on the experiments library:
  fwd      one schro_hip_iwt_batch: pixel planes -> coefficient planes;
  inv_lds  one schro_hip_iiwt_batch (plain, no combine) on those coefficient planes with SCHRO_HIP_IIWT_REG=0 and
           SCHRO_HIP_IIWT_HAAR=0: every level on iiwt_level_kernel, the like-for-like LDS formulation -- the yardstick;
  inv      the same call as the product routes it (register kernels, level 1 inside level 0, the element-wise s32 Haar).
The forward result is compared with the round trip first (forward, inverse = the input).  Rounds alternate the forms; per round
a call is timed as the stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps; the table
gives the medians over the rounds, each form's round-to-round spread (max - min) / median, and the fraction of 8 TB/s the median
is on the algorithmic traffic: one read and one write of every sample of every level, 4 B (s16) / 8 B (s32) per sample and level.
"slower": the forward median exceeds the LDS inverse's by more than the larger of the two spreads.

  python scripts/iwt_fwd_ab.py [--rounds 5] [--steps 20] [--out profiles/r11_iwt_fwd.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SCHRO_HIP_LIB", os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so"))

import numpy as np                      # noqa: E402
import schroedinger_amd as sa           # noqa: E402

DEPTH, NPIC, W, H = 3, 8, 3840, 2160
PEAK = 8e12
NAMES = ["DD(9,7)", "LeGall(5,3)", "DD(13,7)", "Haar0", "Haar1", "Fidelity", "Daub(9,7)"]
FORMS = ("fwd", "inv_lds", "inv")


def call(ctx, form, pix, co, back, filt):
    if form == "fwd":
        ctx.iwt_batch(list(zip(pix, co)), DEPTH, filt)
        return
    for name in ("SCHRO_HIP_IIWT_REG", "SCHRO_HIP_IIWT_HAAR"):
        if form == "inv_lds":
            os.environ[name] = "0"
        else:
            os.environ.pop(name, None)
    ctx.iiwt_batch(list(zip(co, back)), DEPTH, filt)


def timed(ctx, form, args, steps, warmup):
    for _ in range(warmup):
        call(ctx, form, *args)
    ctx.synchronize()
    ctx.timer_begin()
    for _ in range(steps):
        call(ctx, form, *args)
    return ctx.timer_end() / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--filters", default="0,1,2,3,4,5,6")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.rounds >= 5, "at least five alternating rounds"
    ctx = sa.Context(0)
    rows = []

    def flush():
        lines = ["# scripts/iwt_fwd_ab.py: %d x %dx%d 4:2:0 pictures per call, depth %d; ms per call, medians of %d alternating rounds x %d calls"
                 % (NPIC, W, H, DEPTH, a.rounds, a.steps),
                 "# fwd = schro_hip_iwt_batch (iwt_fwd_level_kernel); inv_lds = schro_hip_iiwt_batch with every level on iiwt_level_kernel "
                 "(experiments library, SCHRO_HIP_IIWT_REG=0 SCHRO_HIP_IIWT_HAAR=0): the yardstick; inv = the product's routing",
                 "# of8TB/s = (4 B (s16) / 8 B (s32) per sample and level) / median / 8 TB/s; spread = (max - min) / median over the rounds;",
                 "# slower: (fwd - inv_lds) / inv_lds > the larger of the two spreads",
                 "%-4s %-12s %9s %8s %7s %9s %8s %7s %9s %8s %7s %8s %s" % ("type", "filter", "fwd", "of8TB/s", "spread", "inv_lds", "of8TB/s", "spread",
                                                                          "inv", "of8TB/s", "spread", "fwd/lds", "slower")]
        for r in rows:
            lines.append("%-4s %-12s %9.4f %7.1f%% %6.1f%% %9.4f %7.1f%% %6.1f%% %9.4f %7.1f%% %6.1f%% %8.2f %s" % (
                r["type"], r["name"], r["fwd_ms"], 100 * r["fwd_frac"], 100 * r["fwd_spread"], r["inv_lds_ms"], 100 * r["inv_lds_frac"],
                100 * r["inv_lds_spread"], r["inv_ms"], 100 * r["inv_frac"], 100 * r["inv_spread"], r["ratio"], "YES" if r["slower"] else "no"))
        text = "\n".join(lines) + "\n"
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return text

    dims = [(H, W), (H // 2, W // 2), (H // 2, W // 2)] * NPIC
    samples = sum(h * w for h, w in dims)
    for dtype in (np.int16, np.int32):
        bpp = np.dtype(dtype).itemsize
        traffic = sum((samples >> (2 * l)) * 2 * bpp for l in range(DEPTH))
        rng = np.random.default_rng(11)
        host = [rng.integers(-128, 128, size=d).astype(dtype) for d in dims[:3]]
        pix = [ctx.upload(host[k % 3]) for k in range(len(dims))]
        co = [ctx.plane(d[0], d[1], dtype) for d in dims]
        back = [ctx.plane(d[0], d[1], dtype) for d in dims]
        for filt in [int(f) for f in a.filters.split(",")]:
            args = (pix, co, back, filt)
            for form in ("fwd", "inv_lds"):
                call(ctx, form, *args)
            ctx.synchronize()
            for n in (0, 1, len(dims) - 1):
                assert np.array_equal(back[n].download(), host[n % 3]), ("round trip", dtype, filt, n)
            t = {f: [] for f in FORMS}
            for _ in range(a.rounds):
                for form in FORMS:
                    t[form].append(timed(ctx, form, args, a.steps, a.warmup))
            med = {f: statistics.median(v) for f, v in t.items()}
            spread = {f: (max(v) - min(v)) / med[f] for f, v in t.items()}
            row = {"type": "s16" if dtype == np.int16 else "s32", "filter": filt, "name": NAMES[filt],
                   "ratio": med["fwd"] / med["inv_lds"],
                   "slower": (med["fwd"] - med["inv_lds"]) / med["inv_lds"] > max(spread["fwd"], spread["inv_lds"]),
                   "rounds": {f: [round(x, 4) for x in v] for f, v in t.items()}}
            for f in FORMS:
                row[f + "_ms"], row[f + "_spread"], row[f + "_frac"] = med[f], spread[f], traffic / (med[f] * 1e-3) / PEAK
            rows.append(row)
            print(json.dumps(row), flush=True)
            flush()
        [p.free() for p in pix + co + back]
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
