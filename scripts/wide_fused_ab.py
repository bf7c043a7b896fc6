#!/usr/bin/env python3
"""What the > 8-bit level route (iiwt.hip, iiwt_wide_kernel: the finest level shifts, converts and writes v216 / ARGB / AY64)
saves against the chain it replaces.

Depth 3, every filter, s16 and s32 sources, without a shift and with one (2).  Per call 8 x 2160p pictures (eight: the working
set exceeds the 256 MiB Infinity Cache) 4:2:2 -> v216, 4:4:4 -> ARGB and 4:4:4 -> AY64, and one 8K 4:2:2 picture -> v216.  Two
forms in one process and one build:
  level   schro_hip_iiwt_pack_wide_batch with the experiments library and SCHRO_HIP_WIDE_LEVEL=1: every combination takes the
          level kernel, also those the product library keeps on the two passes (all pictures must report the LEVEL route);
  chain   the three plane-layer calls it replaces: schro_hip_iiwt_batch into s16 / s32 pixel planes, schro_hip_shift_right_batch
          (with a shift), schro_hip_pack_wide_batch.
The outputs of the two forms are compared first.  Rounds alternate the forms; per round a call is timed as the stream's
elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps; the table gives the medians over the
rounds and each form's round-to-round spread (max - min) / median.  A combination counts as faster on the level route only
if the gap between the medians exceeds both spreads; the product library takes LEVEL where that holds without a shift AND
with one (wide_level_combination, iiwt_pack.cpp).

  python scripts/wide_fused_ab.py [--rounds 5] [--steps 20] [--out-prefix profiles/r10_wide_fused]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SCHRO_HIP_LIB", os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so"))
os.environ["SCHRO_HIP_WIDE_LEVEL"] = "1"
os.environ.pop("SCHRO_HIP_WIDE_TWO_PASS", None)

import numpy as np                      # noqa: E402
import schroedinger_amd as sa           # noqa: E402

DEPTH, SHIFT = 3, 2
NAMES = ["DD(9,7)", "LeGall(5,3)", "DD(13,7)", "Haar0", "Haar1", "Fidelity", "Daub(9,7)"]
# (name, format, h_shift, width, height, pictures per call)
CONFIGS = [("v216-422", sa.FORMAT_V216, 1, 3840, 2160, 8), ("argb-444", sa.FORMAT_ARGB, 0, 3840, 2160, 8),
           ("ay64-444", sa.FORMAT_AY64, 0, 3840, 2160, 8), ("v216-8k", sa.FORMAT_V216, 1, 7680, 4320, 1)]
ROW = {sa.FORMAT_V216: lambda w: 4 * w, sa.FORMAT_ARGB: lambda w: 4 * w, sa.FORMAT_AY64: lambda w: 8 * w}


def pictures(ctx, fmt, hs, w, h, npic, dtype, seed):
    rng = np.random.default_rng(seed)
    dims = [(h, w), (h, w >> hs), (h, w >> hs)]
    co_np = [rng.integers(-3000, 3000, size=d).astype(dtype) for d in dims]
    return [{"co": [ctx.upload(a) for a in co_np], "pixel": [ctx.plane(d[0], d[1], dtype) for d in dims],
             "level": ctx.plane(h, ROW[fmt](w), np.uint8), "chain": ctx.plane(h, ROW[fmt](w), np.uint8)} for _ in range(npic)]


def call(ctx, form, pics, fmt, hs, w, h, filt, shift):
    if form == "level":
        ctx.iiwt_pack_wide_batch([(p["co"], hs, 0, p["level"], w, h, fmt, shift) for p in pics], DEPTH, filt)
    else:
        ctx.iiwt_batch([(p["co"][k], p["pixel"][k]) for p in pics for k in range(3)], DEPTH, filt)
        if shift:
            ctx.shift_right_batch([p["pixel"][k] for p in pics for k in range(3)], shift)
        ctx.pack_wide_batch([(p["pixel"], hs, 0, p["chain"], w, h, fmt) for p in pics])


def timed(ctx, form, pics, args, steps, warmup):
    for _ in range(warmup):
        call(ctx, form, pics, *args)
    ctx.synchronize()
    ctx.wide_routes(reset=True)
    ctx.timer_begin()
    for _ in range(steps):
        call(ctx, form, pics, *args)
    ms = ctx.timer_end() / steps
    got = ctx.wide_routes(reset=True)
    assert got == ({"level": steps * len(pics), "two_pass": 0} if form == "level" else {"level": 0, "two_pass": 0}), (form, got)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--filters", default="0,1,2,3,4,5,6")
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    ap.add_argument("--out-prefix")
    a = ap.parse_args()
    assert a.rounds >= 5 and a.rounds * a.steps >= 100, "at least five rounds and 100 timed steps per form"
    ctx = sa.Context(0)
    rows = []

    def flush():
        lines = ["# scripts/wide_fused_ab.py: depth %d, ms per call, medians of %d rounds x %d calls; 8 x 3840x2160 pictures per call, "
                 "v216-8k one 7680x4320 picture" % (DEPTH, a.rounds, a.steps),
                 "# level = schro_hip_iiwt_pack_wide_batch on the LEVEL route; chain = schro_hip_iiwt_batch + schro_hip_shift_right_batch "
                 "(shift %d) + schro_hip_pack_wide_batch;" % SHIFT,
                 "# spread = (max - min) / median over the rounds; faster: (chain - level) / chain > the larger spread",
                 "%-9s %-4s %-5s %-12s %9s %9s %7s %8s %8s %s" % ("config", "type", "shift", "filter", "level", "chain", "ratio", "spr.lvl",
                                                               "spr.chn", "faster")]
        for r in rows:
            lines.append("%-9s %-4s %-5d %-12s %9.4f %9.4f %7.2f %7.1f%% %7.1f%% %s" % (
                r["config"], r["type"], r["shift"], r["name"], r["level_ms"], r["chain_ms"], r["ratio"],
                100 * r["level_spread"], 100 * r["chain_spread"], "yes" if r["faster"] else "NO"))
        text = "\n".join(lines) + "\n"
        if a.out_prefix:
            with open(a.out_prefix + ".jsonl", "w") as f:
                f.writelines(json.dumps(r) + "\n" for r in rows)
            with open(a.out_prefix + ".txt", "w") as f:
                f.write(text)
        return text

    for (cname, fmt, hs, w, h, npic) in CONFIGS:
        if cname not in a.configs.split(","):
            continue
        for dtype in (np.int16, np.int32):
            pics = pictures(ctx, fmt, hs, w, h, npic, dtype, 11)
            for filt in [int(f) for f in a.filters.split(",")]:
                for shift in (0, SHIFT):
                    args = (fmt, hs, w, h, filt, shift)
                    for form in ("level", "chain"):
                        call(ctx, form, pics, *args)
                    ctx.synchronize()
                    for n in (0, npic - 1):
                        assert np.array_equal(pics[n]["level"].download(), pics[n]["chain"].download()), (cname, dtype, filt, shift, n)
                    t = {"level": [], "chain": []}
                    for _ in range(a.rounds):
                        for form in ("level", "chain"):
                            t[form].append(timed(ctx, form, pics, args, a.steps, a.warmup))
                    med = {f: statistics.median(v) for f, v in t.items()}
                    spread = {f: (max(v) - min(v)) / med[f] for f, v in t.items()}
                    row = {"config": cname, "type": "s16" if dtype == np.int16 else "s32", "shift": shift, "filter": filt,
                           "name": NAMES[filt], "depth": DEPTH, "pictures": npic, "size": "%dx%d" % (w, h), "level_ms": med["level"],
                           "chain_ms": med["chain"], "ratio": med["level"] / med["chain"], "level_spread": spread["level"],
                           "chain_spread": spread["chain"], "faster": (med["chain"] - med["level"]) / med["chain"] > max(spread.values()),
                           "rounds": {f: [round(x, 4) for x in v] for f, v in t.items()}}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    flush()
            for p in pics:
                [q.free() for q in p["co"] + p["pixel"] + [p["level"], p["chain"]]]
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
