#!/usr/bin/env python3
"""What the packed 8-bit level route (iiwt.hip, iiwt_pack8_kernel: the finest level writes YUYV / UYVY / AYUV) saves against
the chain it replaces.

8 x 2160p s16 pictures per call (eight: the working set exceeds the 256 MiB Infinity Cache), every filter, depth 3, with
and without a prediction, 4:2:2 -> YUYV and 4:4:4 -> AYUV.  Two forms in one process and one build:
  level   schro_hip_iiwt_pack_u8_batch with the experiments library and SCHRO_HIP_PACK8_LEVEL=1: every filter takes the level
          kernel, also those the product library keeps on the two passes (all pictures must report the LEVEL route);
  chain   schro_hip_iiwt_batch in its combine form into planar u8 planes, then schro_hip_pack_u8_batch.
The outputs of the two forms are compared first.  Rounds alternate the forms; per round a call is timed as the stream's
elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps; the table gives the medians over the
rounds and each form's round-to-round spread (max - min) / median.  A filter counts as faster on the level route only if
the gap between the medians exceeds both spreads.

  python scripts/pack8_fused_ab.py [--rounds 5] [--steps 20] [--out-prefix profiles/r09_pack8_fused]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SCHRO_HIP_LIB", os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so"))
os.environ["SCHRO_HIP_PACK8_LEVEL"] = "1"

import numpy as np                      # noqa: E402
import schroedinger_amd as sa           # noqa: E402

W, H, NPIC, DEPTH = 3840, 2160, 8, 3
NAMES = ["DD(9,7)", "LeGall(5,3)", "DD(13,7)", "Haar0", "Haar1", "Fidelity", "Daub(9,7)"]
CONFIGS = [("yuyv-422", sa.FORMAT_YUYV, 1), ("ayuv-444", sa.FORMAT_AYUV, 0)]


def pictures(ctx, fmt, hs, with_pred, seed):
    rng = np.random.default_rng(seed)
    dims = [(H, W), (H, W >> hs), (H, W >> hs)]
    co_np = [rng.integers(-300, 300, size=d, dtype=np.int16) for d in dims]
    pr_np = [rng.integers(0, 256, size=d, dtype=np.uint8) for d in dims]
    row = 4 * W if fmt == sa.FORMAT_AYUV else 2 * W
    pics = []
    for _ in range(NPIC):
        pics.append({"co": [ctx.upload(a) for a in co_np], "pred": [ctx.upload(a) for a in pr_np] if with_pred else None,
                     "planar": [ctx.plane(d[0], d[1], np.uint8) for d in dims],
                     "level": ctx.plane(H, row, np.uint8), "chain": ctx.plane(H, row, np.uint8)})
    return pics


def call(ctx, form, pics, fmt, hs, filt):
    if form == "level":
        ctx.iiwt_pack_u8_batch([(p["co"], hs, 0, p["pred"], p["level"], W, H, fmt) for p in pics], DEPTH, filt)
    else:
        ctx.iiwt_batch([(p["co"][k], p["planar"][k], p["pred"][k] if p["pred"] else None) for p in pics for k in range(3)], DEPTH, filt)
        ctx.pack_u8_batch([(p["planar"], hs, 0, p["chain"], W, H, fmt) for p in pics])


def timed(ctx, form, pics, fmt, hs, filt, steps, warmup):
    for _ in range(warmup):
        call(ctx, form, pics, fmt, hs, filt)
    ctx.synchronize()
    ctx.pack8_routes(reset=True)
    ctx.timer_begin()
    for _ in range(steps):
        call(ctx, form, pics, fmt, hs, filt)
    ms = ctx.timer_end() / steps
    got = ctx.pack8_routes(reset=True)
    assert got == ({"level": steps * NPIC, "two_pass": 0} if form == "level" else {"level": 0, "two_pass": 0}), (form, got)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--filters", default="0,1,2,3,4,5,6")
    ap.add_argument("--out-prefix")
    a = ap.parse_args()
    assert a.rounds * a.steps >= 100, "at least 100 timed steps per form"
    ctx = sa.Context(0)
    rows = []
    for (cname, fmt, hs) in CONFIGS:
        for with_pred in (False, True):
            pics = pictures(ctx, fmt, hs, with_pred, 11)
            for filt in [int(f) for f in a.filters.split(",")]:
                for form in ("level", "chain"):
                    call(ctx, form, pics, fmt, hs, filt)
                ctx.synchronize()
                for n in (0, NPIC - 1):
                    assert np.array_equal(pics[n]["level"].download(), pics[n]["chain"].download()), (cname, with_pred, filt, n)
                t = {"level": [], "chain": []}
                for _ in range(a.rounds):
                    for form in ("level", "chain"):
                        t[form].append(timed(ctx, form, pics, fmt, hs, filt, a.steps, a.warmup))
                med = {f: statistics.median(v) for f, v in t.items()}
                spread = {f: (max(v) - min(v)) / med[f] for f, v in t.items()}
                row = {"config": cname, "prediction": with_pred, "filter": filt, "name": NAMES[filt], "depth": DEPTH,
                       "pictures": NPIC, "size": "%dx%d" % (W, H), "level_ms": med["level"], "chain_ms": med["chain"],
                       "ratio": med["level"] / med["chain"], "level_spread": spread["level"], "chain_spread": spread["chain"],
                       "faster": (med["chain"] - med["level"]) / med["chain"] > max(spread.values()),
                       "rounds": {f: [round(x, 4) for x in v] for f, v in t.items()}}
                rows.append(row)
                print(json.dumps(row), flush=True)
            for p in pics:
                [q.free() for q in p["co"] + (p["pred"] or []) + p["planar"] + [p["level"], p["chain"]]]
    lines = ["# scripts/pack8_fused_ab.py: %d x %dx%d s16 pictures per call, depth %d, ms per call, medians of %d rounds x %d calls"
             % (NPIC, W, H, DEPTH, a.rounds, a.steps),
             "# level = schro_hip_iiwt_pack_u8_batch on the LEVEL route; chain = schro_hip_iiwt_batch (combine) + schro_hip_pack_u8_batch;"
             " spread = (max - min) / median over the rounds",
             "%-9s %-5s %-12s %9s %9s %7s %8s %8s %s" % ("config", "pred", "filter", "level", "chain", "ratio", "spr.lvl", "spr.chn", "faster")]
    for r in rows:
        lines.append("%-9s %-5s %-12s %9.4f %9.4f %7.2f %7.1f%% %7.1f%% %s" % (
            r["config"], "yes" if r["prediction"] else "no", r["name"], r["level_ms"], r["chain_ms"], r["ratio"],
            100 * r["level_spread"], 100 * r["chain_spread"], "yes" if r["faster"] else "NO"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out_prefix:
        with open(a.out_prefix + ".jsonl", "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
        with open(a.out_prefix + ".txt", "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
