#!/usr/bin/env python3
"""What the v210 level route (iiwt.hip, iiwt_v210_kernel: the finest level writes v210) saves against the two passes.

One 4:2:2 s32 picture per call of schro_hip_iiwt_pack_v210_batch, for every filter, at 7680 x 4320 and 1920 x 1080 (the
transform 1920 x 1088 at depth 4 is another case; here depth 3: 1080 rows are a whole transform), depth 3.  One process with
the experiments library: SCHRO_HIP_V210_TWO_PASS=1 sends the picture to the two passes (transform into a pixel frame, then
the pack), unset it takes the level route (the three-level s32 Haar kernel takes 7680 x 4320 Haar
whichever is asked for: "haar3" in both columns).  Rounds alternate the routes; per round a call is timed as the stream's
elapsed time around `steps` calls after `warmup` more, divided by steps; the table gives medians over the rounds.  "kernel" is the
level route's v210 launch alone at depth 1 (no coarse levels: the launch's own time from its HIP events) with the bytes it
must move -- the frame's four sub-bands read once, the v210 rows written once -- against 8 TB/s.

  SCHRO_HIP_LIB=schroedinger_amd/libschro_hip_exp.so python scripts/v210_every_filter.py [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXP = os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so")
os.environ.setdefault("SCHRO_HIP_LIB", EXP)

import numpy as np                      # noqa: E402
import schroedinger_amd as sa           # noqa: E402

SIZES = [(7680, 4320), (1920, 1080)]
NAMES = ["DD(9,7)", "LeGall(5,3)", "DD(13,7)", "Haar0", "Haar1", "Fidelity", "Daub(9,7)"]


def picture(ctx, w, h, seed):
    rng = np.random.default_rng(seed)
    co = [ctx.upload(rng.integers(-2000, 2000, size=d, dtype=np.int32)) for d in [(h, w), (h, w // 2), (h, w // 2)]]
    dst = ctx.plane(h, 16 * (-(-w // 6)), np.uint8)
    return co, dst


def timed(ctx, jobs, depth, filt, route, steps, warmup):
    if route == "two_pass":
        os.environ["SCHRO_HIP_V210_TWO_PASS"] = "1"
    else:
        os.environ.pop("SCHRO_HIP_V210_TWO_PASS", None)
    for _ in range(warmup):
        ctx.iiwt_pack_v210_batch(jobs, depth, filt)
    ctx.synchronize()
    ctx.v210_routes(reset=True)
    ctx.timer_begin()
    for _ in range(steps):
        ctx.iiwt_pack_v210_batch(jobs, depth, filt)
    ms = ctx.timer_end() / steps
    got = ctx.v210_routes(reset=True)
    took = [r for r, n in got.items() if n]
    assert len(took) == 1 and got[took[0]] == steps * len(jobs) \
        and (took[0] == "haar3" or (took[0] == "two_pass") == (route == "two_pass")), (route, got)
    return ms, took[0]


def kernel_alone(ctx, jobs, filt, steps):
    os.environ.pop("SCHRO_HIP_V210_TWO_PASS", None)
    ctx.iiwt_pack_v210_batch(jobs, 1, filt)
    ctx.synchronize()
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(steps):
        ctx.iiwt_pack_v210_batch(jobs, 1, filt)
    ctx.synchronize()
    ms, n = ctx.profile_read()["iiwt_finest"]
    ctx.profile_enable(False)
    assert n == steps, n
    return ms / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = sa.Context(0)
    rows = []
    for (w, h) in SIZES:
        co, dst = picture(ctx, w, h, 7)
        jobs = [(co, 1, 0, dst, w, h)]
        for filt in range(7):
            t = {"level": [], "two_pass": []}
            for _ in range(a.rounds):
                for route in ("level", "two_pass"):
                    ms, took = timed(ctx, jobs, 3, filt, route, a.steps, a.warmup)
                    t[route].append(ms)
                    if route == "level":
                        first = took
            k = kernel_alone(ctx, jobs, filt, a.steps)
            nbytes = 4 * w * h * 2 + 16 * (-(-w // 6)) * h
            row = {"size": "%dx%d" % (w, h), "filter": filt, "name": NAMES[filt], "depth": 3, "route": first,
                   "level_ms": statistics.median(t["level"]), "two_pass_ms": statistics.median(t["two_pass"]),
                   "kernel_ms": k, "kernel_mb": nbytes / 1e6, "kernel_tbs": nbytes / (k * 1e-3) / 1e12,
                   "rounds": {r: [round(x, 4) for x in v] for r, v in t.items()}}
            row["kernel_of_8tbs"] = row["kernel_tbs"] / 8.0
            rows.append(row)
            print(json.dumps(row), flush=True)
        [p.free() for p in co + [dst]]
    lines = ["# scripts/v210_every_filter.py: one 4:2:2 s32 picture per call, depth 3, medians of %d rounds x %d calls"
             % (a.rounds, a.steps),
             "# level = iiwt_v210_kernel route (coarse levels + finest level writing v210); two_pass = pixel frame + pack;"
             " kernel = the v210 launch alone at depth 1",
             "%-10s %-12s %-6s %9s %9s %7s %10s %8s %7s" % ("size", "filter", "route", "level", "two_pass", "ratio", "kernel_ms", "TB/s", "of 8")]
    for r in rows:
        lines.append("%-10s %-12s %-6s %9.4f %9.4f %7.2f %10.4f %8.2f %6.0f%%" % (
            r["size"], r["name"], r["route"], r["level_ms"], r["two_pass_ms"], r["level_ms"] / r["two_pass_ms"], r["kernel_ms"],
            r["kernel_tbs"], 100 * r["kernel_of_8tbs"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
