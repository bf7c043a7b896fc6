#!/usr/bin/env python3
"""What the packed level 0 of the forward wavelet (iwt_fwd.hip, iwt_fwd_packed_kernel: schro_hip_unpack_iwt_batch's FUSED
route) costs against the chain it replaces and against the transform of planes that are already on the device.

Depth 3.  Workloads: 8 x 3840x2160 4:2:2 UYVY -> s16 coefficients, LeGall (5,3) and DD (9,7); 4 x 7680x4320 4:2:2 v210 ->
s32 coefficients, Haar (BASELINE config 5 turned round).  Three forms in one process and one build:
  fused     schro_hip_unpack_iwt_batch with the experiments library and SCHRO_HIP_UNPACK_FUSED=1: every combination takes the
            packed level 0, also those the product library keeps on the two passes (all pictures must report FUSED);
  two_pass  the chain: schro_hip_unpack_batch into the packed format's own depth, schro_hip_unpack_batch (planar source)
            into the transform frame, schro_hip_iwt_batch;
  planar    schro_hip_iwt_batch over planar planes of the transform's depth: what a host that unpacks on the CPU and
            uploads 4 bytes per pixel runs -- the best there was before, and what the comparison is against.
The coefficients of the three forms are compared first.  Rounds alternate the forms; per round a call is timed as the
stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps; the table gives the medians
over the rounds and each form's round-to-round spread (max - min) / median.

  python scripts/unpack_iwt_ab.py [--rounds 5] [--steps 20] [--out-prefix profiles/unpack_iwt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# the experiments library with every combination on the FUSED route, also those the product library keeps on the two passes
os.environ.setdefault("SCHRO_HIP_LIB", os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so"))
os.environ["SCHRO_HIP_UNPACK_FUSED"] = "1"
os.environ.pop("SCHRO_HIP_UNPACK_TWO_PASS", None)

import numpy as np                      # noqa: E402
import schroedinger_amd as sa           # noqa: E402

DEPTH = 3
NAMES = ["DD(9,7)", "LeGall(5,3)", "DD(13,7)", "Haar0", "Haar1", "Fidelity", "Daub(9,7)"]
FORMS = ("fused", "two_pass", "planar")
# (name, format, the unpacked frame's dtype, width, height, pictures per call, coefficient dtype, filters)
CONFIGS = [("uyvy-2160p", sa.FORMAT_UYVY, np.uint8, 3840, 2160, 8, np.int16, (1, 0)),
           ("v210-8k", sa.FORMAT_V210, np.int16, 7680, 4320, 4, np.int32, (3,))]
# --sweep: every format x sample type x filter at 8 x 2160p, the table the product library's routes are read from
# (unpack_fused_combination, plane_unpack.cpp)
SWEEP = [("%s-%s" % (name, np.dtype(dt).name), fmt, own, 3840, 2160, 8, dt, tuple(range(7)))
         for (name, fmt, own) in (("yuyv", sa.FORMAT_YUYV, np.uint8), ("uyvy", sa.FORMAT_UYVY, np.uint8),
                                  ("ayuv", sa.FORMAT_AYUV, np.uint8), ("v210", sa.FORMAT_V210, np.int16),
                                  ("v216", sa.FORMAT_V216, np.int16), ("ay64", sa.FORMAT_AY64, np.int32))
         for dt in (np.int16, np.int32)]


def pictures(ctx, fmt, own, w, h, npic, dtype, seed):
    rng = np.random.default_rng(seed)
    row = sa.unpack_row_bytes(fmt, w)
    hs = 0 if fmt in (sa.FORMAT_AYUV, sa.FORMAT_AY64) else 1
    dims = [(h, w), (h, w >> hs), (h, w >> hs)]
    out = []
    for _ in range(npic):
        p = {"packed": ctx.upload(rng.integers(0, 256, (h, row), dtype=np.uint8)),
             "own": [ctx.plane(a, b, own) for a, b in dims], "frame": [ctx.plane(a, b, dtype) for a, b in dims]}
        for form in FORMS:
            p[form] = [ctx.plane(a, b, dtype) for a, b in dims]
        out.append(p)
    return out


def call(ctx, form, pics, fmt, w, h, filt):
    hs = 0 if fmt in (sa.FORMAT_AYUV, sa.FORMAT_AY64) else 1
    if form == "fused":
        ctx.unpack_iwt_batch([(p["packed"], fmt, w, h, w, h, p["fused"], hs, 0, w, h) for p in pics], DEPTH, filt)
        return
    if form == "two_pass":
        ctx.unpack_batch([((p["packed"], fmt, w, h), p["own"], hs, 0, w, h) for p in pics])
        ctx.unpack_batch([((p["own"], hs, 0, w, h), p["frame"], hs, 0, w, h) for p in pics])
    # (planar: p["frame"] holds the planes the two converts left)
    ctx.iwt_batch([(p["frame"][k], p[form][k]) for p in pics for k in range(3)], DEPTH, filt)


def timed(ctx, form, pics, args, steps, warmup):
    for _ in range(warmup):
        call(ctx, form, pics, *args)
    ctx.synchronize()
    ctx.unpack_routes(reset=True)
    ctx.timer_begin()
    for _ in range(steps):
        call(ctx, form, pics, *args)
    ms = ctx.timer_end() / steps
    got = ctx.unpack_routes(reset=True)
    assert got == {"fused": steps * len(pics) if form == "fused" else 0, "two_pass": 0}, (form, got)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="every format, sample type and filter at 8 x 2160p")
    ap.add_argument("--configs", default=None)
    ap.add_argument("--out-prefix")
    a = ap.parse_args()
    assert a.rounds >= 5 and a.rounds * a.steps >= 100, "at least five rounds and 100 timed steps per form"
    ctx = sa.Context(0)
    rows = []

    def flush():
        lines = ["# scripts/unpack_iwt_ab.py: depth %d, ms per call, medians of %d rounds x %d calls" % (DEPTH, a.rounds, a.steps),
                 "# fused = schro_hip_unpack_iwt_batch on the FUSED route; two_pass = schro_hip_unpack_batch x 2 + schro_hip_iwt_batch;",
                 "# planar = schro_hip_iwt_batch over planes already on the device; spread = (max - min) / median over the rounds",
                 "%-11s %-12s %9s %9s %9s %8s %8s %8s %12s %12s" % ("config", "filter", "fused", "two_pass", "planar", "spr.fus", "spr.two",
                                                                 "spr.pla", "fused/two", "fused/planar")]
        for r in rows:
            lines.append("%-11s %-12s %9.4f %9.4f %9.4f %7.1f%% %7.1f%% %7.1f%% %12.2f %12.2f" % (
                r["config"], r["name"], r["fused_ms"], r["two_pass_ms"], r["planar_ms"], 100 * r["fused_spread"],
                100 * r["two_pass_spread"], 100 * r["planar_spread"], r["fused_ms"] / r["two_pass_ms"], r["fused_ms"] / r["planar_ms"]))
        text = "\n".join(lines) + "\n"
        if a.out_prefix:
            with open(a.out_prefix + ".jsonl", "w") as f:
                f.writelines(json.dumps(r) + "\n" for r in rows)
            with open(a.out_prefix + ".txt", "w") as f:
                f.write(text)
        return text

    configs = SWEEP if a.sweep else CONFIGS
    for (cname, fmt, own, w, h, npic, dtype, filters) in configs:
        if a.configs and cname not in a.configs.split(","):
            continue
        pics = pictures(ctx, fmt, own, w, h, npic, dtype, 11)
        for filt in filters:
            args = (fmt, w, h, filt)
            for form in ("two_pass", "fused", "planar"):
                call(ctx, form, pics, *args)
            ctx.synchronize()
            for n in (0, npic - 1):
                for k in range(3):
                    want = pics[n]["two_pass"][k].download()
                    assert np.array_equal(pics[n]["fused"][k].download(), want), (cname, filt, n, k, "fused")
                    assert np.array_equal(pics[n]["planar"][k].download(), want), (cname, filt, n, k, "planar")
            t = {f: [] for f in FORMS}
            for _ in range(a.rounds):
                for form in FORMS:
                    t[form].append(timed(ctx, form, pics, args, a.steps, a.warmup))
            med = {f: statistics.median(v) for f, v in t.items()}
            row = {"config": cname, "filter": filt, "name": NAMES[filt], "depth": DEPTH, "pictures": npic, "size": "%dx%d" % (w, h),
                   "type": np.dtype(dtype).name, "rounds": {f: [round(x, 4) for x in v] for f, v in t.items()}}
            for f in FORMS:
                row[f + "_ms"] = med[f]
                row[f + "_spread"] = (max(t[f]) - min(t[f])) / med[f]
            row["fused_slower_than_chain"] = (med["fused"] - med["two_pass"]) / med["two_pass"] > max(row["fused_spread"],
                                                                                                     row["two_pass_spread"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            flush()
        for p in pics:
            [q.free() for q in [p["packed"]] + p["own"] + p["frame"] + sum((p[f] for f in FORMS), [])]
    print(flush())
    ctx.close()


if __name__ == "__main__":
    main()
