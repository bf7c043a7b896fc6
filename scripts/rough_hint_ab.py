#!/usr/bin/env python3
"""First numbers for the rough motion search on the device (rough_hint.hip).

Workload: 8 x 2160p luma, 8 x 8 blocks (480 x 270 of them), 5 pyramid levels made on the device (schro_hip_downsample_batch,
aprons of 32), one and two references per picture.

  chain     schro_hip_rough_me_batch: the nohint level at 5 (distance 12) and the hint levels 4 .. 1 (distance 4) of every
            (picture, reference) chain in ONE launch, one workgroup per chain, the pyramid already there;
  hint k    schro_hip_rough_hint_batch: level k alone for the 8 pictures, under the chain's field of level k + 1;
and, in the same run, what the library could do before it had the kernel:
  nohint    schro_rough_me_heirarchical_scan_nohint_hip on level 5 of one picture (host clock: the call builds the
            descriptors, runs the scan batch, waits and fills the vectors);
  scans     level 1's 32 400 scans per picture through schro_hip_metric_scan_batch with host-built descriptors, all 8
            pictures in one call (windows around the chain's own winners).  A LOWER BOUND on a host-driven hint level: it
            leaves out the candidate tests and the 374 host round trips (one per anti-diagonal) the dependency would force,
            each with its own descriptor table.  Host clock (call + wait) and device time.
Device times are the stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps: medians
over `rounds` rounds and the spread (max - min) / median; host clocks are medians of rounds x steps calls, each waited for.
Before anything is timed the chain of the first picture is compared with tests/rough_hint_ref.py, record for record.

  python scripts/rough_hint_ab.py [--rounds 5] [--steps 5] [--out profiles/r16_rough_hint.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import analysis_ref as A                # noqa: E402
import rough_hint_cases as K            # noqa: E402
import rough_hint_ref as R              # noqa: E402
import schroedinger_amd as sa           # noqa: E402
from schroedinger_amd import _lib      # noqa: E402

W, H, SEP, LEVELS, EXT, NPIC = 3840, 2160, 8, 5, 32, 8
P = dict(x_num_blocks=W // SEP, y_num_blocks=H // SEP, xbsep_luma=SEP, ybsep_luma=SEP)


def timed(ctx, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    ctx.timer_begin()
    for _ in range(steps):
        fn()
    return ctx.timer_end() / steps


def rounds_of(ctx, fn, a):
    t = [timed(ctx, fn, a.steps, a.warmup) for _ in range(a.rounds)]
    med = statistics.median(t)
    return med, (max(t) - min(t)) / med


def host_clock(ctx, fn, a):
    t = []
    for _ in range(a.rounds * a.steps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), len(t)


def device_pyramids(ctx, planes):
    """levels[k][p]: picture p at level k (k >= 1: a view inside a plane with its apron), one downsample call per level."""
    levels, srcs = [None], [ctx.upload(p) for p in planes]
    keep = list(srcs)
    for _ in range(LEVELS):
        dsts = [ctx.plane((s.height + 1) // 2 + 2 * EXT, (s.width + 1) // 2 + 2 * EXT, np.uint8) for s in srcs]
        ctx.downsample_batch([(s, d, EXT) for s, d in zip(srcs, dsts)])
        srcs = [sa.SubPlane(d, EXT, EXT, (s.height + 1) // 2, (s.width + 1) // 2) for s, d in zip(srcs, dsts)]
        levels.append(srcs)
        keep += dsts
    return levels, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = sa.Context(0)
    lines = ["# scripts/rough_hint_ab.py: medians of %d rounds x %d calls (HIP events), %d warm-up calls per round; %d x %dx%d luma, %dx%d blocks, "
             "%d levels" % (a.rounds, a.steps, a.warmup, NPIC, W, H, SEP, SEP, LEVELS)]
    frames = [K.texture(W, H, 40 + n) for n in range(NPIC)]
    refs = [[K.moved(f, 9 + n, -7, 0, noise=0), K.moved(f, -11, 5 + n, 0, noise=0)] for n, f in enumerate(frames)]
    fl, keep = device_pyramids(ctx, frames)
    rl = []
    for r in (0, 1):
        lv, k2 = device_pyramids(ctx, [refs[n][r] for n in range(NPIC)])
        rl.append(lv)
        keep += k2
    fields = [[[ctx.motion_field(P) for _ in range(LEVELS)] for _ in range(NPIC)] for _ in (0, 1)]

    def chains(nrefs):
        return [([(fl[k][n], rl[r][k][n], EXT) for k in range(1, LEVELS + 1)], P, r, fields[r][n]) for r in range(nrefs) for n in range(NPIC)]

    # ---- the chain is the restatement's, record for record (first picture, first reference)
    ctx.rough_me_batch(chains(2))
    ctx.synchronize()
    want = R.rough_scan(A.pyramid(frames[0], LEVELS), A.pyramid(refs[0][0], LEVELS), P, LEVELS, 0, EXT)
    for k in range(1, LEVELS + 1):
        assert ctx.download_field(fields[0][0][k - 1]).tobytes() == want[k].tobytes(), ("chain", k)
    lines.append("checked  the chain of picture 0, reference 0 equals tests/rough_hint_ref.rough_scan on analysis_ref.pyramid at all %d levels"
                 % LEVELS)

    diagonals = sum(-(-P["x_num_blocks"] >> k) + -(-P["y_num_blocks"] >> k) - 1 for k in range(1, LEVELS))
    blocks = sum((-(-P["x_num_blocks"] >> k)) * (-(-P["y_num_blocks"] >> k)) for k in range(1, LEVELS + 1))
    for nrefs in (1, 2):
        c = chains(nrefs)
        med, spread = rounds_of(ctx, lambda: ctx.rough_me_batch(c), a)
        lines.append("chain    %d chains (%d pictures x %d reference%s), levels 5 .. 1, %d blocks and %d barriers per chain: %9.4f ms per launch  "
                     "spread %4.1f%%  = %7.4f ms per picture" % (len(c), NPIC, nrefs, "s" if nrefs > 1 else "", blocks, diagonals + LEVELS, med,
                                                                 100 * spread, med / NPIC))
    for shift in range(LEVELS - 1, 0, -1):
        out = [ctx.motion_field(P) for _ in range(NPIC)]
        pics = [(fl[shift][n], rl[0][shift][n], EXT, P, shift, 4, 0, fields[0][n][shift], out[n]) for n in range(NPIC)]
        ctx.rough_hint_batch(pics)
        ctx.synchronize()
        assert ctx.download_field(out[0]).tobytes() == want[shift].tobytes(), ("hint", shift)
        med, spread = rounds_of(ctx, lambda: ctx.rough_hint_batch(pics), a)
        nb = (-(-P["x_num_blocks"] >> shift)) * (-(-P["y_num_blocks"] >> shift))
        nd = -(-P["x_num_blocks"] >> shift) + -(-P["y_num_blocks"] >> shift) - 1
        lines.append("hint %d   %d pictures, level %d alone (%dx%d, %d blocks, %d diagonals): %9.4f ms per launch  spread %4.1f%%  = %6.2f us per diagonal"
                     % (shift, NPIC, shift, fl[shift][0].width, fl[shift][0].height, nb, nd, med, 100 * spread, 1e3 * med / nd))
        [p.free() for p in out]

    # ---- what the library could do without the kernel
    top_f, top_r = ctx.upload(A.edgeextend(A.pyramid(frames[0], LEVELS)[LEVELS], EXT)), ctx.upload(A.edgeextend(A.pyramid(refs[0][0], LEVELS)[LEVELS], EXT))
    got = ctx.rough_scan_nohint(top_f, top_r, P, LEVELS, 12, 0, extension=EXT)
    assert got.tobytes() == want[LEVELS].tobytes()
    med, lo, n = host_clock(ctx, lambda: ctx.rough_scan_nohint(top_f, top_r, P, LEVELS, 12, 0, extension=EXT), a)
    lines.append("nohint   schro_rough_me_heirarchical_scan_nohint_hip, level %d of ONE picture (%d scans): %9.4f ms per call (host clock, median of %d; "
                 "min %.4f)" % (LEVELS, (-(-P["x_num_blocks"] >> LEVELS)) * (-(-P["y_num_blocks"] >> LEVELS)), med, n, lo))

    # level 1's scans, windows around the chain's winners (>> 1), all pictures in one call
    lw, lh = fl[1][0].width, fl[1][0].height
    t0 = time.perf_counter()
    scans = []
    f1 = want[1]
    for j in range(0, P["y_num_blocks"], 2):
        for i in range(0, P["x_num_blocks"], 2):
            x, y = (i >> 1) * SEP, (j >> 1) * SEP
            bw, bh = min(SEP, lw - x), min(SEP, lh - y)
            dx, dy = int(f1[j * P["x_num_blocks"] + i]["v"][0]) >> 1, int(f1[j * P["x_num_blocks"] + i]["v"][2]) >> 1
            rx, ry, sw, sh = A.scan_setup(x, y, bw, bh, lw, lh, EXT, dx, dy, 4)
            scans.append((x, y, bw, bh, rx, ry, sw, sh, dx, dy, dx, dy))
    scans = np.array(scans, np.int32).view(sa.SCAN_DTYPE).reshape(-1)
    build = (time.perf_counter() - t0) * 1e3
    res = [ctx.plane(len(scans), 4, np.int32, stride=16) for _ in range(NPIC)]
    pic = (_lib.MetricScanPicture * NPIC)(*[_lib.MetricScanPicture(fl[1][n].ptr, fl[1][n].stride, rl[0][1][n].ptr, rl[0][1][n].stride, lw, lh, EXT,
                                                                    scans.ctypes.data_as(C.POINTER(_lib.MetricScan)), len(scans), res[n].ptr, None)
                                            for n in range(NPIC)])

    def run():
        sa.check(ctx.lib.schro_hip_metric_scan_batch(ctx.h, pic, NPIC))

    run()
    got = res[0].download()
    blocks1 = [(i, j) for j in range(0, P["y_num_blocks"], 2) for i in range(0, P["x_num_blocks"], 2)]
    for k in range(0, len(scans), 997):
        i, j = blocks1[k]
        mv = f1[j * P["x_num_blocks"] + i]
        # (the window lies around the winner, not around the chain's start vector: it holds positions the chain never saw,
        # so the scan may find a smaller metric than the chain's -- never a larger one, the winner is its gravity position)
        assert int(got[k][2]) <= int(mv["metric"]), ("scans", k)
        if int(got[k][2]) == int(mv["metric"]):
            assert (int(got[k][0]) << 1, int(got[k][1]) << 1) == (int(mv["v"][0]), int(mv["v"][2])), ("scans", k)
    med, spread = rounds_of(ctx, run, a)
    hmed, hlo, n = host_clock(ctx, run, a)
    lines.append("scans    level 1 through schro_hip_metric_scan_batch, %d pictures x %d scans in one call (descriptor table %.1f MB): %9.4f ms device  "
                 "spread %4.1f%%; %9.4f ms host clock, call + wait (median of %d; min %.4f)"
                 % (NPIC, len(scans), NPIC * len(scans) * 64 / 1e6, med, 100 * spread, hmed, n, hlo))
    lines.append("         (its descriptors took %.0f ms to build in Python, once, for one picture; not in the figures above)" % build)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
