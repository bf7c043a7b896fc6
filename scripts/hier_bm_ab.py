#!/usr/bin/env python3
"""First numbers for the hierarchical block matching on the device (hier_bm.hip), the default encoder's motion search.

Workload: 8 x 2160p 4:2:0 pictures x 2 references, blocks every 16 x 16 samples (240 x 135 of them), 5 pyramid levels of
all three components made on the device (schro_hip_downsample_batch, aprons of 32).

  chain     schro_hip_hbm_batch: levels 5 .. 1 (h_range 20, 10, 5, 3, 3) of every (picture, reference) chain in ONE launch,
            one workgroup per chain, the pyramid already there -- without level 0, and with it (h_range 3);
  level k   schro_hip_hbm_level_batch: level k alone for the 16 chains, under the chain's field of level k + 1 (level 5: no
            hint field).
Device times are the stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps: medians
over `rounds` rounds and the spread (max - min) / median.  Before anything is timed, levels 5 .. 2 of the chain of the first
picture and reference are compared with tests/hier_bm_ref.py record for record, and every level's own launch must
reproduce the chain's field of that level.  Not a gate: nothing reads the output.

  python scripts/hier_bm_ab.py [--rounds 5] [--steps 3] [--out profiles/r17_hier_bm.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import hier_bm_ref as R                 # noqa: E402
import rough_hint_cases as T            # noqa: E402
import schroedinger_amd as sa           # noqa: E402

W, H, SEP, LEVELS, EXT, NPIC, NREF = 3840, 2160, 16, 5, 32, 8, 2
P = dict(x_num_blocks=4 * -(-W // (4 * SEP)), y_num_blocks=4 * -(-H // (4 * SEP)), xbsep_luma=SEP, ybsep_luma=SEP)
CHECKED_DOWN_TO = 2             # the restatement takes about a minute for level 1 and four for level 0


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


def picture(n):
    """(Y, U, V) of picture n, 4:2:0."""
    return tuple(T.texture(W >> (k > 0), H >> (k > 0), 40 + 10 * n + k) for k in range(3))


def reference_of(frame, dx, dy):
    return tuple(T.moved(p, dx >> (k > 0), dy >> (k > 0), 0, noise=0) for k, p in enumerate(frame))


def device_pyramids(ctx, pictures):
    """levels[k][p]: the (Y, U, V) views of picture p at level k inside planes with their apron, one downsample call per level."""
    srcs = [[ctx.upload(c) for c in pic] for pic in pictures]
    keep = [c for pic in srcs for c in pic]
    levels = [srcs]
    for _ in range(LEVELS):
        dsts = [[ctx.plane((c.height + 1) // 2 + 2 * EXT, (c.width + 1) // 2 + 2 * EXT, np.uint8) for c in pic] for pic in srcs]
        ctx.downsample_batch([(s, d, EXT) for ps, pd in zip(srcs, dsts) for s, d in zip(ps, pd)])
        srcs = [[sa.SubPlane(d, EXT, EXT, (s.height + 1) // 2, (s.width + 1) // 2) for s, d in zip(ps, pd)] for ps, pd in zip(srcs, dsts)]
        levels.append(srcs)
        keep += [c for pic in dsts for c in pic]
    return levels, keep


def grid(k):
    return -(-P["x_num_blocks"] >> k), -(-P["y_num_blocks"] >> k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = sa.Context(0)
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say("# scripts/hier_bm_ab.py: medians of %d rounds x %d calls (HIP events), %d warm-up calls per round; %d x %dx%d 4:2:0 x %d references, "
        "blocks every %dx%d (%dx%d of them), %d levels" % (a.rounds, a.steps, a.warmup, NPIC, W, H, NREF, SEP, SEP, P["x_num_blocks"],
                                                            P["y_num_blocks"], LEVELS))
    frames = [picture(n) for n in range(NPIC)]
    refs = [[reference_of(f, 9 + n, -7), reference_of(f, -11, 5 + n)] for n, f in enumerate(frames)]
    fl, keep = device_pyramids(ctx, frames)
    rl = []
    for r in range(NREF):
        lv, k2 = device_pyramids(ctx, [refs[n][r] for n in range(NPIC)])
        rl.append(lv)
        keep += k2
    fields = [[[ctx.motion_field(P) for _ in range(LEVELS + 1)] for _ in range(NPIC)] for _ in range(NREF)]

    def chains():
        return [([(fl[k][n], rl[r][k][n], EXT) for k in range(LEVELS + 1)], 1, 1, P, r, fields[r][n]) for r in range(NREF) for n in range(NPIC)]

    # ---- the chain is the restatement's, record for record (first picture, first reference, the levels a minute pays for)
    ctx.hbm_batch(chains(), True)
    ctx.synchronize()
    fpyr, rpyr = R.pyramid3(frames[0], LEVELS), R.pyramid3(refs[0][0], LEVELS)
    ranges = R.chain_ranges(LEVELS)
    want = None
    for k in range(LEVELS, CHECKED_DOWN_TO - 1, -1):
        want = R.hbm_scan_hint(fpyr[k], rpyr[k], P, k, ranges[k], 0, want, 1, 1, EXT)
        assert ctx.download_field(fields[0][0][k]).tobytes() == want.tobytes(), ("chain", k)
    say("checked  levels %d .. %d of the chain of picture 0, reference 0 equal tests/hier_bm_ref.hbm_scan_hint on the numpy pyramid"
        % (LEVELS, CHECKED_DOWN_TO))
    chain_fields = [[[ctx.download_field(fields[r][n][k]) for k in range(LEVELS + 1)] for n in range(NPIC)] for r in range(NREF)]

    c = chains()
    for with_level0 in (False, True):
        first = 0 if with_level0 else 1
        blocks = sum(grid(k)[0] * grid(k)[1] for k in range(first, LEVELS + 1))
        diagonals = sum(grid(k)[0] + grid(k)[1] - 1 for k in range(first, LEVELS + 1))
        med, spread = rounds_of(ctx, lambda: ctx.hbm_batch(c, with_level0), a)
        say("chain    %d chains (%d pictures x %d references), levels %d .. %d, %d blocks and %d barriers per chain: %9.4f ms per launch  "
            "spread %4.1f%%  = %7.4f ms per picture" % (len(c), NPIC, NREF, LEVELS, first, blocks, diagonals + 1, med, 100 * spread, med / NPIC))
    for shift in range(LEVELS, -1, -1):
        out = [[ctx.motion_field(P) for _ in range(NPIC)] for _ in range(NREF)]
        entries = [(fl[shift][n], rl[r][shift][n], EXT, 1, 1, P, shift, ranges[shift], r, fields[r][n][shift + 1] if shift < LEVELS else None, out[r][n])
                   for r in range(NREF) for n in range(NPIC)]
        ctx.hbm_level_batch(entries)
        ctx.synchronize()
        for r in range(NREF):
            for n in range(NPIC):
                assert ctx.download_field(out[r][n]).tobytes() == chain_fields[r][n][shift].tobytes(), ("level", shift, r, n)
        med, spread = rounds_of(ctx, lambda: ctx.hbm_level_batch(entries), a)
        gx, gy = grid(shift)
        say("level %d  %d entries, level %d alone (%dx%d luma, h_range %2d, %5d blocks, %3d diagonals): %9.4f ms per launch  spread %4.1f%%  "
            "= %6.2f us per diagonal" % (shift, len(entries), shift, fl[shift][0][0].width, fl[shift][0][0].height, ranges[shift], gx * gy,
                                         gx + gy - 1, med, 100 * spread, 1e3 * med / (gx + gy - 1)))
        [p.free() for row in out for p in row]
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
