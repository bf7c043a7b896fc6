#!/usr/bin/env python3
"""First numbers for the split-2 level of the mode decision on the device (mode_split2.hip), the stage behind the sub-pel
refinement.

Workload: 8 x 2160p 4:2:0 pictures, two references each, blocks every 16 x 16 samples (240 x 136 of them, the grid
scripts/subpel_ab.py has), extension 32, lambda 0.1, mv_precision 2.  The sub-pel fields hold the true motion plus or minus
a quarter sample and a metric of the size a 16 x 16 SAD has; the upsampled references (Y, U, V images each) are made on
the device.

  stage    schro_hip_split2_batch: the metric launch, then the choice launch, tables from the context's scratch;
  metric   schro_hip_split2_metric_batch alone: one wave per block over the blocks of all pictures;
  choose   schro_hip_split2_choose_batch alone: one workgroup per picture over the anti-diagonals.  (It reads no picture:
           its time depends on the grid alone.)
Device times are the stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps: medians
over `rounds` rounds and the spread (max - min) / median.  Before anything is timed the stage's motion fields and
superblock tables must equal what the single launches leave, and picture 0's first 8 block rows are compared with
tests/split2_ref.py on a crop that holds everything they read.  Not a gate: nothing reads the output.

  python scripts/split2_ab.py [--rounds 5] [--steps 3] [--out profiles/r19_split2.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import rough_hint_cases as T            # noqa: E402
import schroedinger_amd as sa           # noqa: E402

W, H, SEP, EXT, NPIC, NREF, LAMBDA, PREC = 3840, 2160, 16, 32, 8, 2, 0.1, 2
P = dict(x_num_blocks=4 * -(-W // (4 * SEP)), y_num_blocks=4 * -(-H // (4 * SEP)), xbsep_luma=SEP, ybsep_luma=SEP, mv_precision=PREC)
MOTIONS = [[(9 + n, -7), (-11, 5 + n)] for n in range(NPIC)]
SIZES = [(W, H), (W // 2, H // 2), (W // 2, H // 2)]


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


def field(n, r):
    rng = np.random.default_rng(100 * n + r)
    f = np.zeros(P["x_num_blocks"] * P["y_num_blocks"], sa.MV_DTYPE)
    f["flags"] = r + 1
    f["metric"] = rng.integers(400, 2400, f.size)
    f["v"][:, r] = (MOTIONS[n][r][0] << PREC) + rng.integers(-1, 2, f.size)
    f["v"][:, 2 + r] = (MOTIONS[n][r][1] << PREC) + rng.integers(-1, 2, f.size)
    return f


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

    nb = P["x_num_blocks"] * P["y_num_blocks"]
    say("# scripts/split2_ab.py: medians of %d rounds x %d calls (HIP events), %d warm-up calls per round; %d x %dx%d 4:2:0 pictures x %d "
        "references, blocks every %dx%d (%dx%d of them), extension %d, lambda %g, mv_precision %d"
        % (a.rounds, a.steps, a.warmup, NPIC, W, H, NREF, SEP, SEP, P["x_num_blocks"], P["y_num_blocks"], EXT, LAMBDA, PREC))
    # (one texture per component, rolled from picture to picture: the content does not matter to the time)
    base = [T.texture(w, h, 40 + k) for k, (w, h) in enumerate(SIZES)]
    pics = [[np.roll(base[k], (37 * n, 53 * n), (0, 1)) for k in range(3)] for n in range(NPIC)]
    refs = [[[T.moved(pics[n][k], dx >> (k > 0), dy >> (k > 0), 0, noise=0) for k in range(3)] for (dx, dy) in MOTIONS[n]] for n in range(NPIC)]
    d_pics = [[ctx.upload(p) for p in pics[n]] for n in range(NPIC)]
    hps = [[[ctx.hp_plane(h, w) for (w, h) in SIZES] for _ in range(NREF)] for _ in range(NPIC)]
    for n in range(NPIC):
        for r in range(NREF):
            tmp = [ctx.upload(refs[n][r][k]) for k in range(3)]
            ctx.upsample_batch([(tmp[k], hps[n][r][k]) for k in range(3)])
            ctx.synchronize()
            [t.free() for t in tmp]
    fields = [[field(n, r) for r in range(NREF)] for n in range(NPIC)]
    d_field = [[ctx.upload_bytes(fields[n][r]) for r in range(NREF)] for n in range(NPIC)]
    d_motion = [[ctx.motion_field(P) for _ in range(NPIC)] for _ in range(2)]
    d_sb = [[ctx.plane(1, nb, np.uint8, stride=nb) for _ in range(NPIC)] for _ in range(2)]     # 16 bytes per 16 blocks
    d_table = [ctx.plane(1, nb * sa.SPLIT2_TABLE_INTS, np.int32, stride=nb * 4 * sa.SPLIT2_TABLE_INTS) for _ in range(NPIC)]

    def pictures(out):
        return [(d_pics[n], hps[n], (1, 1), EXT, P, LAMBDA, d_field[n], d_motion[out][n], d_sb[out][n]) for n in range(NPIC)]

    # ---- the stage equals its launches one by one; the top of picture 0 equals the restatement
    ctx.split2_batch(pictures(0))
    ctx.split2_metric_batch(pictures(1), d_table)
    ctx.split2_choose_batch(pictures(1), d_table)
    ctx.synchronize()
    got = [ctx.download_field(d_motion[0][n]) for n in range(NPIC)]
    got_sb = [d_sb[0][n].download().reshape(-1).view(sa.SB_DTYPE) for n in range(NPIC)]
    for n in range(NPIC):
        assert got[n].tobytes() == ctx.download_field(d_motion[1][n]).tobytes(), ("stage against launches: motion", n)
        assert got_sb[n].tobytes() == d_sb[1][n].download().tobytes(), ("stage against launches: superblocks", n)
    import split2_ref as R
    rows = 8
    crop = rows * SEP + 64
    small = dict(P, y_num_blocks=rows, h_shift=1, v_shift=1)
    cut = lambda planes: [planes[0][:crop], planes[1][:crop // 2], planes[2][:crop // 2]]
    want, want_sb, _ = R.split2(cut(pics[0]), [cut(r) for r in refs[0]], small, LAMBDA, [f[:rows * P["x_num_blocks"]] for f in fields[0]], EXT)
    assert got[0][:rows * P["x_num_blocks"]].tobytes() == want.tobytes(), "restatement: motion"
    assert got_sb[0][:len(want_sb)].tobytes() == want_sb.tobytes(), "restatement: superblocks"
    modes = np.bincount(np.concatenate(got)["flags"] & 3, minlength=4)
    say("checked  the stage's %d motion fields and superblock tables equal the single launches', the first %d block rows of picture 0 equal "
        "tests/split2_ref.split2; pred_mode 0 / 1 / 2 / 3 chosen in %d / %d / %d / %d blocks" % (NPIC, rows, *modes))
    stage = pictures(0)
    med, spread = rounds_of(ctx, lambda: ctx.split2_batch(stage), a)
    say("stage    %d pictures x %d blocks: %9.4f ms per call  spread %4.1f%%  = %7.4f ms per picture" % (NPIC, nb, med, 100 * spread, med / NPIC))
    med, spread = rounds_of(ctx, lambda: ctx.split2_metric_batch(stage, d_table), a)
    say("metric   alone, %d waves of one block: %9.4f ms per launch  spread %4.1f%%  = %6.2f ns per block" % (nb * NPIC, med, 100 * spread,
                                                                                                       1e6 * med / (nb * NPIC)))
    diagonals = -(-W // SEP) + -(-H // SEP) - 1
    med, spread = rounds_of(ctx, lambda: ctx.split2_choose_batch(stage, d_table), a)
    say("choose   alone, %d workgroups, %d diagonals: %9.4f ms per launch  spread %4.1f%%  = %6.2f us per diagonal" % (NPIC, diagonals, med, 100 * spread,
                                                                                                                1e3 * med / diagonals))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
