#!/usr/bin/env python3
"""First numbers for the whole mode decision on the device (mode_decision.hip), the stage behind the block matching and the
sub-pel refinement, beside the split-2 stage it grew out of on the same pictures in the same run.

Workload: 8 x 2160p 4:2:0 pictures, two references each, blocks every 16 x 16 samples (240 x 136 of them, the grid
scripts/subpel_ab.py has), extension 32, lambda 0.1, mv_precision 2.  The sub-pel fields hold the true motion plus or minus
a quarter sample and a metric of the size a 16 x 16 SAD has, the level-1 and level-2 fields the true motion plus or minus a
whole sample; the upsampled references (Y, U, V images each) are made on the device.

  stage    schro_hip_mode_decision_batch: the split-2 metric launch, the mode metric launch, the walk, tables from the
           context's scratch;
  metric   schro_hip_mode_metric_batch alone: both metric launches -- one wave per block, then 45 waves per superblock;
  choose   schro_hip_mode_choose_batch alone: one workgroup per picture over the anti-diagonals of superblocks, one wave
           per superblock.  (It reads pictures for the bi-reference trials of split 1 and split 0 only.)
  split2   schro_hip_split2_batch on the same pictures: the stage as it was before this one.
Device times are the stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps: medians
over `rounds` rounds and the spread (max - min) / median.  Before anything is timed the stage's motion fields and
superblock and trial tables and statistics must equal what the single launches leave, and picture 0's first row of
superblocks is compared with tests/mode_ref.py on a crop that holds everything it reads.  Not a gate: nothing reads the
output.  What the numbers do not say: the fields are synthetic and close to the truth, so the share of superblocks per
split and with it the number of bi-reference trials inside the walk are this workload's, not an encoder's.

  python scripts/mode_ab.py [--rounds 5] [--steps 3] [--out profiles/r20_mode.txt]"""
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


def level_field(n, r, level):
    rng = np.random.default_rng(1000 * level + 100 * n + r)
    f = np.zeros(P["x_num_blocks"] * P["y_num_blocks"], sa.MV_DTYPE)
    f["flags"] = r + 1
    f["metric"] = rng.integers(400, 2400, f.size)
    f["v"][:, r] = MOTIONS[n][r][0] + rng.integers(-1, 2, f.size)
    f["v"][:, 2 + r] = MOTIONS[n][r][1] + rng.integers(-1, 2, f.size)
    return f


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
    nsb = nb // 16
    say("# scripts/mode_ab.py: medians of %d rounds x %d calls (HIP events), %d warm-up calls per round; %d x %dx%d 4:2:0 pictures x %d "
        "references, blocks every %dx%d (%dx%d of them, %d superblocks), extension %d, lambda %g, mv_precision %d"
        % (a.rounds, a.steps, a.warmup, NPIC, W, H, NREF, SEP, SEP, P["x_num_blocks"], P["y_num_blocks"], nsb, EXT, LAMBDA, PREC))
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
    levels = [[[level_field(n, r, level) for r in range(NREF)] for n in range(NPIC)] for level in (1, 2)]
    d_field = [[ctx.upload_bytes(fields[n][r]) for r in range(NREF)] for n in range(NPIC)]
    d_level = [[[ctx.upload_bytes(levels[k][n][r]) for r in range(NREF)] for n in range(NPIC)] for k in (0, 1)]
    d_motion = [[ctx.motion_field(P) for _ in range(NPIC)] for _ in range(3)]
    d_sb = [[ctx.plane(1, nb, np.uint8, stride=nb) for _ in range(NPIC)] for _ in range(3)]     # 16 bytes per 16 blocks
    trial_bytes = nsb * 4 * sa.MODE_TRIAL_DTYPE.itemsize
    d_trials = [[ctx.plane(1, trial_bytes, np.uint8, stride=trial_bytes) for _ in range(NPIC)] for _ in range(2)]
    d_stats = [[ctx.plane(1, 3, np.float64, stride=24) for _ in range(NPIC)] for _ in range(2)]
    d_table = []
    for _ in range(NPIC):
        d_table.append(ctx.plane(1, nb * sa.SPLIT2_TABLE_INTS, np.int32, stride=nb * 4 * sa.SPLIT2_TABLE_INTS))
        d_table.append(ctx.plane(1, nsb * sa.MODE_TABLE_INTS, np.int32, stride=nsb * 4 * sa.MODE_TABLE_INTS))

    def pictures(out):
        return [(d_pics[n], hps[n], (1, 1), EXT, P, LAMBDA, d_field[n], d_level[0][n], d_level[1][n], d_motion[out][n], d_sb[out][n], d_trials[out][n],
                 d_stats[out][n]) for n in range(NPIC)]

    # ---- the stage equals its launches one by one; the top of picture 0 equals the restatement
    ctx.mode_decision_batch(pictures(0))
    ctx.mode_metric_batch(pictures(1), d_table)
    ctx.mode_choose_batch(pictures(1), d_table)
    ctx.synchronize()
    got = [ctx.download_field(d_motion[0][n]) for n in range(NPIC)]
    got_sb = [d_sb[0][n].download().reshape(-1).view(sa.SB_DTYPE) for n in range(NPIC)]
    got_trials = [d_trials[0][n].download().reshape(-1).view(sa.MODE_TRIAL_DTYPE).reshape(-1, 4) for n in range(NPIC)]
    for n in range(NPIC):
        assert got[n].tobytes() == ctx.download_field(d_motion[1][n]).tobytes(), ("stage against launches: motion", n)
        assert got_sb[n].tobytes() == d_sb[1][n].download().tobytes(), ("stage against launches: superblocks", n)
        assert got_trials[n].tobytes() == d_trials[1][n].download().tobytes(), ("stage against launches: trials", n)
        assert d_stats[0][n].download().tobytes() == d_stats[1][n].download().tobytes(), ("stage against launches: statistics", n)
    import mode_ref as M
    rows = 4
    crop = rows * SEP + 64
    small = dict(P, y_num_blocks=rows, h_shift=1, v_shift=1)
    cut = lambda planes: [planes[0][:crop], planes[1][:crop // 2], planes[2][:crop // 2]]
    top = rows * P["x_num_blocks"]
    want = M.mode_decision(cut(pics[0]), [cut(r) for r in refs[0]], small, LAMBDA, [f[:top] for f in fields[0]], [f[:top] for f in levels[0][0]],
                           [f[:top] for f in levels[1][0]], EXT)
    assert got[0][:top].tobytes() == want[0].tobytes(), "restatement: motion"
    assert got_sb[0][:len(want[1])].tobytes() == want[1].tobytes(), "restatement: superblocks"
    assert got_trials[0][:len(want[2])].tobytes() == want[2].tobytes(), "restatement: trials"
    splits = np.bincount(np.concatenate([(g["flags"][::4].reshape(P["y_num_blocks"], -1)[::4] >> 3) & 3 for g in got]).reshape(-1), minlength=3)
    say("checked  the stage's %d motion fields, superblock and trial tables and statistics equal the single launches', the first row of superblocks "
        "of picture 0 equals tests/mode_ref.mode_decision; of %d superblocks %.1f%% end at split 0, %.1f%% at split 1, %.1f%% at split 2"
        % (NPIC, nsb * NPIC, *(100.0 * splits / splits.sum())))
    stage = pictures(0)
    med, spread = rounds_of(ctx, lambda: ctx.mode_decision_batch(stage), a)
    say("stage    %d pictures x %d superblocks: %9.4f ms per call  spread %4.1f%%  = %7.4f ms per picture" % (NPIC, nsb, med, 100 * spread, med / NPIC))
    med, spread = rounds_of(ctx, lambda: ctx.mode_metric_batch(stage, d_table), a)
    say("metric   alone, %d + %d waves: %9.4f ms per call  spread %4.1f%%  = %6.2f us per superblock" % (nb * NPIC, 45 * nsb * NPIC, med, 100 * spread,
                                                                                                1e3 * med / (nsb * NPIC)))
    diagonals = P["x_num_blocks"] // 4 + P["y_num_blocks"] // 4 - 1
    med, spread = rounds_of(ctx, lambda: ctx.mode_choose_batch(stage, d_table), a)
    say("choose   alone, %d workgroups, %d diagonals of superblocks: %9.4f ms per launch  spread %4.1f%%  = %6.2f us per diagonal"
        % (NPIC, diagonals, med, 100 * spread, 1e3 * med / diagonals))
    old = [p[:7] + (d_motion[2][n], d_sb[2][n]) for n, p in enumerate(stage)]
    med, spread = rounds_of(ctx, lambda: ctx.split2_batch(old), a)
    say("split2   schro_hip_split2_batch on the same pictures: %9.4f ms per call  spread %4.1f%%" % (med, 100 * spread))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
