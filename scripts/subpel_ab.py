#!/usr/bin/env python3
"""First numbers for the sub-pel motion refinement on the device (subpel.hip), the stage behind the block matching's level 0.

Workload: the luma of 8 x 2160p pictures x 2 references = 16 chains, blocks every 16 x 16 samples (240 x 136 of them, the
grid scripts/hier_bm_ab.py has), extension 32, lambda 0.1, mv_precision 2 and 3.  The start fields hold the true motion
plus or minus one sample and a metric of the size a 16 x 16 SAD has; the upsampled references are made on the device.

  stage    schro_hip_subpel_batch: the copy of the 16 fields, then mv_precision x (error launch, choice launch);
  error p  schro_hip_subpel_error_batch: pass p alone, one wave per block over the blocks of all chains;
  choose p schro_hip_subpel_choose_batch: pass p alone, one workgroup per chain over the anti-diagonals.  (The choice
           rewrites its field, so call after call the vectors double; it reads no picture and scores all eight
           candidates of every block whatever they are, so its time does not depend on them.)
Device times are the stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps: medians
over `rounds` rounds and the spread (max - min) / median.  Before anything is timed the stage's fields must equal the
fields the single launches leave, pass by pass, and picture 0's first 6 block rows are compared with tests/subpel_ref.py
on a crop that holds everything they read.  Not a gate: nothing reads the output.

  python scripts/subpel_ab.py [--rounds 5] [--steps 3] [--out profiles/r18_subpel.txt]"""
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

W, H, SEP, EXT, NPIC, NREF, LAMBDA = 3840, 2160, 16, 32, 8, 2, 0.1
P = dict(x_num_blocks=4 * -(-W // (4 * SEP)), y_num_blocks=4 * -(-H // (4 * SEP)), xbsep_luma=SEP, ybsep_luma=SEP)
MOTIONS = [[(9 + n, -7), (-11, 5 + n)] for n in range(NPIC)]


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


def start_field(n, r):
    rng = np.random.default_rng(100 * n + r)
    f = np.zeros(P["x_num_blocks"] * P["y_num_blocks"], sa.MV_DTYPE)
    f["flags"] = r + 1
    f["metric"] = rng.integers(400, 2400, f.size)
    f["v"][:, r] = MOTIONS[n][r][0] + rng.integers(-1, 2, f.size)
    f["v"][:, 2 + r] = MOTIONS[n][r][1] + rng.integers(-1, 2, f.size)
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
    say("# scripts/subpel_ab.py: medians of %d rounds x %d calls (HIP events), %d warm-up calls per round; luma of %d x %dx%d x %d references = %d "
        "chains, blocks every %dx%d (%dx%d of them), extension %d, lambda %g" % (a.rounds, a.steps, a.warmup, NPIC, W, H, NREF, NPIC * NREF, SEP, SEP,
                                                                                 P["x_num_blocks"], P["y_num_blocks"], EXT, LAMBDA))
    pics = [T.texture(W, H, 40 + 10 * n) for n in range(NPIC)]
    refs = [[T.moved(pics[n], dx, dy, 0, noise=0) for (dx, dy) in MOTIONS[n]] for n in range(NPIC)]
    d_pics = [ctx.upload(p) for p in pics]
    hps = [[ctx.hp_plane(H, W) for _ in range(NREF)] for _ in range(NPIC)]
    for n in range(NPIC):
        tmp = [ctx.upload(refs[n][r]) for r in range(NREF)]
        ctx.upsample_batch([(tmp[r], hps[n][r]) for r in range(NREF)])
        ctx.synchronize()
        [t.free() for t in tmp]
    starts = [[start_field(n, r) for r in range(NREF)] for n in range(NPIC)]
    d_start = [[ctx.upload_bytes(starts[n][r]) for r in range(NREF)] for n in range(NPIC)]
    d_field = [[ctx.motion_field(P) for _ in range(NREF)] for _ in range(NPIC)]
    d_step = [[ctx.motion_field(P) for _ in range(NREF)] for _ in range(NPIC)]
    d_table = [[ctx.plane(1, nb * 8, np.int32, stride=nb * 32) for _ in range(NREF)] for _ in range(NPIC)]
    order = [(n, r) for r in range(NREF) for n in range(NPIC)]
    tables = [d_table[n][r] for n, r in order]

    def chains(prec, src, dst):
        return [(d_pics[n], hps[n][r], EXT, P, prec, r, LAMBDA, src[n][r] if src else None, dst[n][r]) for n, r in order]

    for prec in (2, 3):
        # ---- the stage equals its launches one by one; the top of picture 0 equals the restatement
        ctx.subpel_batch(chains(prec, d_start, d_field))
        ctx.subpel_batch(chains(0, d_start, d_step))
        for p in range(1, prec + 1):
            ctx.subpel_error_batch(chains(prec, None, d_step), p, tables)
            ctx.subpel_choose_batch(chains(prec, None, d_step), p, tables)
        ctx.synchronize()
        got = [[ctx.download_field(d_field[n][r]) for r in range(NREF)] for n in range(NPIC)]
        for n, r in order:
            assert got[n][r].tobytes() == ctx.download_field(d_step[n][r]).tobytes(), ("stage against launches", prec, n, r)
        import subpel_ref as R
        rows, crop = 6, 6 * SEP + 64
        small = dict(P, y_num_blocks=rows)
        want, _ = R.subpel_deep(pics[0][:crop], refs[0][0][:crop], small, prec, 0, LAMBDA, starts[0][0][:rows * P["x_num_blocks"]], EXT)
        assert got[0][0][:rows * P["x_num_blocks"]].tobytes() == want.tobytes(), ("restatement", prec)
        say("checked  mv_precision %d: the stage's 16 fields equal the single launches', the first %d block rows of picture 0, reference 0 equal "
            "tests/subpel_ref.subpel_deep" % (prec, rows))
        moved = sum(int((got[n][r]["v"] != 2 ** prec * starts[n][r]["v"]).any(axis=1).sum()) for n, r in order)
        stage = chains(prec, d_start, d_field)
        med, spread = rounds_of(ctx, lambda: ctx.subpel_batch(stage), a)
        say("stage    mv_precision %d, %d chains x %d blocks, %d passes (%.1f%% of the vectors moved): %9.4f ms per call  spread %4.1f%%  = %7.4f ms per "
            "picture" % (prec, len(order), nb, prec, 100.0 * moved / (nb * len(order)), med, 100 * spread, med / NPIC))
        # ---- the launches of each pass alone, on the fields as the pass finds them
        ctx.subpel_batch(chains(0, d_start, d_step))
        total_e = total_c = 0.0
        for p in range(1, prec + 1):
            one = chains(prec, None, d_step)
            med, spread = rounds_of(ctx, lambda: ctx.subpel_error_batch(one, p, tables), a)
            total_e += med
            say("error %d  mv_precision %d, pass %d alone, %d waves of one block: %9.4f ms per launch  spread %4.1f%%  = %6.2f ns per block"
                % (p, prec, p, nb * len(order), med, 100 * spread, 1e6 * med / (nb * len(order))))
            # (the field of the timed choice drifts; a copy of it does the timing, the real one goes on to the next pass)
            ctx.subpel_batch(chains(0, d_step, d_field))
            drift = chains(prec, None, d_field)
            med, spread = rounds_of(ctx, lambda: ctx.subpel_choose_batch(drift, p, tables), a)
            total_c += med
            diagonals = -(-W // SEP) + -(-H // SEP) - 1
            say("choose %d mv_precision %d, pass %d alone, %d workgroups, %d diagonals: %9.4f ms per launch  spread %4.1f%%  = %6.2f us per diagonal"
                % (p, prec, p, len(order), diagonals, med, 100 * spread, 1e3 * med / diagonals))
            ctx.subpel_choose_batch(one, p, tables)
        say("sum      mv_precision %d: error launches %9.4f ms, choice launches %9.4f ms" % (prec, total_e, total_c))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
