#!/usr/bin/env python3
"""First numbers for the picture statistics (picture_sums.hip, lowpass2.hip, ssim.hip) on 8 x 3840x2160 4:2:0 pictures:

  sums      schro_hip_plane_sums_batch over the 24 planes (the sum of every plane) and over the 24 planes against those of a
            second set of pictures (sum and squared error: what enable_psnr reads);
  lowpass   schro_hip_lowpass2_batch, sigma 5 on the luma and 2.5 on the chroma (schro_frame_filter_lowpass2 (frame, 5) of
            4:2:0), the 24 u8 planes in one call, in place;
  ssim      schro_hip_ssim_batch over the 8 luma pairs, without and with the per-pixel maps;
  download  what they replace: the 8 pictures (99.5 MB) copied to pinned host memory over the bus, enqueued on one queue.
The device times are the stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps:
medians over `rounds` rounds and the spread (max - min) / median.  One small picture is compared with
tests/picture_stats_ref.py first.  Nothing is gated on these numbers.

  python scripts/picture_stats_ab.py [--rounds 5] [--steps 10] [--out profiles/picture_stats.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import picture_stats_cases as K         # noqa: E402
import picture_stats_ref as R           # noqa: E402
import schroedinger_amd as sa           # noqa: E402

NPIC, W, H = 8, 3840, 2160


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


def check_small(ctx):
    a, b = K.ssim_pair("noisy", 130, 67, 1)
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    assert [tuple(int(v) for v in r) for r in ctx.plane_sums_batch([(d_a, d_b)]).download()] == [R.plane_sums(a, b)]
    (res, m, _s), = ctx.ssim_batch([(d_a, d_b, True)])
    values, counts = R.ssim_map(a, b)
    assert np.array_equal(m.download(), values) and sa.Context.ssim_result(res)[1] == counts
    d_c = ctx.upload(a)
    ctx.lowpass2_batch([(d_c, 5, 2.5)])
    assert np.array_equal(d_c.download(), R.lowpass2(a, R.generate_coeff(5), R.generate_coeff(2.5))[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    check_small(ctx)
    lines = ["# scripts/picture_stats_ab.py: %d x %dx%d 4:2:0 u8; medians of %d rounds x %d calls (HIP events), %d warm-up calls per round"
             % (NPIC, W, H, a.rounds, a.steps, a.warmup)]
    shapes = [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
    base = [K.picture(w, h, 3 + k) for k, (h, w) in enumerate(shapes)]
    other = [np.clip(p.astype(np.int16) + 3, 0, 255).astype(np.uint8) for p in base]
    pa = [ctx.upload(base[k % 3]) for k in range(3 * NPIC)]
    pb = [ctx.upload(other[k % 3]) for k in range(3 * NPIC)]
    nbytes = NPIC * sum(h * w for h, w in shapes)

    res = ctx.plane(3 * NPIC, 2, np.int64, stride=16)
    rows = [res.rows_view(k, 1) for k in range(3 * NPIC)]
    for name, jobs, read in (("sums      24 planes, the sum", [(p, None, r) for p, r in zip(pa, rows)], nbytes),
                             ("sums      24 planes against 24, sum and squared error", [(p, q, r) for p, q, r in zip(pa, pb, rows)], 2 * nbytes)):
        ms, spread = rounds_of(ctx, lambda: ctx.plane_sums_batch(jobs), a)
        lines.append("%s: %8.4f ms per call  spread %4.1f%%  %6.1f MB read  = %.2f TB/s" % (name, ms, 100 * spread, read / 1e6, read / ms / 1e9))

    counter = ctx.plane(1, 1, np.uint32, stride=4).fill(0)
    planes = [(p, 5 if k % 3 == 0 else 2.5, 5 if k % 3 == 0 else 2.5, counter) for k, p in enumerate(pa)]
    ms, spread = rounds_of(ctx, lambda: ctx.lowpass2_batch(planes), a)
    lines.append("lowpass   24 planes in place, sigma 5 (chroma 2.5): %8.4f ms per call  spread %4.1f%%  %.2f G samples x passes / s"
                 % (ms, 100 * spread, 4 * nbytes / ms / 1e6))
    for k, p in enumerate(pa):                          # (the planes were filtered over and over: put the pictures back)
        p.upload(base[k % 3])

    scratch = [ctx.plane(1, sa.ssim_scratch_bytes(W, H), np.uint8) for _ in range(NPIC)]
    results = [ctx.plane(1, 32, np.uint8) for _ in range(NPIC)]
    maps = [ctx.plane(H, W, np.float64) for _ in range(NPIC)]
    for name, with_map in (("ssim      8 luma pairs", False), ("ssim      8 luma pairs + maps", True)):
        pics = [(pa[3 * k], pb[3 * k], maps[k] if with_map else None, scratch[k], results[k]) for k in range(NPIC)]
        ms, spread = rounds_of(ctx, lambda: ctx.ssim_batch(pics), a)
        lines.append("%s: %8.4f ms per call  spread %4.1f%%  = %.3f ms per picture" % (name, ms, 100 * spread, ms / NPIC))
    total, counts = sa.Context.ssim_result(results[0])
    lines.append("          (mssim of picture 0: %.6f, out of range %s)" % (total / (W * H), counts))

    host = [ctx.host_array((p.height, p.width), np.uint8) for p in pa]

    def download():
        for p, h in zip(pa, host):
            p.download_async(h)
    ms, spread = rounds_of(ctx, download, a)
    lines.append("download  the 8 pictures to pinned host memory (%.1f MB): %8.4f ms per call  spread %4.1f%%  = %.1f GB/s"
                 % (nbytes / 1e6, ms, 100 * spread, nbytes / ms / 1e6))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
