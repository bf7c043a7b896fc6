#!/usr/bin/env python3
"""First numbers for the encoder-analysis path (analysis.hip): the downsample pyramid and the SAD scan.

  pyramid   five levels (schro_hip_downsample_batch, one call per level, aprons of 32) of 8 x 1080p and 8 x 2160p 4:2:0
            pictures, 24 planes per call; ms per pyramid and its byte floor -- every source sample read once, every destination
            sample (apron included) written once -- over that time as a fraction of 8 TB/s;
  scan      one schro_hip_metric_scan_batch over every 8 x 8 block of one 2160p luma plane at distance 4 (schro_hip_metric_scan_setup:
            9 x 9 windows inside the picture), without and with the metrics tables; positions x pixels per second;
  nohint    schro_rough_me_heirarchical_scan_nohint_hip at shift 5, distance 12 on level 5 of a 2160p picture (host clock: the
            call builds the descriptors, runs the batch, waits and fills the vectors).
The device times are the stream's elapsed time (HIP events) around `steps` calls after `warmup` more, divided by steps: medians
over `rounds` rounds and the spread (max - min) / median.  The results are compared with tests/analysis_ref.py first, on the
smallest planes and a sample of the scans.  CPU column: tests/analysis_ref.py with its inner loops on the reference's compiled
kernels (oracle/_ref/libschroorc_ref.so: downsample_orc, do_scan_orc) where they are built, else the numpy restatement -- the
output says which -- for one 1080p luma plane and 64 of the scans, one thread, Python row and position loops included.

  python scripts/analysis_ab.py [--rounds 5] [--steps 20] [--out profiles/r12_analysis.txt]"""
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
import oracle_lib as O                  # noqa: E402
import schroedinger_amd as sa           # noqa: E402
from schroedinger_amd import _lib      # noqa: E402

PEAK = 8e12
LEVELS, EXT, NPIC = 5, 32, 8


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


def pyramid(ctx, w, h, a, lines):
    comps = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    host = [A.picture(cw, ch, 3 + k) for k, (ch, cw) in enumerate(comps)]
    level0 = [ctx.upload(host[k % 3]) for k in range(3 * NPIC)]
    calls, keep, floor = [], list(level0), 0
    srcs, shapes = level0, [host[k % 3].shape for k in range(3 * NPIC)]
    for _ in range(LEVELS):
        dsts = [ctx.plane((sh[0] + 1) // 2 + 2 * EXT, (sh[1] + 1) // 2 + 2 * EXT, np.uint8) for sh in shapes]
        calls.append([(s, d, EXT) for s, d in zip(srcs, dsts)])
        floor += sum(sh[0] * sh[1] for sh in shapes) + sum(d.height * d.width for d in dsts)
        shapes = [((sh[0] + 1) // 2, (sh[1] + 1) // 2) for sh in shapes]
        srcs = [sa.SubPlane(d, EXT, EXT, sh[0], sh[1]) for d, sh in zip(dsts, shapes)]
        keep += dsts

    def run():
        for jobs in calls:
            ctx.downsample_batch(jobs)

    run()
    ctx.synchronize()
    want = A.pyramid(host[1], LEVELS)
    for n in range(LEVELS):
        assert np.array_equal(calls[n][1][1].download(), A.edgeextend(want[n + 1], EXT)), ("pyramid", w, h, n)
    med, spread = rounds_of(ctx, run, a)
    lines.append("pyramid  %d x %dx%d 4:2:0, %d levels, apron %d: %8.4f ms per pyramid  spread %4.1f%%  floor %6.1f MB  floor / time = %5.1f%% of 8 TB/s"
                 % (NPIC, w, h, LEVELS, EXT, med, 100 * spread, floor / 1e6, 100 * floor / (med * 1e-3) / PEAK))
    [p.free() for p in keep]


def block_scans(w, h, sep, dist, ext):
    out = []
    for y in range(0, h, sep):
        for x in range(0, w, sep):
            bw, bh = min(sep, w - x), min(sep, h - y)
            rx, ry, sw, sh = sa.metric_scan_setup(x, y, bw, bh, w, h, ext, 0, 0, dist)
            out.append((x, y, bw, bh, rx, ry, sw, sh, rx - x, ry - y, rx - x, ry - y))
    return np.array(out, np.int32).view(sa.SCAN_DTYPE).reshape(-1)


def scan(ctx, a, lines):
    w, h = 3840, 2160
    frame = A.picture(w, h, 1)
    ref = np.roll(frame, (1, -2), axis=(0, 1))
    df, dr = ctx.upload(frame), ctx.upload(ref)
    scans = block_scans(w, h, 8, 4, 0)
    work = int((scans["scan_width"].astype(np.int64) * scans["scan_height"] * scans["block_width"] * scans["block_height"]).sum())
    res = ctx.plane(len(scans), 4, np.int32, stride=16)
    met = ctx.plane(len(scans), 42 * 42, np.uint32, stride=4 * 42 * 42)
    for tables in (False, True):
        pic = (_lib.MetricScanPicture * 1)(_lib.MetricScanPicture(df.ptr, df.stride, dr.ptr, dr.stride, w, h, 0,
                                                                  scans.ctypes.data_as(C.POINTER(_lib.MetricScan)), len(scans), res.ptr,
                                                                  met.ptr if tables else None))

        def run():
            sa.check(ctx.lib.schro_hip_metric_scan_batch(ctx.h, pic, 1))

        run()
        got = res.download()
        for k in list(range(0, len(scans), 4001)) + [len(scans) - 1]:
            m = A.do_scan(frame, ref, scans[k])
            assert tuple(int(v) for v in got[k]) == A.get_min(m, scans[k]) + (0,), ("scan", k)
        med, spread = rounds_of(ctx, run, a)
        lines.append("scan     %d scans (every 8x8 block of %dx%d, distance 4)%s: %8.4f ms per batch  spread %4.1f%%  %7.1f G positions x pixels / s"
                     % (len(scans), w, h, " + tables" if tables else "", med, 100 * spread, work / (med * 1e-3) / 1e9))
    # the CPU column: 64 of the scans
    use_orc = O.ref_available()
    sample = scans[np.linspace(0, len(scans) - 1, 64).astype(int)]
    t0 = time.perf_counter()
    for s in sample:
        (A.do_scan_orc(frame[:256, :256], ref[:256, :256], dict(zip(s.dtype.names, (int(v) for v in s)), x=int(s["x"]) % 200, y=int(s["y"]) % 200,
                                                                  ref_x=int(s["x"]) % 200 - 4, ref_y=int(s["y"]) % 200 - 4, scan_width=9, scan_height=9), 8)
         if use_orc else A.do_scan(frame, ref, s))
    dt = (time.perf_counter() - t0) / len(sample)
    lines.append("scan     CPU (%s): %.3f ms per 8x8 scan of 9x9 positions, one thread = %.3f G positions x pixels / s"
                 % ("analysis_ref.do_scan_orc: orc_sad_8x8_u8 of oracle/_ref per position" if use_orc else "analysis_ref.do_scan: numpy",
                    dt * 1e3, 81 * 64 / dt / 1e9))
    [p.free() for p in (df, dr, res, met)]


def nohint(ctx, a, lines):
    w, h, shift = 3840, 2160, 5
    lw, lh = -(-w >> shift), -(-h >> shift)
    frame = A.picture(lw, lh, 2)
    ref = np.roll(frame, (1, 2), axis=(0, 1))
    pf, pr = ctx.upload(A.edgeextend(frame, EXT)), ctx.upload(A.edgeextend(ref, EXT))
    P = dict(x_num_blocks=w // 8, y_num_blocks=-(-h // 8), xbsep_luma=8, ybsep_luma=8)
    got = ctx.rough_scan_nohint(pf, pr, P, shift, 12, 0, extension=EXT)
    assert got.tobytes() == A.rough_scan_nohint(frame, ref, P, shift, 12, 0, extension=EXT).tobytes()
    t = []
    for _ in range(a.rounds * 4):
        t0 = time.perf_counter()
        ctx.rough_scan_nohint(pf, pr, P, shift, 12, 0, extension=EXT)
        t.append((time.perf_counter() - t0) * 1e3)
    n = -(-P["x_num_blocks"] >> shift) * -(-P["y_num_blocks"] >> shift)
    lines.append("nohint   shift %d, distance 12 on the %dx%d level of %dx%d (%d scans of up to 25x25 positions, %d records): %8.4f ms per call "
                 "(host clock, median of %d; min %.4f)" % (shift, lw, lh, w, h, n, len(got), statistics.median(t), len(t), min(t)))
    [p.free() for p in (pf, pr)]


def cpu_downsample(lines):
    src = A.picture(1920, 1080, 9)
    use_orc = O.ref_available()
    fn = A.downsample_orc if use_orc else A.downsample
    assert np.array_equal(fn(src), A.downsample(src))
    t0 = time.perf_counter()
    fn(src)
    dt = time.perf_counter() - t0
    lines.append("pyramid  CPU (%s): %.2f ms for one 1920x1080 plane, one level, one thread"
                 % ("analysis_ref.downsample_orc: orc_downsample_vert_u8 / _horiz_u8 of oracle/_ref per row" if use_orc
                    else "analysis_ref.downsample: numpy", dt * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = sa.Context(0)
    lines = ["# scripts/analysis_ab.py: medians of %d rounds x %d calls (HIP events), %d warm-up calls per round" % (a.rounds, a.steps, a.warmup)]
    pyramid(ctx, 1920, 1080, a, lines)
    pyramid(ctx, 3840, 2160, a, lines)
    cpu_downsample(lines)
    scan(ctx, a, lines)
    nohint(ctx, a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
