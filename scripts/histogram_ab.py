#!/usr/bin/env python3
"""First numbers for the sub-band histograms (hist.hip) beside the quantiser they feed.

8 x 2160p 4:2:0 s16 pictures (24 planes, 240 bands per call), transform depth 3, one schro_hip_histogram_batch call -- the
bands, skips and forms of schro_encoder_generate_subband_histograms for inter pictures (every band the plain form) -- on
two inputs:

  (a) natural  the forward DD(9,7) wavelet (schro_hip_iwt_batch) of natural-like pictures (tests/synth.py picture_u8,
               blurred noise, blurred twice more): most coefficients are zero or tiny, so the lanes of a wave meet on the
               lowest bins;
  (b) uniform  values uniform over s16: the lanes spread over all bins, the highest (2048 values wide) the fullest.
Each beside its byte floor (the sampled rows only, recomputed here from the band table) and beside
schro_hip_quantise_batch (inter, the stream's default codeblock counts) on the same pictures in the same run.  Then the
frame-layer call for ONE picture on the host clock, copy back and scale included, beside the download of the coefficient
frame it replaces.

Times: device events around `steps` calls (Context.timer_begin / timer_end -- the histogram launch has no profile class),
per call; the median of `rounds` rounds after `warmup` calls, and the spread (max - min) / median.  The counts of the first
call are compared with tests/hist_ref.py on one luma and one chroma plane before anything is timed.

With SCHRO_HIP_LIB = the experiments library every form is timed: SCHRO_HIP_HIST_HOT = 0 (every sample an LDS atomic), 4
(the product: bins 0 .. 3 in registers) and 8.

  python scripts/histogram_ab.py [--rounds 5] [--steps 20] [--out profiles/r14_histogram.txt]"""
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
import hist_ref as H                    # noqa: E402
import quant_cases as QC                # noqa: E402
import schroedinger_amd as sa           # noqa: E402
import synth                            # noqa: E402
from schroedinger_amd import _lib, frames       # noqa: E402

NPIC, W, Hh, DEPTH, FILT = 8, 3840, 2160, 3, 0
INTER = ([1, 1, 8, 12], [1, 1, 6, 8])
COMPS = [(Hh, W), (Hh // 2, W // 2), (Hh // 2, W // 2)]


def band_table(stride, w, h, intra=0):
    return [H.band_rect(w, h, DEPTH, i, stride, 2) + (H.band_skip(i), int(bool(intra) and i == 0)) for i in range(1 + 3 * DEPTH)]


def sampled_bytes(bands):
    return sum(2 * bd[2] * len(range(0, bd[3], bd[4])) for bd in bands)


def timed(ctx, fn, a):
    """median ms per call over the rounds, and the spread"""
    rows = []
    for _ in range(a.rounds):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.timer_begin()
        for _ in range(a.steps):
            fn()
        rows.append(ctx.timer_end() / a.steps)
    med = statistics.median(rows)
    return med, (max(rows) - min(rows)) / med


def natural_like(h, w, seed):
    p = synth.picture_u8(h, w, seed=seed, blur=True).astype(np.int32)
    for _ in range(2):
        q = np.pad(p, 1, mode="edge")
        p = sum(q[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) // 9
    return (p - 128).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    experiments = "exp" in os.path.basename(_lib.LIB_PATH)
    rng = np.random.default_rng(1)
    co = [ctx.plane(*COMPS[k % 3], np.int16) for k in range(3 * NPIC)]
    qu = [ctx.plane(p.height, p.width, np.int16, stride=p.stride) for p in co]
    bands = [band_table(co[k].stride, COMPS[k % 3][1], COMPS[k % 3][0]) for k in range(3 * NPIC)]
    floor = sum(sampled_bytes(b) for b in bands)
    samples = NPIC * sum(h * w for h, w in COMPS)
    lines = ["histogram_ab: %d x %dx%d 4:2:0 s16, depth %d, %d bands per call%s" % (NPIC, W, Hh, DEPTH, sum(len(b) for b in bands),
                                                                                   ", experiments library" if experiments else ""),
             "byte floor: the sampled rows of every band = %d bytes (%.1f MB) of the %.1f MB of coefficients; at 8 TB/s (HBM peak) %.4f ms, "
             "at the 6.29 TB/s a copy reaches %.4f ms" % (floor, floor / 1e6, 2 * samples / 1e6, floor / 8e12 * 1e3, floor / 6.29e12 * 1e3)]
    arr, counts, block = ctx.histogram_planes([(co[k], bands[k]) for k in range(3 * NPIC)])

    def histogram():
        sa.check(ctx.lib.schro_hip_histogram_batch(ctx.h, arr, 3 * NPIC, 2))

    qjobs = []
    for k in range(3 * NPIC):
        h, w = COMPS[k % 3]
        recs = QC.layout(w, h, DEPTH, INTER[0], INTER[1], co[k].stride, 2)
        for n, r in enumerate(recs):
            r[4] = 12 + (n % 9)
        qjobs.append((co[k], qu[k], QC.table(recs), 0, None))

    def quantise():
        [s.free() for s in ctx.quantise_batch(qjobs)]

    inputs = {}
    pics = [natural_like(*COMPS[k], seed=5 + k) for k in range(3)]
    src = [ctx.upload(pics[k % 3]) for k in range(3)]
    one = [ctx.plane(*COMPS[k], np.int16) for k in range(3)]
    ctx.iwt_batch([(src[k], one[k]) for k in range(3)], DEPTH, FILT)
    inputs["natural"] = [p.download() for p in one]
    inputs["uniform"] = [rng.integers(-32768, 32768, s).astype(np.int16) for s in COMPS]
    res = {}
    for name, host in inputs.items():
        for k, p in enumerate(co):
            p.upload(host[k % 3])
        histogram()
        for k in (0, 1):
            pitch = co[k].stride // 2
            buf = np.zeros((co[k].height, pitch), np.int16)
            buf[:, :co[k].width] = host[k]
            want = np.stack([H.counts(np.lib.stride_tricks.as_strided(buf.reshape(-1)[bd[0] // 2:], (bd[3], bd[2]), (bd[1], 2)), bd[4], bd[5])
                             for bd in bands[k]])
            got = counts[k].download()
            assert np.array_equal(got, want), (name, k)
        low = sum(int(counts[k].download()[:, :4].sum()) for k in range(3))
        tot = sum(int(counts[k].download().sum()) for k in range(3))
        lines.append("%s: checked against tests/hist_ref.py (planes 0 and 1); %.1f %% of the sampled values in bins 0 .. 3" % (name, 100.0 * low / tot))
        forms = (("0", "every sample an LDS atomic"), ("4", "bins 0 .. 3 in registers: the product"), ("8", "bins 0 .. 7 in registers")) \
            if experiments else ((None, "the product: bins 0 .. 3 in registers"),)
        for hot, what in forms:
            if hot is not None:
                os.environ["SCHRO_HIP_HIST_HOT"] = hot
            t, spread = timed(ctx, histogram, a)
            res[(name, hot)] = t
            lines.append("histogram %s [%s]: %.4f ms per call (%.2f TB/s of sampled bytes; %.2f x the 8 TB/s floor), spread %.1f %%"
                         % (name, what, t, floor / (t * 1e-3) / 1e12, t / (floor / 8e12 * 1e3), 100 * spread))
        os.environ.pop("SCHRO_HIP_HIST_HOT", None)
        tq, spread = timed(ctx, quantise, a)        # (last: it writes the reconstruction over the coefficients)
        res[(name, "q")] = tq
        lines.append("quantise %s (inter, same planes, same run, the same timer; summaries allocated per call as scripts/quantise_ab.py "
                     "does): %.4f ms per call, spread %.1f %%" % (name, tq, 100 * spread))
        key = (name, "4" if experiments else None)
        lines.append("ratio histogram / quantise on %s: %.2f (bytes: %.1f MB read against %.1f MB read and written)"
                     % (name, res[key] / tq, floor / 1e6, 6.0 * samples / 1e6))
    key = "4" if experiments else None
    lines.append("ratio natural / uniform (the price of the lanes meeting on the low bins; below 1: the spread over the LDS bins costs more): %.2f"
                 % (res[("natural", key)] / res[("uniform", key)]))

    # the frame layer, ONE picture, on the host clock
    fmt = frames.frame_format(np.int16, 1, 1)
    dev = frames.DeviceFrame(ctx, fmt, W, Hh).upload(frames.HostFrame(inputs["natural"], 1, 1))
    params = frames.make_params(transform_depth=DEPTH, num_refs=1, iwt_luma_width=W, iwt_luma_height=Hh, iwt_chroma_width=W // 2,
                                iwt_chroma_height=Hh // 2)
    nh = 3 * (1 + 3 * DEPTH)
    hists, ovf = (_lib.Histogram * nh)(), (C.c_uint32 * nh)()

    def host_clock(fn):
        rows = []
        for _ in range(a.rounds):
            for _ in range(a.warmup):
                fn()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            ctx.synchronize()
            rows.append((time.perf_counter() - t0) / a.steps * 1e3)
        med = statistics.median(rows)
        return med, (max(rows) - min(rows)) / med

    t, spread = host_clock(lambda: sa.check(ctx.lib.schro_hipframe_subband_histograms(dev.ptr(), C.byref(params), hists, ovf)))
    wn, wbins, wovf = H.frame_histograms(inputs["natural"], DEPTH, 0)
    assert [h.n for h in hists] == wn.tolist() and np.array_equal(np.array([list(h.bins) for h in hists]), wbins)
    lines.append("frame layer, one picture: schro_hipframe_subband_histograms %.4f ms per call on the host clock (launch, %d bytes copied "
                 "back, wait, scale to doubles), spread %.1f %%; equal to tests/hist_ref.py" % (t, nh * C.sizeof(_lib.HistogramCounts), 100 * spread))
    host_frame = frames.HostFrame([np.zeros(s, np.int16) for s in COMPS], 1, 1)
    td, spread = host_clock(lambda: sa.check(ctx.lib.schro_hipframe_to_cpu(host_frame.ptr(), dev.ptr())))
    lines.append("the download it replaces: schro_hipframe_to_cpu of the coefficient frame (%.1f MB, pageable host memory) %.4f ms per call, "
                 "spread %.1f %%" % (2 * sum(h * w for h, w in COMPS) / 1e6, td, 100 * spread))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
