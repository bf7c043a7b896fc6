#!/usr/bin/env python3
"""First numbers for the arithmetic transform-data decoder (arith_dec.hip) beside what it replaces.

The workload is the reference's own stream (tests/golden/test_stream.drc: 100 pictures, 320 x 240 4:2:0 s16, depth 4), the
only real arithmetic-coded data there is without a slow Python writer, in calls of 1, 8 and 100 pictures (the first ones
in coded order).  In the same run, on the same pictures:

  schro_hip_arith_decode_batch      the whole call (the clear of the results, header, clear, decode), from the stream's
                                    bytes on the device into the coefficient planes: ms per call, bins per second and ns
                                    per bin from the results' `bins`, payload bytes per second;
  a tower per lane                  (experiments library only: SCHRO_HIP_ARDEC_PER_LANE=1) the same kernel with 64 towers
                                    per wave, the alternative shape;
  its launches one at a time        (experiments library only: SCHRO_HIP_ARDEC_STAGES = 1 header, 2 clear, 4 decode);
  the upload the call replaces      the host-to-device copy of the pictures' coefficient planes from pinned memory;
  schro_hip_noarith_decode_batch    on the noarith twin of the same pictures (tests/noarith_twin.py).

For the 1-picture call the restatement also gives the bins of the picture's longest tower: the call cannot end before
that chain has, so time / those bins bounds the latency of one bin in a chain from above.

Before anything is timed every picture's planes are held against the oracle's coefficients.  Times: device events around
`steps` calls, per call; the median of `rounds` rounds after `warmup` calls, and the spread (max - min) / median.  NOT
measured: the reference's host arithmetic decoder (the committed recipe does not build it), and large pictures.

  SCHRO_HIP_LIB=schroedinger_amd/libschro_hip_exp.so python scripts/arith_decode_ab.py [--out profiles/arith_decode.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import schroedinger_amd as sa           # noqa: E402
import arith_dec_ref as AR              # noqa: E402
import arith_stream as AS               # noqa: E402
from schroedinger_amd import _lib       # noqa: E402


def timed(ctx, fn, a):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pictures", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [r for r in AS.pictures(limit=a.pictures) if not r["zero_residual"]]
    ctx = sa.Context(0)
    experiments = "exp" in os.path.basename(_lib.LIB_PATH)
    lines = ["arith_decode_ab: the reference stream, %d pictures with a residual, 320x240 4:2:0 s16, depth %d%s"
             % (len(recs), recs[0]["twin"]["depth"], ", experiments library" if experiments else "")]
    words, nwords = C.sizeof(_lib.ArithDecodeResult) // 4, C.sizeof(_lib.NoarithDecodeResult) // 4
    dev = []
    for r in recs:
        shapes = [c.shape for c in r["coeffs"]]
        dev.append(dict(data=ctx.upload_bytes(np.frombuffer(r["arith"], np.uint8)), twin=ctx.upload_bytes(np.frombuffer(r["transform"], np.uint8)),
                        coeffs=[ctx.plane(h, w, np.int16) for h, w in shapes], res=ctx.plane(1, words, np.uint32),
                        nres=ctx.plane(1, nwords, np.uint32), pinned=[ctx.host_array(s, np.int16) for s in shapes]))
        for p, c in zip(dev[-1]["pinned"], r["coeffs"]):
            p[...] = c
    entries = [AS.entry(r, d["data"], len(r["arith"]), d["coeffs"], None, d["res"]) for r, d in zip(recs, dev)]
    twins = [AS.entry(r, d["twin"], len(r["transform"]), d["coeffs"], None, d["nres"]) for r, d in zip(recs, dev)]

    # the check: every picture's planes (the intra picture's in front of DC prediction: against the restatement)
    ctx.arith_decode_batch(entries)
    ctx.synchronize()
    bins = []
    for r, d in zip(recs, dev):
        res = sa.arith_decode_result(d["res"].download())
        assert res["error"] == 0 and res["bytes_read"] == len(r["arith"]), res
        bins.append(res["bins"])
        if r["twin"]["is_intra"]:
            want = [np.zeros(c.shape, np.int16) for c in r["coeffs"]]
            P = r["twin"]
            band_bins = {}
            ref = AR.decode_transform_data(r["arith"], want, None, P["depth"], P["horiz_cb"], P["vert_cb"], P["cb_mode"], 1, P["compat"], band_bins)
            assert ref["bins"] == res["bins"]
        else:
            want = r["coeffs"]
        for k in range(3):
            assert np.array_equal(d["coeffs"][k].download(), want[k]), (r["number"], k)
    lines.append("every picture's coefficient planes equal the oracle's; bins per picture %d .. %d" % (min(bins), max(bins)))

    # the longest tower of picture 0 (the 1-picture call)
    P0 = recs[0]["twin"]
    want = [np.zeros(c.shape, np.int16) for c in recs[0]["coeffs"]]
    band_bins = {}
    AR.decode_transform_data(recs[0]["arith"], want, None, P0["depth"], P0["horiz_cb"], P0["vert_cb"], P0["cb_mode"], P0["is_intra"], P0["compat"],
                             band_bins)
    towers = [band_bins.get((k, 0), 0) for k in range(3)] + [sum(band_bins.get((k, o + 3 * l), 0) for l in range(P0["depth"]))
                                                             for k in range(3) for o in (1, 2, 3)]
    longest = max(towers)

    for n in (1, 8, len(recs)):
        batch, tbatch = entries[:n], twins[:n]
        nbins, nbytes = sum(bins[:n]), sum(len(r["arith"]) for r in recs[:n])
        planes_bytes = sum(c.nbytes for r in recs[:n] for c in r["coeffs"])
        lines.append("%d picture%s per call: %d bins, %d bytes of transform data, %.2f MB of coefficient planes" % (n, "s" * (n > 1), nbins, nbytes, planes_bytes / 1e6))

        def decode():
            ctx.arith_decode_batch(batch)

        def report(name, t, spread):
            lines.append("  %-26s %9.4f ms per call, spread %4.1f %%: %8.2f Mbin/s, %8.2f ns per bin over the call, %8.2f MB/s of transform data"
                         % (name, t, 100 * spread, nbins / (t * 1e-3) / 1e6, t * 1e6 / nbins, nbytes / (t * 1e-3) / 1e6))

        t, spread = timed(ctx, decode, a)
        report("arith_decode_batch", t, spread)
        if n == 1:
            lines.append("  %-26s the longest tower of the picture has %d of its %d bins: at most %.1f ns per bin of one chain" % ("", longest, nbins, t * 1e6 / longest))
        if experiments:
            os.environ["SCHRO_HIP_ARDEC_PER_LANE"] = "1"
            tw, spread = timed(ctx, decode, a)
            report("a tower per lane", tw, spread)
            os.environ.pop("SCHRO_HIP_ARDEC_PER_LANE", None)
            for bit, name in ((1, "header"), (2, "clear"), (4, "decode")):
                os.environ["SCHRO_HIP_ARDEC_STAGES"] = str(bit)
                ts, spread = timed(ctx, decode, a)
                lines.append("  launch %-19s %9.4f ms per call, spread %4.1f %%" % (name, ts, 100 * spread))
            os.environ.pop("SCHRO_HIP_ARDEC_STAGES", None)
            ctx.arith_decode_batch(batch)       # (the planes as a whole call leaves them)

        def upload():
            for d in dev[:n]:
                for c, p in zip(d["coeffs"], d["pinned"]):
                    c.upload_async(p)

        tu, spread = timed(ctx, upload, a)
        lines.append("  %-26s %9.4f ms per call, spread %4.1f %%: the coefficient planes from pinned memory, %.2f GB/s" % ("upload it replaces", tu, 100 * spread, planes_bytes / (tu * 1e-3) / 1e9))

        def vlc():
            ctx.noarith_decode_batch(tbatch)

        tv, spread = timed(ctx, vlc, a)
        lines.append("  %-26s %9.4f ms per call, spread %4.1f %%: the noarith twin of the same pictures (%d bytes)" % ("noarith_decode_batch", tv, 100 * spread, sum(len(r["transform"]) for r in recs[:n])))
    lines.append("not measured: the reference's host arithmetic decoder (not built by the committed recipe); pictures larger than the stream's")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
