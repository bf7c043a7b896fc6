#!/usr/bin/env python3
"""First numbers for the noarith (VLC) transform-data decoder (noarith_dec.hip) beside what it replaces.

The workload of scripts/noarith_encode_ab.py: 8 x 2160p 4:2:0 s16 pictures per call, transform depth 3, codeblock counts
1 x 1, 1 x 1, 8 x 6, 12 x 8, codeblock_mode_index 1, a residual through the forward DD(9,7) wavelet and
schro_hip_quantise_batch at one quant index for all sub-bands, a low one (8) and a high one (28).  The streams are produced
by schro_hip_noarith_encode_batch and read with compat_quant_offset 1, where the encoder's and the decoder's rules agree.

In the same run, on the same pictures:

  schro_hip_noarith_decode_batch     the whole call (the clear of the results, header, summary, chain, decode, fill), from
                                     the streams on the device into the coefficient planes;
  its launches one at a time         (experiments library only: SCHRO_HIP_NADEC_STAGES = 1 header, 2 summary, 4 chain,
                                     8 decode + fill; each runs on the tables the full call before it left);
  what the call replaces             the host-to-device copy of the tight 2-byte hand-over of a host entropy decoder (every
                                     codeblock's values row-major, from pinned memory) and schro_hip_dequant_plan_run.

Before anything is timed the decoded coefficient planes of every picture are held against the reconstruction the quantiser
left, the quant planes against the quantiser's, and the result blocks against the encoder's sizes.  Times: device events
around `steps` calls (Context.timer_begin / timer_end), per call; the median of `rounds` rounds after `warmup` calls, and
the spread (max - min) / median.  NOT shown: the host's VLC decoder, which is not built here -- the replaced path is only
what remains of it on the device's side; and the copy of the stream itself to the device (13 to 86 MB against 199 MB).

  SCHRO_HIP_LIB=schroedinger_amd/libschro_hip_exp.so python scripts/noarith_decode_ab.py [--out profiles/noarith_decode.txt]"""
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
import synth                            # noqa: E402
from schroedinger_amd import _lib       # noqa: E402

NPIC, W, H, DEPTH, FILT, MODE = 8, 3840, 2160, 3, 0, 1
COUNTS = ([1, 1, 8, 12], [1, 1, 6, 8])
COMPS = [(H, W), (H // 2, W // 2), (H // 2, W // 2)]


def residual(h, w, seed):
    p = synth.picture_u8(h, w, seed=seed, blur=True).astype(np.int16)
    return p - np.roll(p, (1, 1), (0, 1))


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


def hand_over(plane, tab, stride):
    """The values of every record of `tab`, row-major and tight, 2 bytes each, and the records that point into them."""
    raw = np.zeros((plane.shape[0], stride // 2), np.int16)
    raw[:, :plane.shape[1]] = plane
    flat = raw.reshape(-1)
    parts, recs, at = [], [], 0
    for t in tab:
        rows = (t.dst_offset // 2 + np.arange(t.height) * (t.dst_stride // 2))[:, None] + np.arange(t.width)[None, :]
        parts.append(flat[rows].reshape(-1))
        recs.append((t.dst_offset, t.dst_stride, t.width, t.height, at, 2, t.quant_index))
        at += 2 * t.width * t.height
    return np.concatenate(parts), recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    experiments = "exp" in os.path.basename(_lib.LIB_PATH)
    samples = NPIC * sum(h * w for h, w in COMPS)
    lines = ["noarith_decode_ab: %d x %dx%d 4:2:0 s16, depth %d, codeblocks %s x %s, %d samples (%.1f MB of coefficient frames) per call%s"
             % (NPIC, W, H, DEPTH, COUNTS[0], COUNTS[1], samples, 2 * samples / 1e6, ", experiments library" if experiments else "")]
    src = [ctx.upload(residual(*COMPS[k], seed=5 + k)) for k in range(3)]
    co = [[ctx.plane(*COMPS[k], np.int16) for k in range(3)] for _ in range(NPIC)]
    qu = [[ctx.plane(*COMPS[k], np.int16, stride=co[p][k].stride) for k in range(3)] for p in range(NPIC)]
    dco = [[ctx.plane(*COMPS[k], np.int16, stride=co[p][k].stride) for k in range(3)] for p in range(NPIC)]
    dqu = [ctx.plane(*COMPS[k], np.int16, stride=co[0][k].stride) for k in range(3)]
    pairs = [(src[k], co[p][k]) for p in range(NPIC) for k in range(3)]
    bound = sa.noarith_encode_bound([(w, h) for h, w in COMPS], DEPTH, COUNTS[0], COUNTS[1], 2)
    outs = [ctx.plane(1, bound, np.uint8) for _ in range(NPIC)]
    eres = [ctx.plane(1, C.sizeof(_lib.NoarithResult) // 4, np.uint32) for _ in range(NPIC)]
    dres = [ctx.plane(1, C.sizeof(_lib.NoarithDecodeResult) // 4, np.uint32) for _ in range(NPIC)]
    blobs = [[ctx.plane(1, 2 * h * w, np.uint8) for h, w in COMPS] for _ in range(NPIC)]
    pinned = [[ctx.host_array((1, 2 * h * w), np.uint8) for h, w in COMPS] for _ in range(NPIC)]

    for qi in (8, 28):
        tabs = []
        for k, (h, w) in enumerate(COMPS):
            tab = ctx.codeblock_layout(w, h, DEPTH, COUNTS[0], COUNTS[1], co[0][k].stride, 2)
            for t in tab:
                t.quant_index = qi
            tabs.append(tab)
        ctx.iwt_batch(pairs, DEPTH, FILT)
        [s.free() for s in ctx.quantise_batch([(co[p][k], qu[p][k], tabs[k], 0) for p in range(NPIC) for k in range(3)])]
        ctx.noarith_encode_batch([(qu[p], tabs, DEPTH, COUNTS[0], COUNTS[1], MODE, outs[p], bound, eres[p]) for p in range(NPIC)])
        ctx.synchronize()
        sizes = [sa.noarith_result(r.download()) for r in eres]
        assert all(r["overrun"] == 0 and r["false_zero"] == (0, 0) for r in sizes)
        nbytes = [r["bytes"] for r in sizes]

        def pics(quant):
            return [(outs[p], nbytes[p], None, dco[p], quant if p == 0 else None, DEPTH, COUNTS[0], COUNTS[1], MODE, 0, 1, dres[p])
                    for p in range(NPIC)]

        # the check: picture 0 with its quant planes, every picture's coefficients and result
        for batch in ([pics(dqu)[0]], pics(None)):
            ctx.noarith_decode_batch(batch)
        ctx.synchronize()
        want = [c.download() for c in co[0]]
        for k in range(3):
            assert np.array_equal(dqu[k].download(), qu[0][k].download()), ("quant", k)
        for p in range(NPIC):
            r = sa.noarith_decode_result(dres[p].download())
            assert r["error"] == 0 and r["bytes_read"] == nbytes[p] and r["compat_quant_offset"] == 1, r
            assert (r["truncated"], r["not_consumed"], r["overran"], r["long_codes"], r["clamped_quant"]) == (0, 0, 0, 0, 0), r
            for k in range(3):
                assert np.array_equal(dco[p][k].download(), want[k]), ("coeffs", p, k)
        lines.append("quant index %d: %.2f MB of stream for the call (%.3f bits per sample); every picture's coefficients equal the "
                     "quantiser's reconstruction" % (qi, sum(nbytes) / 1e6, 8.0 * sum(nbytes) / samples))
        batch = pics(None)

        def decode():
            ctx.noarith_decode_batch(batch)

        t, spread = timed(ctx, decode, a)
        lines.append("  decode     %8.4f ms per call, %8.4f ms per picture, spread %.1f %% (%.2f GB/s of stream, %.2f TB/s of samples written)"
                     % (t, t / NPIC, 100 * spread, sum(nbytes) / (t * 1e-3) / 1e9, 2.0 * samples / (t * 1e-3) / 1e12))
        if experiments:
            for bit, name in ((1, "header"), (2, "summary"), (4, "chain"), (8, "decode+fill")):
                os.environ["SCHRO_HIP_NADEC_STAGES"] = str(bit)
                ts, spread = timed(ctx, decode, a)
                lines.append("  launch %-11s %8.4f ms per call, spread %.1f %%" % (name, ts, 100 * spread))
            os.environ.pop("SCHRO_HIP_NADEC_STAGES", None)

        # what the call replaces: the tight 2-byte hand-over of a host entropy decoder goes up, the plan dequantises it
        quant0 = [q.download() for q in qu[0]]
        tables = []
        for k in range(3):
            values, recs = hand_over(quant0[k], tabs[k], co[0][k].stride)
            tables.append(ctx.codeblock_table(recs))
            for p in range(NPIC):
                pinned[p][k][0, :] = values.view(np.uint8)
        jobs = [(dco[p][k], blobs[p][k], tables[k], 0) for p in range(NPIC) for k in range(3)]
        plan = ctx.dequant_plan(jobs, arith=1)
        planes = plan.planes(jobs)

        def replaced():
            for p in range(NPIC):
                for k in range(3):
                    blobs[p][k].upload_async(pinned[p][k])
            plan.run(planes=planes)

        def dequant_only():
            plan.run(planes=planes)

        replaced()
        ctx.synchronize()
        for p in (0, NPIC - 1):
            for k in range(3):
                assert np.array_equal(dco[p][k].download(), want[k]), ("hand-over", p, k)
        tr, spread = timed(ctx, replaced, a)
        lines.append("  replaced   %8.4f ms per call: host-to-device copy of the tight 2-byte hand-over (%.1f MB, %.1f GB/s over all) + "
                     "dequant_plan_run, spread %.1f %%" % (tr, 2 * samples / 1e6, 2.0 * samples / (tr * 1e-3) / 1e9, 100 * spread))
        td, spread = timed(ctx, dequant_only, a)
        lines.append("  of which dequant_plan_run alone %8.4f ms per call, spread %.1f %%" % (td, 100 * spread))
        lines.append("  ratio replaced / decode %.2f" % (tr / t))
        plan.free()
    lines.append("not shown: the host's VLC decoder (not built here) in front of the replaced path; the copy of the stream to the device in "
                 "front of the decode")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
