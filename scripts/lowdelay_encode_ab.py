#!/usr/bin/env python3
"""First numbers for the low-delay slice encoder (lowdelay_enc.hip) beside its mirror and the wavelet in front of it.

8K (7680 x 4320) 4:2:2 s16, transform depth 3, 240 x 540 slices of 32 x 8 luma samples, `--bytes` bytes per slice, one
picture per call and eight; the coefficients are the forward DD(9,7) wavelet (schro_hip_iwt_batch) of a natural-like
picture (tests/synth.py picture_u8, blurred noise, blurred twice more).  In the same run, on the same planes:

  schro_hip_lowdelay_encode_batch   the whole call (three launches and the clear of the count);
  its three launches one at a time  (experiments library only: SCHRO_HIP_LDENC_STAGES = 1 estimate, 2 choose, 4 pack; each
                                    runs on the tables the full call before it left);
  schro_hip_lowdelay_batch          the decoder, on the bytes the encoder produced;
  schro_hip_iwt_batch               the forward wavelet that produces the coefficients.

Times: device events around `steps` calls (Context.timer_begin / timer_end), per call; the median of `rounds` rounds after
`warmup` calls, and the spread (max - min) / median.  The serial launch is also given per anti-diagonal of slices
(n_horiz_slices + n_vert_slices - 1 of them, a workgroup barrier each) and as the ratio eight pictures / one.

  SCHRO_HIP_LIB=schroedinger_amd/libschro_hip_exp.so python scripts/lowdelay_encode_ab.py [--out profiles/r15_lowdelay_encode.txt]"""
import argparse
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

W, H, DEPTH, FILT, NH, NV = 7680, 4320, 3, 0, 240, 540
COMPS = [(H, W), (H, W // 2), (H, W // 2)]
MATRIX = [12, 10, 10, 8, 6, 6, 4, 2, 2, 0]


def natural_like(h, w, seed):
    p = synth.picture_u8(h, w, seed=seed, blur=True).astype(np.int32)
    for _ in range(2):
        q = np.pad(p, 1, mode="edge")
        p = sum(q[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) // 9
    return (p - 128).astype(np.int16)


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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bytes", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    experiments = "exp" in os.path.basename(_lib.LIB_PATH)
    P = dict(transform_depth=DEPTH, iwt_luma_width=W, iwt_luma_height=H, iwt_chroma_width=W // 2, iwt_chroma_height=H,
             n_horiz_slices=NH, n_vert_slices=NV, slice_bytes_num=a.bytes, slice_bytes_denom=1, quant_matrix=MATRIX + [0] * 9)
    nslices, nbytes = NH * NV, a.bytes * NH * NV
    lines = ["lowdelay_encode_ab: %dx%d 4:2:2 s16, depth %d, %d x %d slices of %d bytes (%.1f MB of slices for %.1f MB of coefficients)%s"
             % (W, H, DEPTH, NH, NV, a.bytes, nbytes / 1e6, 2 * sum(h * w for h, w in COMPS) / 1e6,
                ", experiments library" if experiments else "")]
    src = [ctx.upload(natural_like(*COMPS[k], seed=5 + k)) for k in range(3)]
    res = {}
    for npic in (1, 8):
        co = [[ctx.plane(*COMPS[k], np.int16) for k in range(3)] for _ in range(npic)]
        pairs = [(src[k], co[p][k]) for p in range(npic) for k in range(3)]
        bufs = [(ctx.plane(1, nbytes, np.uint8), ctx.plane(1, nslices, np.uint8), ctx.plane(1, 1, np.uint32)) for _ in range(npic)]
        dec = [[ctx.plane(*COMPS[k], np.int16) for k in range(3)] for _ in range(npic)]

        def wavelet():
            ctx.iwt_batch(pairs, DEPTH, FILT)

        def encode():
            ctx.lowdelay_encode_batch([(co[p],) + bufs[p] for p in range(npic)], P)

        def decode():
            ctx.lowdelay_batch([(bufs[p][0], dec[p]) for p in range(npic)], P)

        wavelet()
        encode()
        ctx.synchronize()
        index = bufs[0][1].download()[0]
        lines.append("%d picture(s): base indices %d .. %d (median %d), %d over-run slices" % (
            npic, index.min(), index.max(), int(np.median(index)), int(bufs[0][2].download()[0, 0])))
        for name, fn in (("encode", encode), ("decode", decode), ("wavelet", wavelet)):
            t, spread = timed(ctx, fn, a)
            res[(name, npic)] = t
            lines.append("  %-8s %8.4f ms per call, %8.4f ms per picture, spread %.1f %%" % (name, t, t / npic, 100 * spread))
        if experiments:
            for bit, name in ((1, "estimate"), (2, "choose"), (4, "pack")):
                os.environ["SCHRO_HIP_LDENC_STAGES"] = str(bit)
                t, spread = timed(ctx, encode, a)
                res[(name, npic)] = t
                lines.append("  launch %-8s %8.4f ms per call, %8.4f ms per picture, spread %.1f %%" % (name, t, t / npic, 100 * spread))
            os.environ.pop("SCHRO_HIP_LDENC_STAGES", None)
            lines.append("  the serial launch: %.3f us per anti-diagonal (%d of them); %.0f %% of the three launches' sum"
                         % (1e3 * res[("choose", npic)] / (NH + NV - 1), NH + NV - 1,
                            100 * res[("choose", npic)] / sum(res[(n, npic)] for n in ("estimate", "choose", "pack"))))
        lines.append("  ratio encode / decode %.1f, encode / wavelet %.1f" % (res[("encode", npic)] / res[("decode", npic)],
                                                                              res[("encode", npic)] / res[("wavelet", npic)]))
        for group in co + dec:
            for p in group:
                p.free()
        for group in bufs:
            for p in group:
                p.free()
    if experiments:
        lines.append("the serial launch from one picture to eight (a workgroup per picture): x %.2f" % (res[("choose", 8)] / res[("choose", 1)]))
    lines.append("the whole call from one picture to eight: x %.2f" % (res[("encode", 8)] / res[("encode", 1)]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
