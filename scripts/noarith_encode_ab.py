#!/usr/bin/env python3
"""First numbers for the noarith (VLC) transform-data encoder (noarith_enc.hip) beside what it replaces.

8 x 2160p 4:2:0 s16 pictures per call, transform depth 3, the stream's default codeblock counts for inter pictures
(schro_params_init, schroparams.c:84-103: 1 x 1, 1 x 1, 8 x 6, 12 x 8), codeblock_mode_index 1.  The values are what the
encode loop leaves in the quant planes: a residual (a natural-like picture, tests/synth.py picture_u8 blurred, minus
itself moved by one sample -- what a motion-compensated prediction leaves behind), its forward DD(9,7) wavelet
(schro_hip_iwt_batch) and schro_hip_quantise_batch at one quant index for all sub-bands, a low one and a high one.

In the same run, on the same planes:

  schro_hip_noarith_encode_batch     the whole call (the clear of the results, count, layout, clear, pack);
  its launches one at a time         (experiments library only: SCHRO_HIP_NAENC_STAGES = 1 count, 2 layout, 4 clear + pack;
                                     each runs on the tables the full call before it left);
  the device-to-host copy            of the eight quant frames into pinned memory: what a host packer needs today.

Before anything is timed the sizes of picture 0 -- every sub-band's bits, the total, false_zero -- are held against a
vectorised count of the same syntax on the downloaded quant planes (the bytes themselves are the GPU tests' business).
Times: device events around `steps` calls (Context.timer_begin / timer_end), per call; the median of `rounds` rounds after
`warmup` calls, and the spread (max - min) / median.  NOT shown: the host's packer, which is not built here; the copy is
only the part of today's path that this call makes unnecessary, the stream bytes still have to reach the host.

  SCHRO_HIP_LIB=schroedinger_amd/libschro_hip_exp.so python scripts/noarith_encode_ab.py [--out profiles/noarith_encode.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import noarith_enc_ref as ref           # noqa: E402
import schroedinger_amd as sa           # noqa: E402
import synth                            # noqa: E402
from schroedinger_amd import _lib       # noqa: E402

NPIC, W, H, DEPTH, FILT, MODE = 8, 3840, 2160, 3, 0, 1
COUNTS = ([1, 1, 8, 12], [1, 1, 6, 8])
COMPS = [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
NSUB = 1 + 3 * DEPTH


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


def uint_bits(v):
    return 2 * (int(v) + 1).bit_length() - 1


def expected_sizes(planes, qi):
    """subband_bits (3 x 19) and the total bytes of one picture, counted with numpy (true zero tests: the values are far
    from a 16-bit row sum of 65536, which the false_zero counts of the call confirm)."""
    bits = np.zeros((3, ref.MAX_SUBBANDS), np.int64)
    total = 0
    for k in range(3):
        for i in range(NSUB):
            b = ref.subband(planes[k], DEPTH, i).astype(np.int64)
            hc, vc = ref.codeblock_counts(i, *COUNTS)
            zf, qo = ref.flags_of(i, hc, vc, MODE)
            mag = np.abs(b)
            code = 2 * (np.floor(np.log2(mag + 1)).astype(np.int64) + 1) - 1 + (mag > 0)
            if not mag.any():
                total += 1
                continue
            payload = 0
            for y in range(vc):
                for x in range(hc):
                    cb = ref.get_codeblock(code, x, y, hc, vc)
                    zero = zf and not ref.get_codeblock(mag, x, y, hc, vc).any()
                    payload += int(zf) + (0 if zero else int(qo) + int(cb.sum()))
            length = (payload + 7) // 8
            header = (uint_bits(length) + uint_bits(qi) + 7) // 8
            bits[k, i] = 8 * (header + length)
            total += header + length
    return bits, total


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
    lines = ["noarith_encode_ab: %d x %dx%d 4:2:0 s16, depth %d, codeblocks %s x %s, %d samples (%.1f MB of quant frames) per call%s"
             % (NPIC, W, H, DEPTH, COUNTS[0], COUNTS[1], samples, 2 * samples / 1e6, ", experiments library" if experiments else "")]
    src = [ctx.upload(residual(*COMPS[k], seed=5 + k)) for k in range(3)]
    co = [[ctx.plane(*COMPS[k], np.int16) for k in range(3)] for _ in range(NPIC)]
    qu = [[ctx.plane(*COMPS[k], np.int16, stride=co[p][k].stride) for k in range(3)] for p in range(NPIC)]
    pairs = [(src[k], co[p][k]) for p in range(NPIC) for k in range(3)]
    bound = sa.noarith_encode_bound([(w, h) for h, w in COMPS], DEPTH, COUNTS[0], COUNTS[1], 2)
    words = C.sizeof(_lib.NoarithResult) // 4
    outs = [ctx.plane(1, bound, np.uint8) for _ in range(NPIC)]
    ress = [ctx.plane(1, words, np.uint32) for _ in range(NPIC)]
    pinned = [[ctx.host_array((h, w), np.int16) for h, w in COMPS] for _ in range(NPIC)]
    lines.append("output capacity per picture (schro_hip_noarith_encode_bound): %.1f MB" % (bound / 1e6))

    def copy_back():
        for p in range(NPIC):
            for k in range(3):
                qu[p][k].download_async(pinned[p][k])

    for qi in (8, 28):
        tabs = []
        for k, (h, w) in enumerate(COMPS):
            tab = ctx.codeblock_layout(w, h, DEPTH, COUNTS[0], COUNTS[1], co[0][k].stride, 2)
            for t in tab:
                t.quant_index = qi
            tabs.append(tab)
        ctx.iwt_batch(pairs, DEPTH, FILT)
        [s.free() for s in ctx.quantise_batch([(co[p][k], qu[p][k], tabs[k], 0) for p in range(NPIC) for k in range(3)])]
        pics = [(qu[p], tabs, DEPTH, COUNTS[0], COUNTS[1], MODE, outs[p], bound, ress[p]) for p in range(NPIC)]

        def encode():
            ctx.noarith_encode_batch(pics)

        encode()
        ctx.synchronize()
        results = [sa.noarith_result(r.download()) for r in ress]
        want_bits, want_total = expected_sizes([q.download() for q in qu[0]], qi)
        assert results[0]["bytes"] == want_total and np.array_equal(results[0]["subband_bits"], want_bits), (results[0], want_total)
        assert all(r["overrun"] == 0 and r["false_zero"] == (0, 0) and r["bytes"] == want_total for r in results)
        nbytes = sum(r["bytes"] for r in results)
        lines.append("quant index %d: %.2f MB of stream for the call (%.3f bits per sample); sizes of picture 0 checked against a host count"
                     % (qi, nbytes / 1e6, 8.0 * nbytes / samples))
        t, spread = timed(ctx, encode, a)
        lines.append("  encode     %8.4f ms per call, %8.4f ms per picture, spread %.1f %% (%.2f TB/s of quant samples read twice)"
                     % (t, t / NPIC, 100 * spread, 4.0 * samples / (t * 1e-3) / 1e12))
        if experiments:
            for bit, name in ((1, "count"), (2, "layout"), (4, "clear+pack")):
                os.environ["SCHRO_HIP_NAENC_STAGES"] = str(bit)
                ts, spread = timed(ctx, encode, a)
                lines.append("  launch %-10s %8.4f ms per call, spread %.1f %%" % (name, ts, 100 * spread))
            os.environ.pop("SCHRO_HIP_NAENC_STAGES", None)
        tc, spread = timed(ctx, copy_back, a)
        lines.append("  copy back  %8.4f ms per call for the eight quant frames (%.1f GB/s), spread %.1f %%; the stream itself is %.2f MB"
                     % (tc, 2.0 * samples / (tc * 1e-3) / 1e9, 100 * spread, nbytes / 1e6))
        lines.append("  ratio copy back / encode %.1f" % (tc / t))
    lines.append("not shown: the host's packer (not built here); the stream bytes still have to be copied to the host")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
