#!/usr/bin/env python3
"""First numbers for the encoder's quantisation (quant.hip) beside its decoder-side twin.

8 x 2160p 4:2:0 s16 pictures (24 planes per call), transform depth 3, the stream's default codeblock counts
(schro_params_init, schroparams.c:84-103: inter 1 x 1, 1 x 1, 8 x 6, 12 x 8; intra 1 x 1, 1 x 1, 1 x 1, 4 x 3):

  quantise inter   schro_hip_quantise_batch, every sub-band through quantise_kernel;
  quantise intra   the same with the LL bands through quantise_dc_kernel, reported separately;
  dequant          schro_hip_dequant_batch (arith 0, two-byte values) on the same geometry, in the same run: the yardstick.
                   It moves 4 bytes per sample (values read, coefficients written) against the quantiser's 6 (coefficients
                   read, quantised and reconstructed values written);
  dc one picture   quantise_dc_kernel alone for the three LL bands of ONE intra picture, with its number of diagonals.
Times are the kernels' own, from the context's profile events (per call: total over the launches of the class / calls);
medians over `rounds` rounds of `steps` calls after `warmup`, and the spread (max - min) / median.  The results of the first
call are compared with tests/quant_ref.py on one luma and one chroma plane before anything is timed.

  python scripts/quantise_ab.py [--rounds 5] [--steps 20] [--out profiles/r13_quantise.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import quant_cases as QC                # noqa: E402
import quant_ref as Q                   # noqa: E402
import schroedinger_amd as sa           # noqa: E402

NPIC, W, H, DEPTH = 8, 3840, 2160, 3
INTER = ([1, 1, 8, 12], [1, 1, 6, 8])
INTRA = ([1, 1, 1, 4], [1, 1, 1, 3])


def profiled(ctx, fn, classes, a):
    """median ms per call of each kernel class, and the spread of their sum"""
    rows = []
    for _ in range(a.rounds):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.profile_reset()
        for _ in range(a.steps):
            fn()
        ctx.synchronize()
        prof = ctx.profile_read()
        rows.append([prof[c][0] / a.steps for c in classes])
    med = [statistics.median(r[k] for r in rows) for k in range(len(classes))]
    tot = [sum(r) for r in rows]
    return med, (max(tot) - min(tot)) / statistics.median(tot)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    ctx.profile_enable(True)
    rng = np.random.default_rng(1)
    comps = [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
    host = [np.clip(np.rint(rng.laplace(0.0, 60.0, s)), -4095, 4095).astype(np.int16) for s in comps]
    co = [ctx.upload(host[k % 3]) for k in range(3 * NPIC)]
    qu = [ctx.plane(p.height, p.width, np.int16, stride=p.stride) for p in co]
    samples = NPIC * sum(h * w for h, w in comps)

    def jobs_for(counts, intra, planes=range(3 * NPIC)):
        jobs = []
        for k in planes:
            h, w = comps[k % 3]
            recs = QC.layout(w, h, DEPTH, counts[0], counts[1], co[k].stride, 2)
            for n, r in enumerate(recs):
                r[4] = 12 + (n % 9)
            dc = (counts[0][0] * counts[1][0], w >> DEPTH, h >> DEPTH) if intra else None
            jobs.append((co[k], qu[k], QC.table(recs), intra, dc, recs))
        return jobs

    lines = ["quantise_ab: %d x %dx%d 4:2:0 s16, depth %d, %d samples per call" % (NPIC, W, H, DEPTH, samples)]
    # correctness first: one luma and one chroma plane of an intra call against the checker
    jobs = jobs_for(INTRA, 1)
    summ = ctx.quantise_batch([j[:5] for j in jobs])
    for k in (0, 1):
        pitch = co[k].stride // 2
        buf = np.zeros((co[k].height, pitch), np.int16)
        buf[:, :co[k].width] = host[k]
        want_q, want_r, want_s = Q.quantise_plane(buf, jobs[k][5], 1, jobs[k][4][0], jobs[k][4][1:])
        assert np.array_equal(qu[k].download(), want_q[:, :co[k].width]) and np.array_equal(co[k].download(), want_r[:, :co[k].width])
        assert summ[k].download().tolist() == [list(s) for s in want_s]
    [s.free() for s in summ]
    lines.append("checked against tests/quant_ref.py: planes 0 and 1 of an intra call, values, reconstruction, summaries")

    def quantise(jobs):
        def fn():
            [s.free() for s in ctx.quantise_batch([j[:5] for j in jobs])]
        return fn

    res = {}
    for name, counts, intra in (("inter", INTER, 0), ("intra", INTRA, 1)):
        for p, h in zip(co, [host[k % 3] for k in range(3 * NPIC)]):
            p.upload(h)
        (tq, tdc), spread = profiled(ctx, quantise(jobs_for(counts, intra)), ("quantise", "quantise_dc"), a)
        res[name] = (tq, tdc)
        n_q = samples - (NPIC * sum((h >> DEPTH) * (w >> DEPTH) for h, w in comps) if intra else 0)
        lines.append("quantise %s: quantise_kernel %.4f ms per call (%.2f TB/s at 6 B per sample), quantise_dc_kernel %.4f ms, spread %.1f %%"
                     % (name, tq, 6.0 * n_q / (tq * 1e-3) / 1e12, tdc, 100 * spread))
    # the yardstick: the decoder's dequantisation of two-byte values on the inter geometry
    djobs, vals = [], []
    for k in range(3 * NPIC):
        h, w = comps[k % 3]
        recs = QC.layout(w, h, DEPTH, INTER[0], INTER[1], co[k].stride, 2)
        off, cbs = 0, []
        for (o, st, cw, ch, _) in recs:
            cbs.append((o, st, cw, ch, off, 2, 20))
            off += 2 * cw * ch
        v = ctx.upload_bytes(np.zeros(off, np.uint8) + 3)
        vals.append(v)
        djobs.append((co[k], v, ctx.codeblock_table(cbs), 0))
    (td,), spread = profiled(ctx, lambda: ctx.dequant_batch(djobs, arith=0), ("dequant",), a)
    lines.append("dequant (yardstick, same geometry, 2-byte values): %.4f ms per call (%.2f TB/s at 4 B per sample), spread %.1f %%"
                 % (td, 4.0 * samples / (td * 1e-3) / 1e12, 100 * spread))
    lines.append("ratio quantise inter / dequant: %.2f (byte ratio 1.5)" % (res["inter"][0] / td))
    # the serial DC bands of one intra picture
    one = jobs_for(INTRA, 1, planes=range(3))
    (_, tdc1), spread = profiled(ctx, quantise(one), ("quantise", "quantise_dc"), a)
    lines.append("dc one picture: quantise_dc_kernel %.4f ms for the three LL bands of one 2160p intra picture (luma %d x %d: %d diagonals; "
                 "chroma %d diagonals), spread %.1f %%" % (tdc1, W >> DEPTH, H >> DEPTH, (W >> DEPTH) + (H >> DEPTH) - 1,
                                                           (W >> (DEPTH + 1)) + (H >> (DEPTH + 1)) - 1, 100 * spread))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
