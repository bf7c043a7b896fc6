#!/usr/bin/env python3
"""First numbers for the quantiser choice on the device (quant_choose.hip) and for the host round trip it removes.

8 x 2160p 4:2:0 s16 pictures, transform depth 3, inter, noarith; coefficients drawn with a two-sided geometric fall-off per
sub-band (no wavelet is run: the stages timed here read coefficients, whatever made them).

  (1) the stage by itself, per engine: one schro_hip_quant_choose_batch over the eight pictures' counts (device events);
  (2) the chain enqueued without a wait: schro_hip_histogram_batch -> schro_hip_quant_choose_batch ->
      schro_hip_quantise_chosen_batch -> schro_hip_noarith_encode_chosen_batch, one queue synchronise per call of the chain
      (host clock: the figure is what a caller sees);
  (3) the same work the way it ran before: histogram, queue synchronise, download of the 8 x 30 x 420 bytes of counts, then
      schro_hip_quantise_batch and schro_hip_noarith_encode_batch with host records that carry the indices (those the
      device chose in (2), fetched once beforehand), one synchronise at the end.  The host's own estimate and choice code
      is NOT built here and is NOT in that figure: (3) is the round trip alone, a lower bound of what (2) replaces.
The quantiser overwrites the coefficients with the reconstruction, so from the second call on the histograms see
reconstructed planes; the launches and their sizes are the same.

Every step runs under its own time limit (--limit seconds, SIGALRM): a step that exceeds it ends the script with a
non-zero status and nothing more is started.

  python scripts/quant_choose_ab.py [--rounds 5] [--steps 10] [--out profiles/quant_choose.txt]"""
import argparse
import ctypes as C
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                      # noqa: E402
import hist_ref as H                    # noqa: E402
import noarith_enc_ref as NR            # noqa: E402
import quant_cases as QC                # noqa: E402
import quant_choose_draws as D          # noqa: E402
import schroedinger_amd as sa           # noqa: E402
from schroedinger_amd import _lib       # noqa: E402

NPIC, W, Hh, DEPTH = 8, 3840, 2160, 3
HC, VC = [1, 1, 8, 12], [1, 1, 6, 8]
COMPS = [(Hh, W), (Hh // 2, W // 2), (Hh // 2, W // 2)]
NB = 1 + 3 * DEPTH
ENGINES = (("lambda", 0), ("bit allocation", 1), ("constant error", 2))


class Step:
    """a step under its own time limit"""

    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def __enter__(self):
        def late(signum, frame):
            sys.stderr.write("quant_choose_ab: step '%s' exceeded %d s; stopping\n" % (self.name, self.limit))
            os._exit(3)
        signal.signal(signal.SIGALRM, late)
        signal.alarm(self.limit)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def draw_plane(rng, h, w):
    p = np.zeros((h, w), np.int16)
    for i in range(NB):
        level = H.position(i) >> 2
        v = NR.subband(p, DEPTH, i)
        v[...] = np.rint(rng.laplace(0.0, 1.5 * 2.0 ** (DEPTH - level + (2 if i == 0 else 0)), v.shape)).clip(-3000, 3000).astype(np.int16)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.Context(0)
    rng = np.random.default_rng(3)
    lines = ["quant_choose_ab: %d x %dx%d 4:2:0 s16, depth %d, inter, noarith; %d sub-bands per call" % (NPIC, W, Hh, DEPTH, 3 * NB * NPIC)]

    with Step("set-up", a.limit):
        host = [draw_plane(rng, *COMPS[k]) for k in range(3)]
        co = [ctx.plane(*COMPS[k % 3], np.int16) for k in range(3 * NPIC)]
        qu = [ctx.plane(p.height, p.width, np.int16, stride=p.stride) for p in co]
        bands = [[H.band_rect(COMPS[k % 3][1], COMPS[k % 3][0], DEPTH, i, co[k].stride, 2) + (H.band_skip(i), 0) for i in range(NB)]
                 for k in range(3 * NPIC)]
        harr, counts, block = ctx.histogram_planes([(co[k], bands[k]) for k in range(3 * NPIC)])
        ctx.quant_choose_tables(D.error_table())
        samples = sum(h * w for h, w in COMPS)
        recs, sub = [], []
        for k in range(3):
            r = QC.layout(COMPS[k][1], COMPS[k][0], DEPTH, HC, VC, co[k].stride, 2)
            recs.append(r)
        for i in range(NB):
            nh, nv = NR.codeblock_counts(i, HC, VC)
            sub += [i] * (nh * nv)
        cap = sa.noarith_encode_bound([(w, h) for h, w in COMPS], DEPTH, HC, VC, 2)
        outs = [ctx.plane(1, cap, np.uint8) for _ in range(NPIC)]
        words = C.sizeof(_lib.NoarithResult) // 4
        ress = [ctx.plane(1, words, np.uint32) for _ in range(NPIC)]
        clamped = ctx.plane(1, 2, np.uint32).fill(0)
        weight = [1.0] * NB
        ratio = [[1.0] * NB] * 3

        def upload():
            for k, p in enumerate(co):
                p.upload(host[k % 3])

        def table(k, indices):
            t = [list(r) for r in recs[k]]
            for n, r in enumerate(t):
                r[4] = sub[n] if indices is None else int(indices[sub[n]])
            return QC.table(t)

        chosen_tabs = [table(k, None) for k in range(3)]

        def specs(engine, target):
            return [dict(counts=counts[3 * n:3 * n + 3], skip=[H.band_skip(i) for i in range(NB)], depth=DEPTH, is_intra=0, is_noarith=1,
                         engine=engine, weight=weight, ratio=ratio, scales=D.SCALES, target=target, result=choice.ptr + n * row)
                    for n in range(NPIC)]

        row = sa.QUANT_CHOICE_DTYPE.itemsize
        qi_off = sa.QUANT_CHOICE_DTYPE.fields["quant_index"][1]
        choice = ctx.plane(NPIC, row, np.uint8, stride=row)
        targets = {0: 1.0, 1: 0.5 * samples, 2: 4.0 * samples}
        upload()
        sa.check(ctx.lib.schro_hip_histogram_batch(ctx.h, harr, 3 * NPIC, 2))
        ctx.synchronize()

    def events(fn):
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

    def host_clock(fn):
        rows = []
        for _ in range(a.rounds):
            for _ in range(a.warmup):
                fn()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            rows.append((time.perf_counter() - t0) / a.steps * 1e3)
        med = statistics.median(rows)
        return med, (max(rows) - min(rows)) / med

    # (1) the stage by itself
    for name, engine in ENGINES:
        with Step("stage, " + name, a.limit):
            arr = sa.quant_choose_pictures(specs(engine, targets[engine]))
            t, spread = events(lambda: sa.check(ctx.lib.schro_hip_quant_choose_batch(ctx.h, arr, NPIC)))
            got = choice.download().view(sa.QUANT_CHOICE_DTYPE).reshape(-1)
            lines.append("stage alone, %s: %.4f ms per call of %d pictures (device events), spread %.1f %%; %d evaluations, picture 0 luma "
                         "indices %s" % (name, t, NPIC, 100 * spread, int(got[0]["evaluations"]), got[0]["quant_index"][0, :NB].tolist()))

    # (2) the chain, enqueued
    carr = sa.quant_choose_pictures(specs(1, targets[1]))
    qjobs = [(co[k], qu[k], chosen_tabs[k % 3], 0, None) for k in range(3 * NPIC)]
    rows_of = [choice.ptr + (k // 3) * row + qi_off + 4 * 19 * (k % 3) for k in range(3 * NPIC)]
    whole = [choice.ptr + n * row + qi_off for n in range(NPIC)]
    npics = [(qu[3 * n:3 * n + 3], chosen_tabs, DEPTH, HC, VC, 1, outs[n], cap, ress[n]) for n in range(NPIC)]

    def chain():
        sa.check(ctx.lib.schro_hip_histogram_batch(ctx.h, harr, 3 * NPIC, 2))
        sa.check(ctx.lib.schro_hip_quant_choose_batch(ctx.h, carr, NPIC))
        [s.free() for s in ctx.quantise_chosen_batch(qjobs, rows_of, clamped)]
        ctx.noarith_encode_chosen_batch(npics, whole, clamped.ptr + 4)
        ctx.synchronize()

    with Step("chain, enqueued", a.limit):
        upload()
        t2, spread = host_clock(chain)
        lines.append("chain enqueued (histograms -> choice [bit allocation] -> quantise -> VLC bytes, one synchronise per chain): %.4f ms "
                     "per chain on the host clock, spread %.1f %%; %d bytes for picture 0"
                     % (t2, 100 * spread, int(sa.noarith_result(ress[0].download())["bytes"])))
        indices = choice.download().view(sa.QUANT_CHOICE_DTYPE).reshape(-1)["quant_index"].copy()

    # (3) the round trip it replaces (the host's choice code left out)
    host_tabs = [[table(k, indices[n][k]) for k in range(3)] for n in range(NPIC)]
    hjobs = [(co[k], qu[k], host_tabs[k // 3][k % 3], 0, None) for k in range(3 * NPIC)]
    hpics = [(qu[3 * n:3 * n + 3], host_tabs[n], DEPTH, HC, VC, 1, outs[n], cap, ress[n]) for n in range(NPIC)]

    def round_trip():
        sa.check(ctx.lib.schro_hip_histogram_batch(ctx.h, harr, 3 * NPIC, 2))
        ctx.synchronize()
        block.download()
        [s.free() for s in ctx.quantise_batch(hjobs)]
        ctx.noarith_encode_batch(hpics)
        ctx.synchronize()

    with Step("chain, round trip", a.limit):
        upload()
        t3, spread = host_clock(round_trip)
        lines.append("the same with the host round trip (histograms, synchronise, %d bytes of counts down, quantise and VLC encode from host "
                     "records; the host's choice code NOT included): %.4f ms per chain on the host clock, spread %.1f %%"
                     % (block.nbytes, t3, 100 * spread))
        lines.append("ratio enqueued / round trip: %.2f" % (t2 / t3))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
