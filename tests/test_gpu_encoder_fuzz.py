"""GPU parity of the encoder-side kernels under random geometry: seeded draws of the forward wavelet (filters, depths 1 - 6,
sample sizes, unlike planes in one call, strides and leads that are no multiple of anything, pixel- and full-range input),
the downsample (sizes, aprons, destination alignments and strides, batches), the SAD scan (pictures, blocks from empty to
64 x 64, windows, gravity positions, pictures full of ties), the frame layer's pyramid and rough scan, and the encoder's
tail -- the codeblock quantiser (quant.hip: layouts, depths, both sample types, intra DC bands down to one sample a side), the
sub-band histograms (hist.hip: every sub-band of random transforms, both forms, planes of equal samples) and the VC-2
low-delay slice encoder (lowdelay_enc.hip: chroma formats, depths, slice counts beyond the LL band, fractional slice
sizes, matrices, unlike pictures in one call, the serial launch in LDS and off it) -- each compared bit for bit with
tests/oracle_lib.py, tests/analysis_ref.py, tests/quant_ref.py, tests/hist_ref.py or tests/lowdelay_enc_ref.py.  The tail's
draws come from tests/encoder_tail_draws.py, which tests/dry_run_encoder_tail_cases.py walks without a device.  The decoder side's draws are tests/test_gpu_fuzz.py; the
conventions are the same: SCHRO_FUZZ_SCALE multiplies the number of draws, SCHRO_FUZZ_SEED shifts the seeds (a long
campaign is `SCHRO_FUZZ_SCALE=50 SCHRO_FUZZ_SEED=7 pytest tests/test_gpu_encoder_fuzz.py -m gpu`), and every failure
message carries its draw."""
import ctypes as C
import os

import numpy as np
import pytest

import analysis_ref as A
import encoder_tail_draws as D
import hist_cases as HC
import lowdelay_enc_ref as R
import oracle_lib as O
import quant_cases as QC
import schroedinger_amd as sa
import synth
from schroedinger_amd import frames
from test_gpu_analysis_edges import check_scans, dst_view, make_scans
from test_gpu_iwt_forward import pixel_range
from test_gpu_lowdelay_encode import run as run_lowdelay_encode

SCALE = int(os.environ.get("SCHRO_FUZZ_SCALE", "1"))
SEED = int(os.environ.get("SCHRO_FUZZ_SEED", "0"))

# (tests/conftest.py gives every test six minutes; a campaign's tests get theirs by its size)
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(360 + 60 * SCALE)]

FILL = 0x5a


def padded(ctx, a, lead, pad, rng):
    """`a` uploaded `lead` samples into a parent whose rows are lead + width + pad samples of random values: (parent, view)."""
    h, w = a.shape
    whole = rng.integers(-100, 100, (h, lead + w + pad)).astype(a.dtype)
    whole[:, lead:lead + w] = a
    parent = ctx.upload(whole, stride=whole.shape[1] * a.dtype.itemsize) if (lead or pad) else ctx.upload(whole)
    return parent, sa.SubPlane(parent, 0, lead, h, w)


def test_forward_wavelet_random_batches(ctx):
    rng = np.random.default_rng(1201 + SEED)
    for rnd in range(60 * SCALE):
        filt, depth = int(rng.integers(0, 7)), int(rng.integers(1, 7))
        dtype = [np.int16, np.int32][int(rng.integers(0, 2))]
        full = bool(rng.integers(0, 2))          # (filter 5 as well: tests/test_gpu_iwt_forward.py says why)
        unit = 1 << depth
        todo, tag = [], (rnd, filt, depth, np.dtype(dtype).name, "full" if full else "pixel")
        for _ in range(int(rng.integers(1, 6))):
            h = min(unit * int(rng.integers(1, 24)), 1024 // unit * unit)
            w = min(unit * int(rng.integers(1, 40)), 1536 // unit * unit)
            seed = int(rng.integers(1, 1 << 20))
            img = synth.full_range(h, w, dtype, seed) if full else pixel_range(h, w, dtype, seed)
            s_lead, s_pad, d_lead, d_pad = (int(v) for v in rng.integers(0, 4, 4))
            sp, sv = padded(ctx, img, s_lead, s_pad, rng)
            dp = ctx.plane(h, d_lead + w + d_pad, dtype, stride=(d_lead + w + d_pad) * np.dtype(dtype).itemsize if (d_lead or d_pad) else None).fill(FILL)
            todo.append((img, sp, sv, dp, sa.SubPlane(dp, 0, d_lead, h, w), d_lead))
        ctx.iwt_batch([(sv, dv) for (_, _, sv, _, dv, _) in todo], depth, filt)
        inverse = rnd % 3 == 0
        backs = [ctx.plane(t[0].shape[0], t[0].shape[1], dtype).fill(0xa5) for t in todo] if inverse else []
        if inverse:
            ctx.iiwt_batch([(t[4], b) for t, b in zip(todo, backs)], depth, filt)
        for n, (img, sp, sv, dp, dv, lead) in enumerate(todo):
            want = O.forward_iwt(img, depth, filt)
            whole = dp.download()
            w = img.shape[1]
            assert np.array_equal(whole[:, lead:lead + w], want), tag + (n, img.shape, "coefficients")
            rest = np.frombuffer(np.delete(whole, np.s_[lead:lead + w], axis=1).tobytes(), np.uint8)
            assert (rest == FILL).all(), tag + (n, img.shape, "written beside the plane")
            if inverse:
                assert np.array_equal(backs[n].download(), O.inverse_iwt(want, depth, filt)), tag + (n, img.shape, "inverse")
        [p.free() for t in todo for p in (t[1], t[3])]
        [p.free() for p in backs]


def test_downsample_random_batches(ctx):
    rng = np.random.default_rng(1302 + SEED)
    aprons = list(range(10)) + [16, 32, 40]
    for rnd in range(60 * SCALE):
        todo = []
        for _ in range(int(rng.integers(1, 9))):
            w, h = int(rng.integers(1, 701)), int(rng.integers(1, 301))
            ext = aprons[int(rng.integers(0, len(aprons)))]
            kind = int(rng.integers(0, 3))
            src = [A.picture(w, h, int(rng.integers(1, 1 << 20))), A.checkerboard(w, h), np.full((h, w), 255, np.uint8)][kind]
            skew, pad = int(rng.integers(0, 8)), int(rng.integers(0, 8))
            parent, view = dst_view(ctx, (h, w), ext, skew, pad, fill=FILL)
            todo.append((src, ctx.upload(src), parent, view, ext, skew, kind))
        ctx.downsample_batch([(d_src, view, ext) for (_, d_src, _, view, ext, _, _) in todo])
        for n, (src, d_src, parent, view, ext, skew, kind) in enumerate(todo):
            tag = (rnd, n, len(todo), src.shape, ext, skew, parent.stride, kind)
            whole = parent.download()
            assert np.array_equal(whole[:, skew:skew + view.width], A.edgeextend(A.downsample(src), ext)), tag
            assert (np.delete(whole, np.s_[skew:skew + view.width], axis=1) == FILL).all(), tag + ("written beside the plane",)
            d_src.free()
            parent.free()


def test_metric_scan_random_batches(ctx):
    rng = np.random.default_rng(1403 + SEED)

    def picture(w, h):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            return A.picture(w, h, int(rng.integers(1, 1 << 20)))
        if kind == 1:           # low contrast: many ties
            return rng.integers(100, 104, (h, w), dtype=np.uint8)
        return np.full((h, w), int(rng.integers(0, 256)), np.uint8)

    def block_size(limit):
        return min(int(rng.integers(4, 17)) if rng.random() < 0.7 else int(rng.integers(0, 65)), limit)

    for rnd in range(40 * SCALE):
        pics, held = [], []
        for _ in range(int(rng.integers(1, 4))):
            w, h = int(rng.integers(16, 201)), int(rng.integers(16, 121))
            ext = [0, 4, 8, 32][int(rng.integers(0, 4))]
            dicts = []
            for _ in range(int(rng.integers(1, 301))):
                bw, bh = block_size(w), block_size(h)
                x, y = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
                vx, vy, dist = int(rng.integers(-24, 25)), int(rng.integers(-24, 25)), int(rng.integers(1, 21))
                rx, ry, sw, sh = sa.metric_scan_setup(x, y, bw, bh, w, h, ext, vx, vy, dist)
                assert (rx, ry, sw, sh) == A.scan_setup(x, y, bw, bh, w, h, ext, vx, vy, dist)
                if sw <= 0 or sh <= 0:
                    continue            # an empty window is not handed to the batch (include/schro_hip.h)
                dicts.append(dict(x=x, y=y, block_width=bw, block_height=bh, ref_x=rx, ref_y=ry, scan_width=sw, scan_height=sh,
                                  gravity_x=rx + int(rng.integers(0, sw)) - x, gravity_y=ry + int(rng.integers(0, sh)) - y,
                                  dx=int(rng.integers(-99, 100)), dy=int(rng.integers(-99, 100))))
            if not dicts:
                continue
            frame, ref = picture(w, h), picture(w, h)
            df, dr = ctx.upload(frame), ctx.upload(ref)
            held += [df, dr]
            pics.append((frame, ref, df, dr, ext, make_scans(dicts)))
        if pics:
            check_scans(ctx, pics, tag=("draw", rnd, [(p[0].shape, p[4], len(p[5])) for p in pics]))
        [p.free() for p in held]


def test_frame_layer_random_pyramids_and_rough_scans(ctx):
    """schro_hipframe_downsample down to the level of the rough scan and schro_rough_me_heirarchical_scan_nohint_hip on that
    level's frames: 4:4:4 / 4:2:2 / 4:2:0 frames of random even sizes, every component of every level and the motion
    field against analysis_ref."""
    rng = np.random.default_rng(1504 + SEED)
    lib = ctx.lib
    for rnd in range(20 * SCALE):
        hs, vs = [(0, 0), (1, 0), (1, 1)][int(rng.integers(0, 3))]
        w, h = 2 * int(rng.integers(8, 64)), 2 * int(rng.integers(8, 40))
        sep = [4, 8, 12, 16][int(rng.integers(0, 4))]
        shift, distance, ref_index = int(rng.integers(0, 4)), int(rng.integers(1, 11)), int(rng.integers(0, 2))
        ext = [0, 8, 32][int(rng.integers(0, 3))]
        nbx, nby = -(-w // sep) + int(rng.integers(0, 5)), -(-h // sep) + int(rng.integers(0, 5))       # they overhang the picture
        tag = (rnd, (w, h), (hs, vs), sep, (nbx, nby), shift, distance, ref_index, ext)
        fmt = frames.frame_format(np.uint8, hs, vs)
        levels, held = [], []
        for seed in (int(rng.integers(1, 1 << 20)), int(rng.integers(1, 1 << 20))):
            comps = [A.picture(w, h, seed), A.picture(w >> hs, h >> vs, seed + 1), A.picture(w >> hs, h >> vs, seed + 2)]
            fr = frames.DeviceFrame(ctx, fmt, w, h).upload(frames.HostFrame(comps, hs, vs))
            chain = [(fr, comps, 0)]
            for n in range(shift):
                comps = [A.downsample(c) for c in comps]
                planes = [ctx.plane(c.shape[0] + 2 * ext, c.shape[1] + 2 * ext, np.uint8).fill(FILL) for c in comps]
                dest = frames.PlaneFrame(ctx, planes, ext, hs, vs)
                sa.check(lib.schro_hipframe_downsample(dest.ptr(), chain[-1][0].ptr()))
                for k, (p, c) in enumerate(zip(planes, comps)):
                    assert np.array_equal(p.download(), A.edgeextend(c, ext)), tag + ("level", n + 1, "component", k)
                held += planes
                chain.append((dest, comps, ext))
            levels.append((fr, chain[-1]))
        (fa, (la, ca, ea)), (fb, (lb, cb, _)) = levels
        P = frames.make_params(x_num_blocks=nbx, y_num_blocks=nby, xbsep_luma=sep, ybsep_luma=sep)
        got = np.zeros(nbx * nby, sa.MV_DTYPE)
        got["metric"] = 12345
        sa.check(lib.schro_rough_me_heirarchical_scan_nohint_hip(la.ptr(), lb.ptr(), C.byref(P), shift, distance, ref_index,
                                                                 got.ctypes.data_as(C.c_void_p)))
        want = A.rough_scan_nohint(ca[0], cb[0], dict(x_num_blocks=nbx, y_num_blocks=nby, xbsep_luma=sep, ybsep_luma=sep),
                                   shift, distance, ref_index, extension=ea)
        assert got.tobytes() == want.tobytes(), tag
        fa.unref(), fb.unref()
        [p.free() for p in held]


def tagged(tag, call):
    """call (); an AssertionError leaves with the draw in front of its message"""
    try:
        return call()
    except AssertionError as e:
        raise AssertionError("%r: %s" % (tag, e)) from e


def test_lowdelay_encode_random_pictures(ctx):
    """schro_hip_lowdelay_encode_batch on the draws of encoder_tail_draws.lowdelay_draws, through the runner of
    tests/test_gpu_lowdelay_encode.py (guarded memory: nothing beside the slices, the indices and the count is written,
    the padded coefficient planes stay as they were): bytes, base indices and the over-run count of every picture equal
    tests/lowdelay_enc_ref.py's.  Slices that over-run are cut and counted by both, so such draws are compared in full."""
    for draw in D.lowdelay_draws(SCALE, SEED):
        pictures = D.lowdelay_pictures(draw)
        got = tagged(draw["tag"], lambda: run_lowdelay_encode(ctx, draw["P"], pictures, pads=draw["pads"], skew=draw["skew"]))
        for n, (planes, (data, index, count)) in enumerate(zip(pictures, got)):
            res = R.encode(planes, draw["P"])
            tag = draw["tag"] + ("picture", n)
            assert index.tolist() == res["index"].tolist(), tag + ("indices", index.tolist(), res["index"].tolist())
            assert count == res["count"], tag + ("over-run count", count, res["count"])
            assert data.size == res["bytes"].size, tag + ("bytes", data.size, res["bytes"].size)
            bad = np.flatnonzero(data != res["bytes"])
            assert bad.size == 0, tag + ("%d bytes differ, first at %d" % (bad.size, bad[0] if bad.size else -1),)


def test_quantise_random_codeblocks(ctx):
    """schro_hip_quantise_batch on the draws of encoder_tail_draws.quantise_draws through quant_cases.run_specs: quantised
    values (the quant plane keeps its fill outside the records), the reconstruction left in the coefficient plane and the
    codeblock summaries equal tests/quant_ref.py's"""
    for draw in D.quantise_draws(SCALE, SEED):
        tagged(draw["tag"], lambda: QC.run_specs(ctx, draw["specs"]))


def test_histogram_random_bands(ctx):
    """schro_hip_histogram_batch on the draws of encoder_tail_draws.histogram_draws through hist_cases.run_specs: the counts
    of every band equal tests/hist_ref.py's.  The counts of all planes of a call lie one behind the other in one block and
    every row of it is compared, so a count that lands in a neighbour's row shows; the planes are uploaded tight, so a
    band's last row ends its allocation."""
    for draw in D.histogram_draws(SCALE, SEED):
        tagged(draw["tag"], lambda: HC.run_specs(ctx, draw["specs"]))
