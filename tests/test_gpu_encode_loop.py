"""GPU: the encoder's inter loop as a loop (schro_encoder_render_picture -> quantise -> schro_encoder_reconstruct_picture,
schroencoder.c:2430-2460, :2692-2726) on the device, three pictures deep, and the product's decoder path on the same
quantised values.  Per draw of tests/encode_loop_draws.py the whole group runs through the batch calls without a host
trip between stages -- upsample_batch of the references, obmc_batch (prediction_only 2), subtract_batch, iwt_batch,
histogram_batch, quantise_batch, then iiwt_batch, add_batch, convert_u8_batch on the encoder side and dequant_batch
(+ dc_predict_batch), iiwt_batch, obmc_batch with the residual (or convert_u8_batch) on the decoder side, into fresh
planes -- and the next picture's references are the encoder-side u8 reconstructions as they lie on the device.  What one
stage writes is therefore checked as what the next one reads: strides, the offset of 128, the zero padding and the crop,
band positions, the in-place reconstruction.  Everything is compared after the last stage only, exactly, and every
plane, blob, field, summary and count of a draw lies in ONE guarded block (tests/guard_lib.py) with its footprint.

Two device-side copies stand in for what a host would do with a host trip, both by add_batch into zeroed memory: the
coefficients are copied aside after the histogram call (quantise_batch then overwrites them with the reconstruction), and
the quant plane's codeblocks are repacked tight, row-major, into the decoder's hand-over.

tests/test_encode_loop_draws.py holds, on the CPU, that encoder and decoder side agree on the checkers for every draw:
a mismatch here is the device's.  SCHRO_FUZZ_SCALE multiplies the seeded draws, SCHRO_FUZZ_SEED shifts their seeds."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import analysis_ref as A
import encode_loop_draws as E
import guard_lib as G
import hist_ref as H
import quant_cases as QC
import rough_hint_ref as R
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

SCALE = int(os.environ.get("SCHRO_FUZZ_SCALE", "1"))
SEED = int(os.environ.get("SCHRO_FUZZ_SEED", "0"))

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(360 + 60 * SCALE)]

MV = sa.MV_DTYPE.itemsize
COUNTS = C.sizeof(_lib.HistogramCounts)


class View:
    """some rows of s16 samples inside a plane or blob of the block"""

    def __init__(self, base, offset, stride, width, height):
        self.ptr, self.stride, self.width, self.height, self.dtype = base.ptr + offset, stride, width, height, np.dtype(np.int16)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(1, -1)


def u8_stride(w):
    return -(-w // 16) * 16 + 16


class Group:
    """The planes of one draw's three pictures in one guarded block, and the calls of the loop."""

    def __init__(self, ctx, name, combine=False):
        self.ctx, self.name, self.combine = ctx, name, combine
        self.d, self.want, self.pics = E.get(name), E.expected(name), E.pictures(name)
        self.dims, self.iwt, self.P = E.dims(self.d), E.iwt_dims(self.d), E.motion_params(self.d)
        self.search = self.d["vectors"] == "search"
        self.lay, self.s, self.exp, self.hp, self.free = G.Layout(), {}, {}, {}, []
        for n in range(3):
            self.layout_picture(n)
        self.blk = G.GuardedBlock(ctx, self.lay, seed=zlib.crc32(name.encode()) & 0xffff)

    # -- layout ----------------------------------------------------------------------------------------------------------
    def plane(self, key, stage, h, w, dtype, stride=None, footprint="rect"):
        n, k = key
        self.s[n, k, stage] = self.lay.plane(h, w, dtype, stride=stride, footprint=footprint,
                                            name="%s: picture %d component %s stage %s" % (self.name, n, k, stage))

    def span(self, key, stage, nbytes, footprint, align=64):
        n, k = key
        self.s[n, k, stage] = self.lay.span(nbytes, align=align, footprint=("bytes", nbytes) if footprint else None,
                                           name="%s: picture %d component %s stage %s" % (self.name, n, k, stage))

    def layout_picture(self, n):
        d = self.d
        nb = 1 + 3 * d["depth"]
        if n:
            self.span((n, "-"), "vectors", self.P["x_num_blocks"] * self.P["y_num_blocks"] * MV, footprint=self.search and n == 1)
        if self.search and n == 1:
            self.span((n, "-"), "vectors of level 2", self.P["x_num_blocks"] * self.P["y_num_blocks"] * MV, footprint=True)
            h, w = self.dims[0]
            self.plane((n, 0), "picture", h, w, np.uint8, stride=u8_stride(w), footprint=None)
            for side in ("picture", "reference"):
                lh, lw = h, w
                for level in range(1, E.SEARCH_LEVELS + 1):
                    lh, lw = (lh + 1) // 2, (lw + 1) // 2
                    self.plane((n, 0), "%s pyramid level %d" % (side, level), lh, lw, np.uint8, stride=u8_stride(lw))
        for k in range(3):
            (h, w), (ih, iw) = self.dims[k], self.iwt[k]
            nrec = len(E.band_of_record(d))
            co_stride = iw * 2 + (6, 2, 10)[k]
            self.plane((n, k), "residual", ih, iw, np.int16, stride=iw * 2 + (0, 4, 2)[k], footprint="rect" if n else None)
            if n:
                self.plane((n, k), "prediction", h, w, np.int16, stride=w * 2 + (2, 0, 6)[k])
            self.plane((n, k), "coefficients", ih, iw, np.int16)
            self.span((n, k), "counts", nb * COUNTS, footprint=True)
            self.plane((n, k), "reconstruction", ih, iw, np.int16, stride=co_stride)
            self.plane((n, k), "quantised values", ih, iw, np.int16, stride=co_stride)
            self.span((n, k), "summaries", 8 * nrec, footprint=True)
            self.plane((n, k), "encoder sum", ih, iw, np.int16, stride=iw * 2 + (4, 0, 2)[k])
            self.plane((n, k), "encoder u8", h, w, np.uint8, stride=u8_stride(w))
            self.span((n, k), "tight values", 2 * ih * iw, footprint=True)
            self.plane((n, k), "decoder coefficients", ih, iw, np.int16, stride=iw * 2 + (2, 6, 0)[k])
            # (the combine form never writes a residual plane)
            self.plane((n, k), "decoder residual", ih, iw, np.int16, stride=iw * 2 + (0, 2, 4)[k],
                       footprint=None if self.combine and n else "rect")
            if self.combine and n:
                self.plane((n, k), "decoder prediction", h, w, np.uint8, stride=u8_stride(w))
            self.plane((n, k), "decoder u8", h, w, np.uint8, stride=u8_stride(w))

    def __call__(self, n, k, stage):
        return self.blk[self.s[n, k, stage]]

    def expect(self, n, k, stage, value):
        self.exp[self.s[n, k, stage]] = value

    def zero(self, p):
        sa.check(self.ctx.lib.schro_hip_memset(self.ctx.h, p.ptr, 0, p.spec.extent))

    # -- references ------------------------------------------------------------------------------------------------------
    def reference(self, m):
        """[component] of what obmc_batch reads of the encoder-side reconstruction of picture m: the u8 planes themselves at
        full pel, else their half-pel images (chroma of 4:2:0 and 4:2:2 as one pair image), made once"""
        planes = [self(m, k, "encoder u8") for k in range(3)]
        if self.d["prec"] == 0:
            return planes
        if m not in self.hp:
            ctx = self.ctx
            g0 = ctx.hp_plane(*self.dims[0])
            ctx.upsample_batch([(planes[0], g0)])
            if E.CHROMA[self.d["fmt"]][0] == 1:
                gp = ctx.hp_plane(*self.dims[1], pair=True)
                ctx.upsample_batch([((planes[1], planes[2]), gp)])
                self.hp[m] = [g0, gp, gp]
                self.free += [g0, gp]
            else:
                g1, g2 = ctx.hp_plane(*self.dims[1]), ctx.hp_plane(*self.dims[2])
                ctx.upsample_batch([(planes[1], g1), (planes[2], g2)])
                self.hp[m] = [g0, g1, g2]
                self.free += [g0, g1, g2]
        return self.hp[m]

    def vectors(self, n):
        """the device field of picture n: uploaded, or (the search draw's picture 1) written by rough_me_batch over pyramids
        from downsample_batch and never downloaded in between"""
        field = self(n, "-", "vectors")
        mv = self.want[n][1]
        if not (self.search and n == 1):
            field.upload(as_bytes(mv))
            return field
        ctx = self.ctx
        top = {"picture": self(n, 0, "picture").upload(self.pics[n][0]), "reference": self(0, 0, "encoder u8")}
        levels = []
        for level in range(1, E.SEARCH_LEVELS + 1):
            pair = []
            for side in ("picture", "reference"):
                dst = self(n, 0, "%s pyramid level %d" % (side, level))
                ctx.downsample_batch([(top[side], dst, 0)])
                top[side] = dst
                pair.append(dst)
            levels.append((pair[0], pair[1], 0))
        want = R.rough_scan(A.pyramid(self.pics[n][0], E.SEARCH_LEVELS), A.pyramid(self.want[0][0][0]["enc_u8"], E.SEARCH_LEVELS),
                              E.search_params(self.d), E.SEARCH_LEVELS, 0, 0)
        for level in range(1, E.SEARCH_LEVELS + 1):
            for side, plane in (("picture", self.pics[n][0]), ("reference", self.want[0][0][0]["enc_u8"])):
                self.expect(n, 0, "%s pyramid level %d" % (side, level), A.pyramid(plane, level)[level])
        ctx.rough_me_batch([(levels, E.search_params(self.d), 0, [field, self(n, "-", "vectors of level 2")])])
        self.expect(n, "-", "vectors", as_bytes(mv))
        self.expect(n, "-", "vectors of level 2", as_bytes(want[2]))
        return field

    # -- one picture -----------------------------------------------------------------------------------------------------
    def code(self, n):
        ctx, d, lib = self.ctx, self.d, self.ctx.lib
        comps = self.want[n][0]
        depth, filt = d["depth"], d["filt"]
        for k in range(3):
            self(n, k, "residual").upload(comps[k]["src"])
        if n:
            refs = [self.reference(m) for m in range(n)] + [[None] * 3] * (2 - n)
            mvs = self.vectors(n)
            ctx.obmc_batch([sa.obmc_plane(mvs, self.P, k, refs[0][k], refs[1][k], None, self(n, k, "prediction"), prediction_only=2)
                            for k in range(3)])
            ctx.subtract_batch([(self(n, k, "residual"), self(n, k, "prediction")) for k in range(3)])
        ctx.iwt_batch([(self(n, k, "residual"), self(n, k, "reconstruction")) for k in range(3)], depth, filt)
        # the histograms; then the coefficients aside, as the histogram call left them
        harr, qarr, keep = (_lib.HistogramPlane * 3)(), (_lib.QuantPlane * 3)(), []
        for k in range(3):
            co = self(n, k, "reconstruction")
            bands = E.hist_bands(d, n, k, co.stride)
            tab = (_lib.HistogramBand * len(bands))(*[_lib.HistogramBand(*(int(v) for v in b)) for b in bands])
            keep.append(tab)
            a = harr[k]
            a.coeffs, a.bytes, a.bands, a.nbands, a.counts = co.ptr, co.spec.extent, tab, len(bands), self(n, k, "counts").ptr
        sa.check(lib.schro_hip_histogram_batch(ctx.h, harr, 3, 2))
        for k in range(3):
            self.zero(self(n, k, "coefficients"))
        ctx.add_batch([(self(n, k, "coefficients"), self(n, k, "reconstruction")) for k in range(3)])
        recs = []
        for k in range(3):
            co, qu = self(n, k, "reconstruction"), self(n, k, "quantised values")
            recs.append(E.records(d, n, k, co.stride))
            tab = QC.table(recs[k])
            keep.append(tab)
            a = qarr[k]
            a.coeffs, a.quant, a.bytes, a.codeblocks, a.ncodeblocks, a.is_intra = co.ptr, qu.ptr, co.spec.extent, tab, len(tab), int(n == 0)
            dc = E.dc_of(d, n, k)
            if dc:
                a.dc_predict_first, a.dc_width, a.dc_height = dc
            a.summary = self(n, k, "summaries").ptr
        sa.check(lib.schro_hip_quantise_batch(ctx.h, qarr, 3, 2))
        # the encoder's local decode
        ctx.iiwt_batch([(self(n, k, "reconstruction"), self(n, k, "encoder sum")) for k in range(3)], depth, filt)
        if n:
            ctx.add_batch([(self(n, k, "encoder sum"), self(n, k, "prediction")) for k in range(3)])
        ctx.convert_u8_batch([(self(n, k, "encoder sum"), self(n, k, "encoder u8")) for k in range(3)])
        # the decoder, into fresh planes, from the quant plane's values repacked tight
        jobs, pairs = [], []
        for k in range(3):
            blob, qu = self(n, k, "tight values"), self(n, k, "quantised values")
            self.zero(blob)
            dec, drecs, off = self(n, k, "decoder coefficients"), [], 0
            for (o, st, w, h, qi), (do, ds, _, _, _) in zip(recs[k], E.records(d, n, k, dec.stride)):
                pairs.append((View(blob, off, 2 * w, w, h), View(qu, o, st, w, h)))
                drecs.append((do, ds, w, h, off, 2, qi))
                off += 2 * w * h
            jobs.append((dec, blob, drecs, n == 0))
        ctx.add_batch(pairs)
        ctx.dequant_batch(jobs, arith=0)
        if n == 0:
            ctx.dc_predict_batch([View(self(n, k, "decoder coefficients"), 0, self(n, k, "decoder coefficients").stride << depth,
                                       self.iwt[k][1] >> depth, self.iwt[k][0] >> depth) for k in range(3)])
        if self.combine and n:
            ctx.obmc_batch([sa.obmc_plane(mvs, self.P, k, refs[0][k], refs[1][k], None, self(n, k, "decoder prediction"), prediction_only=1)
                            for k in range(3)])
            ctx.iiwt_batch([(self(n, k, "decoder coefficients"), self(n, k, "decoder u8"), self(n, k, "decoder prediction"))
                            for k in range(3)], depth, filt)
        else:
            ctx.iiwt_batch([(self(n, k, "decoder coefficients"), self(n, k, "decoder residual")) for k in range(3)], depth, filt)
            if n:
                ctx.obmc_batch([sa.obmc_plane(mvs, self.P, k, refs[0][k], refs[1][k], self(n, k, "decoder residual"), self(n, k, "decoder u8"))
                                for k in range(3)])
            else:
                ctx.convert_u8_batch([(self(n, k, "decoder residual"), self(n, k, "decoder u8")) for k in range(3)])
        # what the checkers say, in the order of the stages
        for k, c in enumerate(comps):
            if n:
                self.expect(n, k, "prediction", c["pred"])
            self.expect(n, k, "residual", c["residual"])
            self.expect(n, k, "coefficients", c["coeffs"])
            self.expect(n, k, "counts", as_bytes(c["counts"]))
            self.expect(n, k, "quantised values", c["quant"])
            self.expect(n, k, "reconstruction", c["recon"])
            self.expect(n, k, "summaries", as_bytes(c["summaries"]))
            self.expect(n, k, "encoder sum", c["enc_sum"])
            self.expect(n, k, "encoder u8", c["enc_u8"])
            self.expect(n, k, "tight values", as_bytes(c["blob"]))
            self.expect(n, k, "decoder coefficients", c["dec_coeffs"])
            if not (self.combine and n):
                self.expect(n, k, "decoder residual", c["dec_res"])
            self.expect(n, k, "decoder u8", c["dec_u8"])

    def run(self):
        try:
            for n in range(3):
                self.code(n)
            self.ctx.synchronize()
            raw = self.blk.raw()
            G.report(*G.find_changes(self.lay, self.blk.before, raw, self.exp))
            for n in range(3):
                for k in range(3):
                    a, b = self.s[n, k, "encoder u8"].payload(raw), self.s[n, k, "decoder u8"].payload(raw)
                    assert np.array_equal(a, b), "%s: picture %d component %d stage encoder u8 against decoder u8: the encoder's reconstruction is not the decoder's picture" % (self.name, n, k)
        finally:
            self.blk.free()
            for p in self.free:
                p.free()


def test_loop_on_the_plane_layer(ctx):
    for name in E.names(SCALE, SEED):
        Group(ctx, name).run()


@pytest.mark.parametrize("name", E.COMBINE_FORM)
def test_decoder_combine_form_agrees(ctx, name):
    """The decoder side of pictures 1 and 2 through the combine form (obmc_batch with prediction_only 1, then iiwt_batch
    adding the prediction in its last step, tests/test_gpu_combine.py): the same bytes."""
    Group(ctx, name, combine=True).run()


def test_loop_on_the_frame_layer(ctx):
    """The same group through the SchroFrame-shaped calls: schro_frame_to_hip, schro_upsampled_hipframe_upsample,
    schro_motion_render_hip in its prediction form into mc_tmp, schro_hipframe_subtract, schro_hipframe_iwt_transform,
    schro_hipframe_subband_histograms, schro_hipframe_quantise, schro_frame_inverse_iwt_transform_hip, schro_hipframe_add,
    schro_hipframe_convert; the decoder side schro_hipframe_dequantise, schro_frame_inverse_iwt_transform_hip and
    schro_motion_render_hip with add = TRUE.  The assertions are the plane layer's, on the downloaded frames."""
    name = E.FRAME_LAYER
    d, want = E.get(name), E.expected(name)
    lib, depth = ctx.lib, d["depth"]
    hs, vs = E.CHROMA[d["fmt"]]
    dm, im, P = E.dims(d), E.iwt_dims(d), E.motion_params(d)
    fmt16, fmt8 = frames.frame_format(np.int16, hs, vs), frames.frame_format(np.uint8, hs, vs)
    (lh, lw), (ch, cw) = im[0], im[1]
    held, recons, ups = [], [], []

    def frame(fmt, w, h, **kw):
        f = frames.DeviceFrame(ctx, fmt, w, h, **kw)
        held.append(f)
        return f

    def same(got, key, n, stage, crop=False):
        for k in range(3):
            g = got[k][:dm[k][0], :dm[k][1]] if crop else got[k]
            assert np.array_equal(g, want[n][0][k][key]), "%s: picture %d component %d stage %s" % (name, n, k, stage)

    try:
        for n in range(3):
            comps, mv = want[n]
            params = frames.make_params(
                wavelet_filter_index=d["filt"], transform_depth=depth, iwt_luma_width=lw, iwt_luma_height=lh, iwt_chroma_width=cw,
                iwt_chroma_height=ch, num_refs=n, xblen_luma=P["xblen_luma"], yblen_luma=P["yblen_luma"], xbsep_luma=P["xbsep_luma"],
                ybsep_luma=P["ybsep_luma"], mv_precision=d["prec"], picture_weight_bits=1, picture_weight_1=1, picture_weight_2=1,
                x_num_blocks=P["x_num_blocks"], y_num_blocks=P["y_num_blocks"])
            for l in range(depth + 1):
                params.horiz_codeblocks[l], params.vert_codeblocks[l] = d["hc"][l], d["vc"][l]
            iwt = frame(fmt16, lw, lh).upload(frames.HostFrame([c["src"] for c in comps], hs, vs))
            assert [(iwt.c.components[k].height, iwt.c.components[k].width) for k in range(3)] == im
            if n:
                while len(ups) < n:
                    m = len(ups)
                    if d["prec"] > 0:
                        u = frame(fmt8, d["w"], d["h"], upsampled=True)
                        sa.check(lib.schro_upsampled_hipframe_upsample(u.ptr(), recons[m].ptr()))
                        ups.append(u)
                    else:
                        ups.append(recons[m])
                mc_tmp = frame(fmt16, d["w"], d["h"])
                motion = _lib.Motion(ups[0].ptr(), ups[1].ptr() if n == 2 else None, mv.ctypes.data, C.pointer(params))
                sa.check(lib.schro_motion_render_hip(C.byref(motion), mc_tmp.ptr(), None, 0, None))
                same(mc_tmp.download(), "pred", n, "prediction", crop=True)
                sa.check(lib.schro_hipframe_subtract(iwt.ptr(), mc_tmp.ptr()))
            same(iwt.download(), "residual", n, "residual")
            sa.check(lib.schro_hipframe_iwt_transform(ctx.h, iwt.ptr(), C.byref(params)))
            hn, hbins, hovf = ctx.subband_histograms(iwt, params)
            same(iwt.download(), "coeffs", n, "coefficients")
            wn, wbins, wovf = H.frame_histograms([c["coeffs"] for c in comps], depth, n == 0)
            assert np.array_equal(hn, wn) and np.array_equal(hbins, wbins) and np.array_equal(hovf, wovf), "%s: picture %d stage counts" % (name, n)
            quant = frame(fmt16, lw, lh)
            recs = [E.records(d, n, k, iwt.c.components[k].stride) for k in range(3)]
            idx = [(C.c_int * len(r))(*[rec[4] for rec in r]) for r in recs]
            summ = [ctx.host_array((len(r), 2), np.uint32) for r in recs]
            qi = (C.POINTER(C.c_int) * 3)(*[C.cast(a, C.POINTER(C.c_int)) for a in idx])
            sp = (C.POINTER(_lib.CodeblockSummary) * 3)(*[C.cast(a.ctypes.data, C.POINTER(_lib.CodeblockSummary)) for a in summ])
            sa.check(lib.schro_hipframe_quantise(quant.ptr(), iwt.ptr(), C.byref(params), qi, sp))
            ctx.synchronize()
            got_q = quant.download()
            same(got_q, "quant", n, "quantised values")
            same(iwt.download(), "recon", n, "reconstruction")
            for k in range(3):
                assert np.array_equal(summ[k], comps[k]["summaries"]), "%s: picture %d component %d stage summaries" % (name, n, k)
            # the encoder's local decode
            rec = frame(fmt16, lw, lh)
            sa.check(lib.schro_frame_inverse_iwt_transform_hip(rec.ptr(), iwt.ptr(), C.byref(params)))
            if n:
                sa.check(lib.schro_hipframe_add(rec.ptr(), mc_tmp.ptr()))
            same(rec.download(), "enc_sum", n, "encoder sum")
            enc = frame(fmt8, d["w"], d["h"])
            sa.check(lib.schro_hipframe_convert(enc.ptr(), rec.ptr()))
            recons.append(enc)
            got_enc = enc.download()
            same(got_enc, "enc_u8", n, "encoder u8")
            # the decoder: the quantised values of the quant frame, tight, through schro_hipframe_dequantise
            tf = frame(fmt16, lw, lh)
            qp, keep = _lib.QuantisedPicture(), []
            for k in range(3):
                blob, tight = QC.tight_values(got_q[k], E.records(d, n, k, im[k][1] * 2), 2)
                tab = sa.Context.codeblock_table([(r[0], r[1], r[2], r[3], t[4], 2, r[4]) for r, t in zip(recs[k], tight)])
                keep += [blob, tab]
                qp.codeblocks[k], qp.ncodeblocks[k] = C.cast(tab, C.POINTER(_lib.Codeblock)), len(tab)
                qp.values[k], qp.values_bytes[k] = blob.ctypes.data, blob.size
            qp.values_on_device = 0
            sa.check(lib.schro_hipframe_dequantise(tf.ptr(), C.byref(qp), C.byref(params)))
            same(tf.download(), "dec_coeffs", n, "decoder coefficients")
            res = frame(fmt16, lw, lh)
            sa.check(lib.schro_frame_inverse_iwt_transform_hip(res.ptr(), tf.ptr(), C.byref(params)))
            same(res.download(), "dec_res", n, "decoder residual")
            dec = frame(fmt8, d["w"], d["h"])
            if n:
                sa.check(lib.schro_motion_render_hip(C.byref(motion), None, res.ptr(), 1, dec.ptr()))
            else:
                sa.check(lib.schro_hipframe_convert(dec.ptr(), res.ptr()))
            got_dec = dec.download()
            same(got_dec, "dec_u8", n, "decoder u8")
            for k in range(3):
                assert np.array_equal(got_enc[k], got_dec[k]), "%s: picture %d component %d stage encoder u8 against decoder u8: the encoder's reconstruction is not the decoder's picture" % (name, n, k)
    finally:
        for f in held:
            f.unref()
