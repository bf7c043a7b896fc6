"""GPU: the VLC decoder chain -- schro_hip_motion_decode_batch and schro_hip_noarith_decode_batch in front of the inverse
wavelet and OBMC -- from bytes to pixels, bit for bit, and the four VLC stages on data the reference produced.

The bytes are the noarith twin of the reference's own stream (tests/noarith_twin.py, pinned on the CPU by
tests/test_noarith_twin.py): its pictures 0, 1 and 2, decoded on the device from VLC bytes, must carry the digests the
reference's own decoder printed for them (tests/golden/stream_md5.json, "reference").  What the stream lacks -- splits 0
and 1, sub-pel vectors, 4:2:0 and 4:4:4, quant offsets, several codeblocks in sub-band 0, s32 -- comes from drawn
pictures, whose expected values are the restatements' and the oracle's.

A transform has one depth and one filter per iiwt_batch call, so unlike pictures take a call each there; every other stage
takes the pictures of a pass in one call."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import guard_lib as G
import motion_dec_ref as MD
import motion_enc_cases as MC
import motion_enc_ref as ME
import noarith_dec_ref as ND
import noarith_enc_cases as NC
import noarith_enc_ref as NE
import noarith_twin as T
import oracle_lib as O
import schroedinger_amd as sa
import stream_lib as S
import synth
from schroedinger_amd import _lib
from test_gpu_motion_decode import same
from test_gpu_noarith_decode import same_result
from test_gpu_obmc import Ref, comp_size

pytestmark = pytest.mark.gpu

MWORDS = C.sizeof(_lib.MotionDecodeResult) // 4
EWORDS = C.sizeof(_lib.MotionEncodeResult) // 4
TWORDS = C.sizeof(_lib.NoarithDecodeResult) // 4
NWORDS = C.sizeof(_lib.NoarithResult) // 4
RECORD = sa.MV_DTYPE.itemsize
CLEAN = dict(error=0, truncated=0, not_consumed=0, overran=0, long_codes=0, clamped_quant=0)


def as_row(data):
    return np.frombuffer(bytes(data), np.uint8).reshape(1, -1)


def twelve():
    recs = list(T.pictures(limit=12))
    assert [r["number"] for r in recs] == T.FIRST_TWELVE
    assert [r["num_refs"] for r in recs].count(1) == 3 and [r["num_refs"] for r in recs].count(2) == 8 and recs[0]["num_refs"] == 0
    return recs


# ---- the stages on the twin, between guard blocks ---------------------------------------------------------------------------

def test_motion_data_of_stream_pictures(ctx):
    """The eight pictures of noarith_twin.MOTION_EIGHT: one motion_encode_batch over the stream's fields writes the twin's
    bytes, one motion_decode_batch reads those device bytes through the encoder's `bytes` word and gives the fields back;
    no wait between the two."""
    by_number = {r["number"]: r for r in T.motion_pictures(numbers=set(T.MOTION_EIGHT))}
    recs = [by_number[n] for n in T.MOTION_EIGHT]
    lay, spans = G.Layout(), []
    for n, r in enumerate(recs):
        nbytes = r["nbx"] * r["nby"] * RECORD
        room = sa.motion_encode_bound(r["nbx"], r["nby"], r["num_refs"], 0)
        assert room >= len(r["motion"])
        spans.append((lay.span(nbytes, align=64, footprint=None, name="field%d" % n),
                      lay.span(room, align=64, skew=n % 4, footprint=("bytes", len(r["motion"])), name="bytes%d" % n),
                      lay.plane(1, EWORDS, np.uint32, footprint="rect", name="encoded%d" % n),
                      lay.span(nbytes, align=64, footprint=("bytes", nbytes), name="decoded%d" % n),
                      lay.plane(1, MWORDS, np.uint32, footprint="rect", name="result%d" % n), room))
    block = G.GuardedBlock(ctx, lay, seed=96)
    try:
        enc, dec = [], []
        for r, (field, out, eres, back, dres, room) in zip(recs, spans):
            assert r["mv"].dtype == sa.MV_DTYPE
            block[field].upload(as_row(r["mv"].tobytes()))
            geometry = (r["nbx"], r["nby"], r["num_refs"], 0)
            enc.append((block[field],) + geometry + (block[out], room, block[eres]))
            # SchroHipMotionEncodeResult.bytes is the result's first word
            dec.append((block[out], room, block[eres]) + geometry + (block[back], block[dres]))
        ctx.synchronize()               # (the last wait in front of the two calls)
        assert ctx.motion_encode_batch(enc) is None
        assert ctx.motion_decode_batch(dec) is None
        ctx.synchronize()
        expected = {}
        for r, (field, out, eres, back, dres, room) in zip(recs, spans):
            n, data = r["number"], r["motion"]
            e = sa.motion_encode_result(block[eres].download())
            assert (e["bytes"], e["overrun"], e["section_bytes"]) == (len(data), 0, r["section_bytes"]), n
            assert (e["asserted"], e["unverified"], e["first_unverified"]) == (0, 0, -1), n
            tail = block.before[out.offset + len(data):out.offset + room]          # (the canary behind the bytes)
            expected[out] = np.concatenate([as_row(data)[0], tail]).reshape(1, -1)
            want = MD.decode(data, r["nbx"], r["nby"], r["num_refs"], 0)
            assert want[0].tobytes() == ME.canonical(r["mv"]).tobytes() == r["mv"].tobytes(), n
            assert (want[1]["truncated"], want[1]["overran"], want[1]["not_consumed"], want[1]["long_codes"], want[1]["unverified"]) == (0,) * 5
            same(block[back].download(), sa.motion_decode_result(block[dres].download()), want, "picture %d" % n)
        block.check(expected)
    finally:
        block.free()


def tables_of(ctx, rec, planes):
    """Per component the codeblock records of the picture with its sub-bands' quant indices."""
    P = rec["twin"]
    tabs = []
    for k, p in enumerate(planes):
        tab = ctx.codeblock_layout(p.width, p.height, P["depth"], P["horiz_cb"], P["vert_cb"], p.stride, p.dtype.itemsize)
        n = 0
        for i in range(1 + 3 * P["depth"]):
            hc, vc = NE.codeblock_counts(i, P["horiz_cb"], P["vert_cb"])
            for _ in range(hc * vc):
                tab[n].quant_index = rec["quant_indices"][k][i]
                n += 1
        assert n == len(tab)
        tabs.append(tab)
    return tabs


def test_transform_data_of_stream_pictures(ctx):
    """The first 12 pictures: noarith_decode_batch of the transform twins gives the stream's coefficients (behind
    dc_predict_batch for the intra picture); noarith_encode_batch of the stream's quant planes gives the restated
    encoder's bytes; the device decode of those bytes, their length taken from the encoder's word, the same planes."""
    recs = twelve()
    lay, specs = G.Layout(), []
    for n, r in enumerate(recs):
        P = r["twin"]
        shapes = [P["iwt"][0], P["iwt"][1], P["iwt"][1]]
        plane = lambda what, k, fp: lay.plane(shapes[k][0], shapes[k][1], np.int16, stride=shapes[k][1] * 2 + 64, footprint=fp,
                                              name="p%d-%s%d" % (n, what, k))
        written = NE.encode_transform_data([q.astype(np.int16) for q in r["quant"]], P["depth"], P["horiz_cb"], P["vert_cb"], P["cb_mode"],
                                           r["quant_indices"])[0]
        room = len(written) + 37
        specs.append(dict(data=lay.span(len(r["transform"]), align=64, skew=n % 4, footprint=None, name="p%d-twin" % n),
                          coeffs=[plane("coeffs", k, "rect") for k in range(3)],
                          result=lay.plane(1, TWORDS, np.uint32, footprint="rect", name="p%d-result" % n),
                          quant=[plane("quant", k, None) for k in range(3)],
                          out=lay.span(room, align=64, skew=(n + 1) % 4, footprint=("bytes", len(written)), name="p%d-bytes" % n),
                          encoded=lay.plane(1, NWORDS, np.uint32, footprint="rect", name="p%d-encoded" % n),
                          again=[plane("again", k, "rect") for k in range(3)],
                          result2=lay.plane(1, TWORDS, np.uint32, footprint="rect", name="p%d-result2" % n), written=written, room=room))
    block = G.GuardedBlock(ctx, lay, seed=12)
    try:
        first, enc, second, ll = [], [], [], []
        for r, s in zip(recs, specs):
            P = r["twin"]
            block[s["data"]].upload(as_row(r["transform"]))
            quant = [block[q].upload(v.astype(np.int16)) for q, v in zip(s["quant"], r["quant"])]
            shape = (P["depth"], P["horiz_cb"], P["vert_cb"], P["cb_mode"])
            first.append((block[s["data"]], len(r["transform"]), None, [block[c] for c in s["coeffs"]], None) + shape
                         + (P["is_intra"], P["compat"], block[s["result"]]))
            enc.append((quant, tables_of(ctx, r, quant)) + shape + (block[s["out"]], s["room"], block[s["encoded"]]))
            # SchroHipNoarithResult.bytes is the result's first word; the encoder's rules are those of a decoder in compat mode
            second.append((block[s["out"]], s["room"], block[s["encoded"]], [block[c] for c in s["again"]], None) + shape
                          + (P["is_intra"], 1, block[s["result2"]]))
            if P["is_intra"]:
                ll.append([sa.SubPlane(block[c], 0, 0, block[c].height >> P["depth"], block[c].width >> P["depth"], block[c].stride << P["depth"])
                           for c in s["coeffs"] + s["again"]])
        assert len(ll) == 1
        ctx.synchronize()
        assert ctx.noarith_decode_batch(first) is None
        ctx.dc_predict_batch(ll[0][:3])
        assert ctx.noarith_encode_batch(enc) is None
        assert ctx.noarith_decode_batch(second) is None
        ctx.dc_predict_batch(ll[0][3:])
        ctx.synchronize()
        expected = {}
        for r, s in zip(recs, specs):
            n, data = r["number"], s["written"]
            d = sa.noarith_decode_result(block[s["result"]].download())
            same_result(d, dict(CLEAN, bytes_read=len(r["transform"])), "picture %d, the twin" % n)
            e = sa.noarith_result(block[s["encoded"]].download())
            assert (e["bytes"], e["overrun"], e["false_zero"]) == (len(data), 0, (0, 0)), n
            d = sa.noarith_decode_result(block[s["result2"]].download())
            same_result(d, dict(CLEAN, bytes_read=len(data), compat_quant_offset=1), "picture %d, the encoder's bytes" % n)
            tail = block.before[s["out"].offset + len(data):s["out"].offset + s["room"]]
            expected[s["out"]] = np.concatenate([as_row(data)[0], tail]).reshape(1, -1)
            for k in range(3):
                expected[s["coeffs"][k]] = expected[s["again"][k]] = r["coeffs"][k]
        block.check(expected)
    finally:
        block.free()


# ---- from VLC bytes to pixels -----------------------------------------------------------------------------------------------

class Chain:
    """One picture with device buffers of its own, every output filled with a canary.  pic: motion (bytes or None), nbx, nby,
    num_refs, transform (bytes), shapes (rows, columns per component at the transform's size), dims (the picture's), dtype,
    depth, wavelet, hc, vc, mode, is_intra, compat, params (obmc_plane's).  refs: per reference the three device planes or
    half-pel images.  combine: the prediction alone from OBMC, the picture from the transform's last step."""

    def __init__(self, ctx, pic, refs, combine):
        self.ctx, self.pic, self.refs, self.combine = ctx, pic, refs, combine
        self.keep = []
        plane = lambda h, w, dtype, byte: self._own(ctx.plane(h, w, dtype).fill(byte))
        if pic["motion"] is not None:
            self.mdata = self._own(ctx.upload_bytes(as_row(pic["motion"])[0]))
            self.field = plane(1, pic["nbx"] * pic["nby"] * RECORD, np.uint8, 0xa5)
            self.mres = plane(1, MWORDS, np.uint32, 0xa5)
        self.tdata = self._own(ctx.upload_bytes(as_row(pic["transform"])[0]))
        self.coeffs = [plane(h, w, pic["dtype"], 0x5a) for h, w in pic["shapes"]]
        self.tres = plane(1, TWORDS, np.uint32, 0xa5)
        self.out = [plane(h, w, np.uint8, 0x11) for h, w in pic["dims"]]
        if not combine:
            self.res = [plane(h, w, pic["dtype"], 0x22) for h, w in pic["shapes"]]
        elif pic["motion"] is not None:
            self.pred = [plane(h, w, np.uint8, 0x33) for h, w in pic["dims"]]

    def _own(self, p):
        self.keep.append(p)
        return p

    def motion_entry(self):
        p = self.pic
        return (self.mdata, len(p["motion"]), None, p["nbx"], p["nby"], p["num_refs"], 0, self.field, self.mres)

    def transform_entry(self):
        p = self.pic
        return (self.tdata, len(p["transform"]), None, self.coeffs, None, p["depth"], p["hc"], p["vc"], p["mode"], p["is_intra"], p["compat"],
                self.tres)

    def obmc_jobs(self):
        """The prediction alone (combine) or the picture from the residual."""
        r1 = self.refs[0]
        r2 = self.refs[1] if len(self.refs) > 1 else None
        return [sa.obmc_plane(self.field, self.pic["params"], k, r1[k], r2[k] if r2 is not None else None, None if self.combine else self.res[k],
                              self.pred[k] if self.combine else self.out[k], prediction_only=1 if self.combine else 0) for k in range(3)]

    def transform(self):
        """The inverse wavelet: into the residual planes, or (combine) into the picture."""
        p = self.pic
        if p["is_intra"]:
            self.ctx.dc_predict_batch([c.level_view(p["depth"]) for c in self.coeffs])
        if not self.combine:
            pairs = list(zip(self.coeffs, self.res))
        else:
            pairs = [(c, o, self.pred[k] if p["motion"] is not None else None) for k, (c, o) in enumerate(zip(self.coeffs, self.out))]
        self.ctx.iiwt_batch(pairs, p["depth"], p["wavelet"])

    def enqueue(self):
        """Every launch of the picture, nothing waited for."""
        inter = self.pic["motion"] is not None
        if inter:
            assert self.ctx.motion_decode_batch([self.motion_entry()]) is None
            if self.combine:
                self.ctx.obmc_batch(self.obmc_jobs())
        assert self.ctx.noarith_decode_batch([self.transform_entry()]) is None
        self.transform()
        if inter and not self.combine:
            self.ctx.obmc_batch(self.obmc_jobs())
        elif not inter and not self.combine:
            self.ctx.convert_u8_batch(list(zip(self.res, self.out)))

    def check(self, what, field, coeffs, out):
        """field: (records, result dict) or None; coeffs: the planes the transform data decodes to, or None (not looked at);
        out: the picture."""
        if field is not None:
            same(self.field.download(), sa.motion_decode_result(self.mres.download()), field, what)
        d = sa.noarith_decode_result(self.tres.download())
        same_result(d, dict(CLEAN, bytes_read=len(self.pic["transform"])), what)
        got = [o.download() for o in self.out]
        for k in range(3):
            if coeffs is not None and not self.pic["is_intra"]:
                assert np.array_equal(self.coeffs[k].download(), coeffs[k]), (what, "coefficients", k)
            if not np.array_equal(got[k], out[k]):
                bad = np.argwhere(got[k] != out[k])
                raise AssertionError("%s component %d: %d of %d samples differ, first at (y, x) = %s: %d, expected %d"
                                     % (what, k, len(bad), got[k].size, tuple(bad[0]), got[k][tuple(bad[0])], out[k][tuple(bad[0])]))
        return got

    def free(self):
        for p in self.keep:
            p.free()


def stream_picture(rec):
    """A record of noarith_twin.pictures as Chain takes it."""
    P = rec["twin"]
    pic = dict(motion=rec.get("motion"), num_refs=rec["num_refs"], transform=rec["transform"], shapes=[P["iwt"][0], P["iwt"][1], P["iwt"][1]],
               dims=[o.shape for o in rec["out"]], dtype=np.dtype(np.int16), depth=P["depth"], wavelet=P["wavelet"], hc=P["horiz_cb"], vc=P["vert_cb"],
               mode=P["cb_mode"], is_intra=P["is_intra"], compat=P["compat"], params=rec.get("params"))
    if rec["num_refs"]:
        pic.update(nbx=P["nbx"], nby=P["nby"])
        assert rec["params"]["mv_precision"] == 0            # the references are the plain pictures
    return pic


def stream_field(rec):
    return MD.decode(rec["motion"], rec["twin"]["nbx"], rec["twin"]["nby"], rec["num_refs"], 0)


@pytest.mark.parametrize("order", ["residual", "combine"])
def test_first_pictures_from_vlc_bytes_to_pixels(ctx, order):
    """The first 12 pictures in coded order, each to planes of its own, the references the device's own earlier pictures;
    everything is enqueued, one wait at the end.  residual: OBMC adds the inverse wavelet's residual; combine: OBMC leaves
    the prediction and the transform's last step writes the picture."""
    md5 = json.load(open(os.path.join(S.GOLDEN, "stream_md5.json")))
    recs = twelve()
    chains, decoded = [], {}
    try:
        for rec in recs:
            chain = Chain(ctx, stream_picture(rec), [decoded[n] for n in rec["refs"]], order == "combine")
            chains.append(chain)
            decoded[rec["number"]] = chain.out
        ctx.synchronize()               # (the last wait in front of the twelve pictures)
        for chain in chains:
            chain.enqueue()
        ctx.synchronize()
        digests = {}
        for rec, chain in zip(recs, chains):
            n = rec["number"]
            got = chain.check("picture %d" % n, stream_field(rec) if rec["num_refs"] else None, None, rec["out"])
            digests[n] = S.D.frame_md5(got)
            assert digests[n] == md5["oracle"][n] == rec["md5"], n
        # what the reference's own decoder made of pictures 0, 1 and 2
        assert [digests[n] for n in (0, 1, 2)] == md5["reference"]
    finally:
        for chain in chains:
            chain.free()


# ---- what the stream lacks: drawn pictures ----------------------------------------------------------------------------------

DRAWN = {   # name: width, height, chroma format, chroma shifts, references, mv_precision, (xblen, xbsep), filter, depth, dtype, seed
    "420": (96, 64, 420, (1, 1), 2, 2, (12, 8), 0, 3, np.int16, 1),
    "422": (104, 72, 422, (1, 0), 2, 3, (12, 8), 5, 1, np.int16, 2),
    "444": (64, 48, 444, (0, 0), 1, 1, (8, 4), 4, 2, np.int16, 3),
    "s32": (80, 48, 420, (1, 1), 2, 1, (8, 4), 3, 2, np.int32, 4),
}
COUNTS = {1: [(2, 1), (3, 2)], 2: [(2, 2), (1, 2), (3, 3)], 3: [(1, 2), (2, 1), (3, 2), (4, 3)]}      # by depth; several in sub-band 0


def offsets_drawn(k, i, x, y):
    """-3 .. 3, as noarith_dec_cases.offsets_small"""
    return (x + 2 * y + i + k) % 7 - 3


def fill_small(case, rng):
    """Values of -3 .. 3, a third of them zero, some sub-bands and codeblocks zero: at the quant indices of `drawn` the
    residual is of the size of the prediction, so that the picture is not all clamped."""
    for p in case.planes:
        v = rng.integers(-3, 4, p.shape)
        p[...] = np.where(rng.random(p.shape) < 0.35, 0, v)
    for k in range(3):
        for i in range(case.nsub):
            hc, vc = case.counts(i)
            if (i + 2 * k) % 5 == 3:
                case.band(k, i)[...] = 0
            else:
                NE.get_codeblock(case.band(k, i), (i + k) % hc, k % vc, hc, vc)[...] = 0


@functools.lru_cache(maxsize=None)
def drawn(name):
    """(pic as Chain takes it less the references, the arguments of Ref, expected field, expected coefficients,
    render (reference UpComps) -> expected picture)."""
    w, h, fmt, chroma, num_refs, prec, (xblen, xbsep), filt, depth, dtype, seed = DRAWN[name]
    P = synth.motion_params(w, h, xblen, xbsep, prec, (1, 1, 1), chroma)
    nbx, nby = P["x_num_blocks"], P["y_num_blocks"]
    field = MC.draw(4000 + seed, nbx, nby, num_refs, 0, vmax=24 << prec)
    motion, encoded = ME.encode(field, nbx, nby, num_refs, 0)
    assert encoded["unverified"] == 0 and encoded["asserted"] == 0
    want_field = MD.decode(motion, nbx, nby, num_refs, 0)
    assert want_field[0].tobytes() == ME.canonical(field).tobytes()
    splits, modes = (field["flags"] >> 3) & 3, field["flags"] & 3
    assert set(splits.tolist()) == {0, 1, 2} and set(modes.tolist()) == ({0, 1, 2, 3} if num_refs > 1 else {0, 1})
    # quant planes, non-zero offsets (carried from codeblock to codeblock) and the writer as tests/noarith_dec_draws.py has them,
    # with header indices of 8 .. 13 so that no carried index leaves 0 .. 60 (clamped_quant stays 0)
    case = NC.Case("drawn-" + name, dtype, w, h, fmt, depth, COUNTS[depth], 1, fill_small, seed)
    case.qidx = [[8 + k + i % 4 for i in range(case.nsub)] for k in range(3)]
    data, used = ND.write_transform_data(case.planes, depth, case.hc, case.vc, 1, 0, case.qidx, offsets_drawn)
    assert len({int(q) for qis in used.values() for q in qis.ravel() if q >= 0}) > 8
    coeffs = [np.zeros((hh, ww), dtype) for ww, hh in case.sizes]
    result = ND.decode_transform_data(data, coeffs, None, depth, case.hc, case.vc, 1, 0, 0)
    assert case.counts(0) != (1, 1) and all(result[key] == value for key, value in CLEAN.items()) and result["bytes_read"] == len(data)
    assert max(int(np.abs(c).max()) for c in coeffs) < 1 << 15
    dims = [comp_size(w, h, k, chroma)[::-1] for k in range(3)]
    pic = dict(motion=motion, nbx=nbx, nby=nby, num_refs=num_refs, transform=data, shapes=[(hh, ww) for ww, hh in case.sizes], dims=dims,
               dtype=np.dtype(dtype), depth=depth, wavelet=filt, hc=case.hc, vc=case.vc, mode=1, is_intra=0, compat=0, params=P)
    residual = [O.inverse_iwt(c, depth, filt) for c in coeffs]

    def render(ups):
        op = O.MotionParams(**P)
        return [O.motion_render(want_field[0], op, k, ups[0][k], ups[1][k] if num_refs > 1 else None, residual[k], dims[k][1], dims[k][0])
                for k in range(3)]
    return pic, (w, h, chroma, True, False, 500 + 20 * seed), want_field, coeffs, render


class DrawnRun:
    """A drawn picture on a context: the references (uploaded and upsampled by upsample_batch on the context's stream when
    they are made), the chain, the expected picture."""

    def __init__(self, ctx, name):
        self.name = name
        pic, (w, h, chroma, up, pair, seed), self.field, self.coeffs, render = drawn(name)
        self.refs = [Ref(ctx, w, h, chroma, up, pair, seed + 7 * r) for r in range(pic["num_refs"])]
        self.chain = Chain(ctx, pic, [r.dev for r in self.refs], False)
        self.want = render([r.up for r in self.refs])

    def check(self, what=""):
        self.chain.check("the drawn picture %s%s" % (self.name, what), self.field, self.coeffs, self.want)

    def free(self):
        self.chain.free()
        for r in self.refs:
            r.free()


def run_drawn(ctx, names):
    runs = []
    try:
        for name in names:
            runs.append(DrawnRun(ctx, name))
        chains = [r.chain for r in runs]
        # one call per stage for the pictures of the pass, no wait between the stages (a transform call has one depth and filter)
        assert ctx.motion_decode_batch([c.motion_entry() for c in chains]) is None
        assert ctx.noarith_decode_batch([c.transform_entry() for c in chains]) is None
        for c in chains:
            c.transform()
        ctx.obmc_batch([job for c in chains for job in c.obmc_jobs()])
        ctx.synchronize()
        for r in runs:
            r.check()
    finally:
        for r in runs:
            r.free()


def test_drawn_pictures_from_vlc_bytes_to_pixels(ctx):
    """Three unlike s16 pictures in one pass -- 4:2:0, 4:2:2 and 4:4:4; two references and one; mv_precision 2, 3 and 1;
    blocks 12/8 and 8/4; filters 0, 5 and 4 at depths 3, 1 and 2; splits 0, 1 and 2 mixed, every mode, quant offsets,
    several codeblocks in every sub-band -- and one s32 picture alone (filter 3, depth 2)."""
    assert len({(DRAWN[n][2], DRAWN[n][5], DRAWN[n][7], DRAWN[n][8]) for n in ("420", "422", "444")}) == 3
    run_drawn(ctx, ["420", "422", "444"])
    run_drawn(ctx, ["s32"])


def scratch_words(chain):
    """(motion_decode_batch's, noarith_decode_batch's) words of queue scratch for the chain's picture."""
    t = _lib.load().schro_hip_noarith_decode_scratch_words(sa.noarith_decode_pictures([chain.transform_entry()]), 1, chain.pic["dtype"].itemsize)
    return sa.motion_decode_scratch_words([chain.motion_entry()]), int(t)


def test_scratch_shared_by_the_decode_stages():
    """On a context of its own, whose queue's one grow-only block starts empty: the small 4:4:4 drawn picture, stream
    picture 1, the small picture again, nothing waited for in between.  Both decode stages and the wavelet's LL images take
    the block; it has to grow -- the stream is waited for, the block freed -- between the small picture and the large one,
    and the third picture runs in the grown block."""
    recs = {r["number"]: r for r in T.pictures(limit=3)}
    assert sorted(recs) == [0, 1, 3] and recs[1]["refs"] == [0, 3]
    ctx = sa.Context(0)
    keep, runs, chain = [], [], None
    try:
        refs = [[ctx.upload(p) for p in recs[n]["out"]] for n in recs[1]["refs"]]
        keep = [p for r in refs for p in r]
        runs = [DrawnRun(ctx, "444"), DrawnRun(ctx, "444")]
        chain = Chain(ctx, stream_picture(recs[1]), refs, False)
        small, large = scratch_words(runs[0].chain), scratch_words(chain)
        assert 4 * small[0] <= large[0] and 4 * small[1] <= large[1]
        assert chain.pic["depth"] > 2 and runs[0].chain.pic["depth"] == 2           # levels 3 .. 1 against level 1 in the scratch
        ctx.synchronize()               # (the last wait in front of the three pictures)
        runs[0].chain.enqueue()
        chain.enqueue()
        runs[1].chain.enqueue()
        ctx.synchronize()
        runs[0].check(", first")
        got = chain.check("stream picture 1", stream_field(recs[1]), recs[1]["coeffs"], recs[1]["out"])
        assert S.D.frame_md5(got) == json.load(open(os.path.join(S.GOLDEN, "stream_md5.json")))["reference"][1]
        runs[1].check(", again")
    finally:
        for r in runs:
            r.free()
        if chain is not None:
            chain.free()
        for p in keep:
            p.free()
        ctx.close()
