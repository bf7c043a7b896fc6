"""GPU: schro_hip_arith_decode_batch -- arithmetic-coded transform data decoded on the device -- against the restatement
(tests/arith_dec_ref.py) and, on the reference's own stream, against oracle/dirac_stream.py and the reference decoder's
digests.  Every call's buffers lie in a guard_lib.GuardedBlock, so the write footprint is checked with the values."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import arith_dec_draws as AD
import arith_stream as AS
import guard_lib as G
import noarith_enc_ref as enc
import oracle_lib
import schroedinger_amd as sa
import stream_lib as S
from schroedinger_amd import _lib, frames
from test_gpu_noarith_decode import same_result
from test_gpu_noarith_twin import CLEAN, Chain, as_row, stream_picture

pytestmark = pytest.mark.gpu

WORDS = C.sizeof(_lib.ArithDecodeResult) // 4


def run_guarded(ctx, cases, skews, pad=0, with_quant=True, words=None):
    """The cases (one sample size) in ONE call, everything in one guarded block; raises on any difference.  words: per case
    None or the value of a bytes_on_device word of its own in the block, which must keep its value."""
    b = cases[0].dtype.itemsize
    lay, specs = G.Layout(), []
    words = [None] * len(cases) if words is None else words
    wanted = [case.expected(None if word is None else min(word, case.data_bytes)) for case, word in zip(cases, words)]
    for n, (case, skew) in enumerate(zip(cases, skews)):
        fp = "rect" if wanted[n][0] is not None else None           # a picture with the error: nothing may change
        tag = "p%d-%s-" % (n, case.name)
        data = lay.span(max(len(case.data), 1), align=64, skew=skew, footprint=None, name=tag + "data")
        plane = lambda what, k, w, h, shift: lay.plane(h, w, case.dtype, stride=(w * b + 63) // 64 * 64 + pad * b, skew=b * ((skew + k + shift) % 4),
                                                       footprint=fp, name="%s%s%d" % (tag, what, k))
        coeffs = [plane("coeffs", k, w, h, 0) for k, (w, h) in enumerate(case.sizes)]
        quant = [plane("quant", k, w, h, 2) for k, (w, h) in enumerate(case.sizes)] if with_quant else None
        res = lay.plane(1, WORDS, np.uint32, align=64, skew=4 * (skew % 4), footprint="rect", name=tag + "result")
        word = lay.plane(1, 1, np.uint32, align=64, skew=4 * ((skew + 1) % 4), footprint=None, name=tag + "length word") \
            if words[n] is not None else None
        specs.append((data, coeffs, quant, res, word))
    block = G.GuardedBlock(ctx, lay, seed=len(cases) + pad)
    try:
        pics, expected = [], {}
        for n, (case, (data, coeffs, quant, res, word)) in enumerate(zip(cases, specs)):
            if case.data:
                block[data].upload(as_row(case.data))
            if word is not None:
                block[word].upload(np.array([[words[n]]], np.uint32))
            pics.append((block[data], case.data_bytes, block[word] if word is not None else None, [block[s] for s in coeffs],
                         [block[s] for s in quant] if quant else None, case.depth, case.hc, case.vc, case.mode, case.is_intra, case.compat,
                         block[res]))
            if wanted[n][0] is not None:
                expected.update(zip(coeffs, wanted[n][0]))
                if quant:
                    expected.update(zip(quant, wanted[n][1]))
        assert ctx.arith_decode_batch(pics) is None
        ctx.synchronize()
        for n, (case, (data, coeffs, quant, res, word)) in enumerate(zip(cases, specs)):
            same_result(sa.arith_decode_result(block[res].download()), wanted[n][2], case.name)
        block.check(expected)
    finally:
        block.free()


# ---- the reference's stream ---------------------------------------------------------------------------------------------------

def twelve():
    recs = list(AS.pictures(limit=12))
    assert [r["number"] for r in recs] == AS.T.FIRST_TWELVE and recs[0]["twin"]["is_intra"]
    return recs


def test_first_twelve_stream_pictures_in_one_call(ctx):
    """The stream's own bytes at data skews 0 .. 3: the planes are the oracle's coefficients (picture 0 behind
    dc_predict_batch), the results clean, bytes_read the length, and bins what the restatement counts."""
    recs = twelve()
    lay, specs = G.Layout(), []
    for n, r in enumerate(recs):
        (h0, w0), (h1, w1) = r["twin"]["iwt"]
        shapes = [(h0, w0), (h1, w1), (h1, w1)]
        specs.append(dict(data=lay.span(len(r["arith"]), align=64, skew=n % 4, footprint=None, name="p%d-data" % n),
                          coeffs=[lay.plane(h, w, np.int16, stride=w * 2 + 64, footprint="rect", name="p%d-coeffs%d" % (n, k))
                                  for k, (h, w) in enumerate(shapes)],
                          quant=[lay.plane(h, w, np.int16, stride=w * 2 + 64, footprint="rect", name="p%d-quant%d" % (n, k))
                                 for k, (h, w) in enumerate(shapes)] if n % 2 == 0 else None,
                          result=lay.plane(1, WORDS, np.uint32, footprint="rect", name="p%d-result" % n)))
    block = G.GuardedBlock(ctx, lay, seed=24)
    try:
        pics, ll, expected = [], [], {}
        for r, s in zip(recs, specs):
            block[s["data"]].upload(as_row(r["arith"]))
            coeffs = [block[c] for c in s["coeffs"]]
            pics.append(AS.entry(r, block[s["data"]], len(r["arith"]), coeffs, [block[q] for q in s["quant"]] if s["quant"] else None,
                                 block[s["result"]]))
            if r["twin"]["is_intra"]:
                d = r["twin"]["depth"]
                ll += [sa.SubPlane(c, 0, 0, c.height >> d, c.width >> d, c.stride << d) for c in coeffs]
            expected.update(zip(s["coeffs"], r["coeffs"]))
            if s["quant"]:
                expected.update(zip(s["quant"], [q.astype(np.int16) for q in r["quant"]]))
        assert len(ll) == 3
        ctx.synchronize()
        assert ctx.arith_decode_batch(pics) is None
        ctx.dc_predict_batch(ll)
        ctx.synchronize()
        compat = 0
        for r, s in zip(recs, specs):
            assert r["twin"]["compat"] == compat
            d = sa.arith_decode_result(block[s["result"]].download())
            compat = d["compat_quant_offset"]
            same_result(d, dict(CLEAN, bytes_read=len(r["arith"])), "picture %d" % r["number"])
            shapes = [c.shape for c in r["coeffs"]]
            want = AD.Case("stream", np.int16, [(w, h) for h, w in shapes], r["twin"]["depth"], r["twin"]["horiz_cb"], r["twin"]["vert_cb"],
                           r["twin"]["cb_mode"], r["twin"]["compat"], r["twin"]["is_intra"], r["arith"]).expected()[2] if r["number"] < 2 else None
            if want is not None:
                same_result(d, want, "picture %d against the restatement" % r["number"])
        assert compat == 1              # picture 0 runs the compat test and turns the state on
        block.check(expected)
    finally:
        block.free()


class ArithChain(Chain):
    """test_gpu_noarith_twin.Chain with the stream's own transform data, decoded by arith_decode_batch, and the motion field
    uploaded from the oracle (its arithmetic decode is not on the device yet)."""

    def __init__(self, ctx, rec, refs):
        pic = dict(stream_picture(rec), transform=rec["arith"], motion=None)
        Chain.__init__(self, ctx, pic, refs, False)
        self.pic["motion"] = b"" if rec["num_refs"] else None            # (Chain.obmc_jobs / transform look at `is not None`)
        self.tres.free()
        self.keep.remove(self.tres)
        self.tres = self._own(ctx.plane(1, WORDS, np.uint32).fill(0xa5))
        if rec["num_refs"]:
            self.field = self._own(ctx.upload_bytes(np.frombuffer(rec["mv"].tobytes(), np.uint8)))

    def enqueue(self):
        assert self.ctx.arith_decode_batch([self.transform_entry()]) is None
        self.transform()
        if self.pic["motion"] is not None:
            self.ctx.obmc_batch(self.obmc_jobs())
        else:
            self.ctx.convert_u8_batch(list(zip(self.res, self.out)))


def test_stream_bytes_to_pixels(ctx):
    """Pictures 0, 1 and 2 with the pictures they reference (0, 3, 1, 2 in coded order): the transform data decoded on the
    device from the stream's bytes, inverse wavelet and OBMC enqueued behind it, one wait at the end; the digests are the
    reference decoder's own."""
    md5 = json.load(open(os.path.join(S.GOLDEN, "stream_md5.json")))
    recs = [r for r in AS.pictures(limit=4)]
    assert [r["number"] for r in recs] == [0, 3, 1, 2]
    chains, decoded = [], {}
    try:
        for rec in recs:
            chain = ArithChain(ctx, rec, [decoded[n] for n in rec["refs"]])
            chains.append(chain)
            decoded[rec["number"]] = chain.out
        ctx.synchronize()
        for chain in chains:
            chain.enqueue()
        ctx.synchronize()
        digests = {}
        for rec, chain in zip(recs, chains):
            d = sa.arith_decode_result(chain.tres.download())
            same_result(d, dict(CLEAN, bytes_read=len(rec["arith"])), "picture %d" % rec["number"])
            got = [o.download() for o in chain.out]
            for k in range(3):
                assert np.array_equal(got[k], rec["out"][k]), (rec["number"], k)
            digests[rec["number"]] = S.D.frame_md5(got)
        assert [digests[n] for n in (0, 1, 2)] == md5["reference"]
    finally:
        for chain in chains:
            chain.free()


# ---- drawn pictures, hostile payloads -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", AD.draws(), ids=lambda c: c.name)
def test_drawn_picture_is_the_restatement_bit_for_bit(ctx, case):
    n = AD.draws().index(case)
    run_guarded(ctx, [case], [n % 4], pad=n % 3, with_quant=n % 4 != 3)


@pytest.mark.parametrize("case", AD.hostile(), ids=lambda c: c.name)
def test_hostile_payloads_are_defined(ctx, case):
    n = AD.hostile().index(case)
    run_guarded(ctx, [case], [(n + 1) % 4], pad=(n + 1) % 3)


@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=["s16", "s32"])
def test_more_towers_than_a_wave_and_an_error_picture_at_both_ends(ctx, dtype):
    """Every drawn and hostile picture of the sample size in one call (s16: 15 unlike pictures, more than 150 towers; chains
    from one bin to 80 000), the picture with the error first and again last: it stays byte for byte untouched, its
    neighbours are unaffected."""
    middle = [c for c in AD.draws() + AD.hostile() if c.dtype == np.dtype(dtype) and not c.expected()[2]["error"]]
    if np.dtype(dtype) == np.int32:
        # the s16 draws' bytes on s32 planes: other pictures (the restatement is asked again for the wider type)
        middle += [AD.Case(c.name + "-as-s32", np.int32, c.sizes, c.depth, c.hc, c.vc, c.mode, c.compat, c.is_intra, c.data)
                   for c in AD.draws() if c.dtype == np.int16][:6]
    cases = [AD.error_picture(dtype)] + middle + [AD.error_picture(dtype)]
    assert len(middle) >= 8 and sum(3 * (4 if c.depth else 1) for c in cases) >= 96
    assert cases[0].expected()[0] is None and cases[-1].expected()[2]["error"] == 1
    run_guarded(ctx, cases, [n % 4 for n in range(len(cases))], pad=1)


def test_length_from_a_word_on_the_device(ctx):
    cases = [AD.draws()[5], AD.draws()[7], AD.hostile()[0]]
    run_guarded(ctx, cases, [3, 0, 1], words=[len(cases[0].data) + 9, len(cases[1].data) // 3, 40])


def test_queue_order_and_scratch_growth():
    """On a context of its own: arith_decode_batch -> dc_predict_batch -> iiwt_batch with nothing waited for, over a small,
    a much larger and a small intra picture, so that the queue's scratch has to grow between them; each length comes
    through bytes_on_device."""
    small = AD.drawn("small", np.int16, 32, 32, 444, 2, [1, 2, 2], [1, 1, 2], 1, 1, 1, 41)
    large = AD.drawn("large", np.int16, 64, 64, 444, 4, [1, 2, 2, 3, 4], [1, 1, 2, 2, 3], 1, 1, 1, 42)
    assert sa.arith_decode_scratch_words([host_entry(large)], 2) > sa.arith_decode_scratch_words([host_entry(small)], 2)
    ctx = sa.Context(0)
    keep = []
    try:
        runs = []
        for case in (small, large, small):
            own = lambda p: keep.append(p) or p
            data = own(ctx.upload_bytes(np.frombuffer(case.data + b"\x00" * 7, np.uint8)))
            word = own(ctx.upload(np.array([[len(case.data)]], np.uint32)))
            coeffs = [own(ctx.plane(h, w, np.int16).fill(0x5a)) for w, h in case.sizes]
            out = [own(ctx.plane(h, w, np.int16).fill(0x33)) for w, h in case.sizes]
            res = own(ctx.plane(1, WORDS, np.uint32).fill(0xa5))
            runs.append((case, data, word, coeffs, out, res))
        ctx.synchronize()
        for case, data, word, coeffs, out, res in runs:
            assert ctx.arith_decode_batch([(data, len(case.data) + 7, word, coeffs, None, case.depth, case.hc, case.vc, case.mode, 1, case.compat,
                                            res)]) is None
            ctx.dc_predict_batch([c.level_view(case.depth) for c in coeffs])
            ctx.iiwt_batch(list(zip(coeffs, out)), case.depth, 1)
        ctx.synchronize()
        for case, data, word, coeffs, out, res in runs:
            want_c, _, want_r = case.expected()
            same_result(sa.arith_decode_result(res.download()), want_r, case.name)
            for k in range(3):
                c = want_c[k].copy()
                ll = enc.subband(c, case.depth, 0)
                ll[...] = oracle_lib.dc_predict(ll)
                assert np.array_equal(coeffs[k].download(), c), (case.name, k)
                assert np.array_equal(out[k].download(), oracle_lib.inverse_iwt(c, case.depth, 1)), (case.name, k)
    finally:
        for p in keep:
            p.free()
        ctx.close()


class _Fake:
    """A plane that is only an address: the host-only calls dereference nothing."""

    def __init__(self, ptr, w, h, b):
        self.ptr, self.width, self.height, self.stride = ptr, w, h, w * b


def host_entry(case):
    planes = [_Fake((k + 1) << 24, w, h, case.dtype.itemsize) for k, (w, h) in enumerate(case.sizes)]
    return (1 << 30, len(case.data), None, planes, None, case.depth, case.hc, case.vc, case.mode, case.is_intra, case.compat, 1 << 31)


# ---- the frame layer ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("number", [0, 3])
def test_frame_layer_on_stream_pictures(ctx, number):
    """schro_hipframe_decode_transform_data_arith on a 4:2:0 device frame: the frame as schro_hipframe_dequantise leaves it
    (the intra picture's LL bands DC-predicted), the result, the compat state; params->is_noarith is refused."""
    rec = {r["number"]: r for r in AS.pictures(limit=2)}[number]
    P = rec["twin"]
    (h0, w0), (h1, w1) = P["iwt"]
    # a 4:2:0 frame whose chroma holds the chroma transform (120 rows round up to 128): the luma has rows to spare
    fh = max(h0, 2 * h1)
    start = [np.full(s, 0x1234, np.int16) for s in ((fh, w0), (h1, w1), (h1, w1))]
    frame = frames.DeviceFrame(ctx, frames.frame_format(np.dtype(np.int16), 1, 1), w0, fh).upload(frames.HostFrame(start, 1, 1))
    params = frames.make_params(transform_depth=P["depth"], num_refs=rec["num_refs"], is_noarith=0, iwt_luma_width=w0, iwt_luma_height=h0,
                                iwt_chroma_width=w1, iwt_chroma_height=h1, codeblock_mode_index=P["cb_mode"])
    for l in range(P["depth"] + 1):
        params.horiz_codeblocks[l], params.vert_codeblocks[l] = P["horiz_cb"][l], P["vert_cb"][l]
    try:
        result, compat, status = ctx.decode_transform_data_arith(frame, rec["arith"], params, P["compat"])
        assert status == 0 and compat == 1
        same_result(result, dict(CLEAN, bytes_read=len(rec["arith"]), compat_quant_offset=1), "picture %d" % number)
        assert result["bins"] > 8 * len(rec["arith"]) // 2
        for k, (got, exp) in enumerate(zip(frame.download(), rec["coeffs"])):
            assert np.array_equal(got[:exp.shape[0]], exp) and (got[exp.shape[0]:] == 0x1234).all(), (number, k)
        params.is_noarith = 1
        with pytest.raises(sa.SchroHipError):
            ctx.decode_transform_data_arith(frame, rec["arith"], params, 0)
        for k, (got, exp) in enumerate(zip(frame.download(), rec["coeffs"])):
            assert np.array_equal(got[:exp.shape[0]], exp), (number, k, "the refused call wrote")
    finally:
        frame.unref()
