"""GPU: core-syntax transform data in the VLC parse codes read on the device (schro_hip_noarith_decode_batch, the frame
layer's schro_hipframe_decode_transform_data_noarith) against tests/noarith_dec_ref.py, the restatement of
schro_decoder_parse_transform_data + schro_decoder_decode_transform_data for is_noarith over oracle_lib.dequant_codeblock:
bit for bit -- the coefficient planes, the quant planes, the whole result block -- with every plane, the input and the
result between guard blocks at four alignments each (the planes 0 .. 3 samples past a 256-byte line, the input at four
byte alignments, the result at four word alignments), so that row padding and everything outside the samples must keep its
canary.  The pictures, the limits they straddle and the hostile streams are tests/noarith_dec_cases.py's; the hostile
ones are defined inputs with expected outputs like the others."""
import ctypes as C

import numpy as np
import pytest

import guard_lib as G
import noarith_dec_cases as DC
import noarith_enc_cases as NC
import noarith_enc_ref as enc
import oracle_lib
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

pytestmark = pytest.mark.gpu

WORDS = C.sizeof(_lib.NoarithDecodeResult) // 4


def same_result(got, want, what):
    for key, value in want.items():
        assert np.array_equal(np.asarray(got[key]), np.asarray(value)), (what, key, got[key], value)


def expected_with_word(case, word):
    """What the case must leave when the call takes its length from a word on the device: the restatement on the first
    min(word, data_bytes) bytes."""
    if word is None:
        return case.expected()
    return DC.Case(case.name, case.dtype, case.sizes, case.depth, case.hc, case.vc, case.mode, case.compat, case.is_intra, case.data,
                   min(word, case.data_bytes)).expected()


def run_guarded(ctx, cases, skews, pad=0, with_quant=True, words=None):
    """The cases (one sample size) in ONE call, everything in one guarded block; returns nothing, raises on any difference.
    words: per case None or the value of a bytes_on_device word of its own in the block, which must keep its value."""
    b = cases[0].dtype.itemsize
    lay = G.Layout()
    specs = []
    words = [None] * len(cases) if words is None else words
    wanted = [expected_with_word(case, word) for case, word in zip(cases, words)]
    for n, (case, skew) in enumerate(zip(cases, skews)):
        coeffs_e, quant_e, result_e = wanted[n]
        fp = "rect" if coeffs_e is not None else None           # a picture with the error: nothing may change
        tag = "p%d-" % n
        data = lay.span(max(len(case.data), 1), align=64, skew=skew, footprint=None, name=tag + "data")
        # planes that are only sample-aligned, as the call accepts them: the lead is 0 .. 3 samples past a 256-byte line, the
        # components of a picture and its two kinds of planes taking unlike ones; the result at four word alignments
        coeffs = [lay.plane(h, w, case.dtype, stride=(w * b + 63) // 64 * 64 + pad * b, skew=b * ((skew + k) % 4), footprint=fp,
                            name="%scoeffs%d" % (tag, k)) for k, (w, h) in enumerate(case.sizes)]
        quant = [lay.plane(h, w, case.dtype, stride=(w * b + 63) // 64 * 64 + pad * b, skew=b * ((skew + k + 2) % 4), footprint=fp,
                           name="%squant%d" % (tag, k)) for k, (w, h) in enumerate(case.sizes)] if with_quant else None
        res = lay.plane(1, WORDS, np.uint32, align=64, skew=4 * (skew % 4), footprint="rect", name=tag + "result")
        word = lay.plane(1, 1, np.uint32, align=64, skew=4 * ((skew + 1) % 4), footprint=None, name=tag + "length word") \
            if words[n] is not None else None
        specs.append((data, coeffs, quant, res, word))
    block = G.GuardedBlock(ctx, lay, seed=len(cases) + pad)
    try:
        pics, expected = [], {}
        for n, (case, (data, coeffs, quant, res, word)) in enumerate(zip(cases, specs)):
            if case.data:
                block[data].upload(np.frombuffer(case.data, np.uint8).reshape(1, -1))
            if word is not None:
                block[word].upload(np.array([[words[n]]], np.uint32))
            pics.append((block[data], case.data_bytes, block[word] if word is not None else None, [block[s] for s in coeffs],
                         [block[s] for s in quant] if quant else None, case.depth, case.hc, case.vc, case.mode, case.is_intra, case.compat,
                         block[res]))
            coeffs_e, quant_e, result_e = wanted[n]
            if coeffs_e is not None:
                expected.update(zip(coeffs, coeffs_e))
                if quant:
                    expected.update(zip(quant, quant_e))
        assert ctx.noarith_decode_batch(pics) is None
        ctx.synchronize()
        for n, (case, (data, coeffs, quant, res, word)) in enumerate(zip(cases, specs)):
            same_result(sa.noarith_decode_result(block[res].download()), wanted[n][2], case.name)
        block.check(expected)
    finally:
        block.free()


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_batch_is_the_reference_bit_for_bit(ctx, case):
    n = DC.CASES.index(case)
    run_guarded(ctx, [case], [n % 4], pad=n % 3)


@pytest.mark.parametrize("case", DC.HOSTILE, ids=lambda c: c.name)
def test_hostile_streams_are_defined(ctx, case):
    n = DC.HOSTILE.index(case)
    run_guarded(ctx, [case], [(n + 1) % 4], pad=(n + 1) % 3)


@pytest.mark.parametrize("bpp", [2, 4])
def test_three_unlike_pictures_in_one_call(ctx, bpp):
    cases = [DC.BY_NAME[n] for n in DC.MIXED[bpp]]
    assert len({(tuple(c.sizes), c.depth) for c in cases}) == 3
    run_guarded(ctx, cases, [1, 2, 3], pad=1)


@pytest.mark.parametrize("bpp", [2, 4])
def test_an_error_picture_leaves_its_neighbours_alone(ctx, bpp):
    t = "s16" if bpp == 2 else "s32"
    cases = [DC.BY_NAME[t + "-all-two-m1-c0"], DC.BY_NAME[t + "-index-61-middle"], DC.BY_NAME[t + "-random-payloads-2"]]
    assert [c.expected()[2]["error"] for c in cases] == [0, 1, 0]
    run_guarded(ctx, cases, [0, 3, 2])


@pytest.mark.parametrize("name", ["s16-all-three-m1-c0", "s32-heads-127"])
def test_without_quant_planes(ctx, name):
    run_guarded(ctx, [DC.BY_NAME[name]], [2], with_quant=False)


@pytest.mark.parametrize("name", ["s16-all-two-m1-c0", "s16-all-two-m1-c1", "s32-all-mixed-m0-c1", "s32-all-three-m1-c0"])
def test_frame_layer(ctx, name):
    """schro_hipframe_decode_transform_data_noarith on a 4:2:0 device frame: the frame as schro_hipframe_dequantise leaves
    it -- the LL bands of an intra picture DC-predicted --, the result and the compat state."""
    case = DC.BY_NAME[name]
    coeffs_e, quant_e, result_e = case.expected()
    (w, h) = case.sizes[0]
    assert case.sizes[1] == ((w + 1) // 2, (h + 1) // 2)
    want = [c.copy() for c in coeffs_e]
    if case.is_intra:
        for p in want:
            ll = enc.subband(p, case.depth, 0)
            ll[...] = oracle_lib.dc_predict(ll)
    start = [np.full((hh, ww), 0x1234, case.dtype) for ww, hh in case.sizes]
    frame = frames.DeviceFrame(ctx, frames.frame_format(case.dtype, 1, 1), w, h).upload(frames.HostFrame(start, 1, 1))
    params = frames.make_params(transform_depth=case.depth, num_refs=0 if case.is_intra else 1, is_noarith=1, iwt_luma_width=w,
                                iwt_luma_height=h, iwt_chroma_width=case.sizes[1][0], iwt_chroma_height=case.sizes[1][1],
                                codeblock_mode_index=case.mode)
    for l in range(case.depth + 1):
        params.horiz_codeblocks[l], params.vert_codeblocks[l] = case.hc[l], case.vc[l]
    try:
        result, compat, status = ctx.decode_transform_data_noarith(frame, case.data, params, case.compat)
        assert status == 0 and compat == result_e["compat_quant_offset"]
        same_result(result, result_e, name)
        for k, (got, exp) in enumerate(zip(frame.download(), want)):
            assert np.array_equal(got, exp), (name, k)
        # picture->error: the status, the result all the same, the frame and the state untouched
        bad = DC.BY_NAME[("s16" if case.dtype.itemsize == 2 else "s32") + "-index-61-middle"]
        assert (bad.sizes, bad.depth) == (case.sizes, case.depth)
        for l in range(bad.depth + 1):
            params.horiz_codeblocks[l], params.vert_codeblocks[l] = bad.hc[l], bad.vc[l]
        params.codeblock_mode_index = bad.mode
        result, compat, status = ctx.decode_transform_data_noarith(frame, bad.data, params, 1)
        assert status == -1 and compat == 1 and result["error"] == 1
        same_result(result, dict(bad.expected()[2], compat_quant_offset=1), bad.name)
        for k, (got, exp) in enumerate(zip(frame.download(), want)):
            assert np.array_equal(got, exp), (bad.name, k)
    finally:
        frame.unref()


def test_refusal_through_the_context(ctx):
    """`data` inside a coefficient plane is refused, the message naming picture and component, and nothing is enqueued."""
    case = DC.BY_NAME["s16-all-two-m1-c0"]
    coeffs = [ctx.plane(h, w, case.dtype).fill(0xa5) for w, h in case.sizes]
    res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)
    try:
        with pytest.raises(sa.SchroHipError, match="picture 0: data overlaps coeffs\\[1\\]") as e:
            ctx.noarith_decode_batch([(coeffs[1].ptr + 8, 64, None, coeffs, None, case.depth, case.hc, case.vc, case.mode, 0, 0, res)])
        assert e.value.code == -1
        ctx.synchronize()
        assert all((p.download().view(np.uint8) == 0xa5).all() for p in coeffs) and (res.download() == 0xa5a5a5a5).all()
    finally:
        for p in coeffs + [res]:
            p.free()


def test_own_buffers_return_the_result(ctx):
    """The short form of Context.noarith_decode_batch: host bytes in, result dicts out."""
    case = DC.BY_NAME["s32-compat-fires-c1"]
    coeffs = [ctx.plane(h, w, case.dtype) for w, h in case.sizes]
    try:
        (result,) = ctx.noarith_decode_batch([(case.data, coeffs, None, case.depth, case.hc, case.vc, case.mode, case.is_intra, case.compat)])
        same_result(result, case.expected()[2], case.name)
        for p, exp in zip(coeffs, case.expected()[0]):
            assert np.array_equal(p.download(), exp)
    finally:
        for p in coeffs:
            p.free()


def chain_round_trip(ctx, dtype, pics, seed=77):
    """quantise_batch -> noarith_encode_batch -> noarith_decode_batch on one queue, nothing waited for in between, for
    pics [(sizes, depth, hc, vc, mode)] where the encoder's and the decoder's rules agree (one codeblock in sub-band 0,
    compat on): the decoder's quant planes are the quantiser's, its coefficient planes the reconstruction the quantiser
    left, and it read the bytes the encoder reported."""
    dtype = np.dtype(dtype)
    b = dtype.itemsize
    rng = np.random.default_rng(seed)
    assert all((hc[0], vc[0]) == (1, 1) for _, _, hc, vc, _ in pics)
    held, enc_pics, dec_pics, jobs = [], [], [], []
    words = C.sizeof(_lib.NoarithResult) // 4
    for sizes, depth, hc, vc, mode in pics:
        src, quant, tabs, dq, dc = [], [], [], [], []
        for k, (w, h) in enumerate(sizes):
            c = ctx.upload(rng.integers(-700, 701, (h, w)).astype(dtype))
            q = ctx.plane(h, w, dtype, stride=c.stride).fill(0x11)
            tab = ctx.codeblock_layout(w, h, depth, hc, vc, c.stride, b)
            n = 0
            for i in range(1 + 3 * depth):
                nh, nv = enc.codeblock_counts(i, hc, vc)
                for _ in range(nh * nv):
                    tab[n].quant_index = (5 + 7 * k + 3 * i) % 40
                    n += 1
            src.append(c), quant.append(q), tabs.append(tab)
            dq.append(ctx.plane(h, w, dtype, stride=c.stride).fill(0x22)), dc.append(ctx.plane(h, w, dtype, stride=c.stride).fill(0x33))
            # (the plane-layer quantiser takes no record without samples -- a tiny sub-band cut into more codeblocks than it has
            # columns or rows --; the encoder takes the whole table)
            jobs.append((c, q, [(t.dst_offset, t.dst_stride, t.width, t.height, t.src_offset, t.src_bytes, t.quant_index)
                                for t in tab if t.width and t.height], 0))
        cap = sa.noarith_encode_bound(sizes, depth, hc, vc, b)
        out = ctx.plane(1, cap, np.uint8)
        eres = ctx.plane(1, words, np.uint32)
        dres = ctx.plane(1, WORDS, np.uint32)
        enc_pics.append((quant, tabs, depth, hc, vc, mode, out, cap, eres))
        # SchroHipNoarithResult.bytes is the result's first word
        dec_pics.append((out, cap, eres, dc, dq, depth, hc, vc, mode, 0, 1, dres))
        held.append((src, quant, dq, dc, out, eres, dres))
    try:
        summaries = ctx.quantise_batch(jobs)
        assert ctx.noarith_encode_batch(enc_pics) is None
        assert ctx.noarith_decode_batch(dec_pics) is None
        ctx.synchronize()
        for s in summaries:
            s.free()
        for n, (src, quant, dq, dc, out, eres, dres) in enumerate(held):
            e = sa.noarith_result(eres.download())
            d = sa.noarith_decode_result(dres.download())
            assert e["overrun"] == 0 and e["false_zero"] == (0, 0)
            assert d["error"] == 0 and d["bytes_read"] == e["bytes"] and d["compat_quant_offset"] == 1
            assert (d["truncated"], d["not_consumed"], d["overran"], d["long_codes"], d["clamped_quant"]) == (0, 0, 0, 0, 0)
            for k in range(3):
                assert np.array_equal(dq[k].download(), quant[k].download()), (n, k)
                assert np.array_equal(dc[k].download(), src[k].download()), (n, k)
    finally:
        for group in held:
            for item in group:
                for p in (item if isinstance(item, list) else [item]):
                    p.free()


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_chain_quantise_encode_decode_without_a_host_wait(ctx, dtype):
    """quantise_batch -> noarith_encode_batch -> noarith_decode_batch on one queue, nothing waited for in between: the
    decoder takes its length from the encoder's result word on the device.  Its quant planes are the quantiser's and its
    coefficient planes the reconstruction the quantiser left.  Two unlike pictures of geometries where the encoder's and
    the decoder's rules agree (one codeblock in sub-band 0, compat on)."""
    chain_round_trip(ctx, dtype, [(NC.iwt_sizes(32, 16, 420, 2), 2, [1, 2, 3], [1, 2, 2], 1), (NC.iwt_sizes(48, 24, 444, 1), 1, [1, 3], [1, 2], 0)])
