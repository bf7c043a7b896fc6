"""GPU: core-syntax transform data in the VLC parse codes written on the device (schro_hip_noarith_encode_batch, the frame
layer's schro_hip_encode_transform_data_noarith) against tests/noarith_enc_ref.py, the literal restatement of
schro_encoder_encode_transform_data for is_noarith: byte for byte, with the reported size, actual_subband_bits and the
false_zero counts.  The pictures, the limits they straddle and the refusals are tests/noarith_enc_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import guard_lib as G
import noarith_enc_cases as NC
import noarith_enc_draws as ND
import noarith_enc_ref as ref
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

pytestmark = pytest.mark.gpu


def tables_of(ctx, case, strides):
    """Per component schro_hip_codeblock_layout's records for the plane's stride, the case's quant indices filled in."""
    tabs = []
    for k, (w, h) in enumerate(case.sizes):
        tab = ctx.codeblock_layout(w, h, case.depth, case.hc, case.vc, strides[k], case.dtype.itemsize)
        for t, q in zip(tab, case.record_indices(k)):
            t.quant_index = q
        assert len(tab) == case.ncodeblocks()
        tabs.append(tab)
    return tabs


def picture_of(ctx, case, pad=0):
    """(planes, tables, depth, hc, vc, mode) of a case: its quant planes uploaded (rows `pad` samples longer than the
    default pitch), what Context.noarith_encode_batch takes."""
    b = case.dtype.itemsize
    planes = [ctx.upload(p, stride=((p.shape[1] * b + 63) // 64 * 64) + pad * b) for p in case.planes]
    return (planes, tables_of(ctx, case, [p.stride for p in planes]), case.depth, case.hc, case.vc, case.mode)


def free(pic):
    for p in pic[0]:
        p.free()


def same(got, result, case, what):
    data, bits, stats = case.expected()
    assert result["bytes"] == len(data), (what, result["bytes"], len(data))
    assert result["overrun"] == 0, what
    if bytes(got) != data:
        n = next(i for i, (a, b) in enumerate(zip(bytes(got), data)) if a != b)
        raise AssertionError("%s: byte %d of %d is %02x, the reference writes %02x" % (what, n, len(data), got[n], data[n]))
    assert np.array_equal(result["subband_bits"], bits), (what, result["subband_bits"], bits)          # trap (b)
    assert result["false_zero"] == (stats["false_zero_codeblocks"], stats["false_zero_subbands"]), what  # trap (a)


@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c.name)
def test_batch_is_the_reference_byte_for_byte(ctx, case):
    pic = picture_of(ctx, case, pad=3 if "d2" in case.name else 0)
    try:
        (got, result), = ctx.noarith_encode_batch([pic])
        same(got, result, case, case.name)
    finally:
        free(pic)


def test_all_zero_pictures_are_one_byte_per_subband(ctx):
    for name in ("s16-zero-d2", "s32-zero-d6"):
        case = NC.BY_NAME[name]
        pic = picture_of(ctx, case)
        try:
            (got, result), = ctx.noarith_encode_batch([pic])
            assert bytes(got) == b"\x80" * (3 * case.nsub) and len(got) <= 57
            assert not result["subband_bits"].any() and result["false_zero"] == (0, 0)
        finally:
            free(pic)


def test_the_s16_zero_test_is_the_references(ctx):
    """Trap (a) in both directions, and what false_zero reports."""
    for name, want in (("s16-trap-codeblock", (1, 0)), ("s16-trap-subband", (0, 1))):
        case = NC.BY_NAME[name]
        pic = picture_of(ctx, case)
        try:
            (got, result), = ctx.noarith_encode_batch([pic])
            same(got, result, case, name)
            assert result["false_zero"] == want, name
        finally:
            free(pic)
    # trap (b): the sub-band called zero reports no bits, its written neighbour header and payload
    assert result["subband_bits"][0, 2] == 0 and result["subband_bits"][0, 1] >= 24


@pytest.mark.parametrize("bpp", [2, 4])
def test_three_unlike_pictures_in_one_call(ctx, bpp):
    cases = [NC.BY_NAME[n] for n in NC.MIXED[bpp]]
    assert len({(tuple(c.sizes), c.depth) for c in cases}) == 3
    pics = [picture_of(ctx, c) for c in cases]
    try:
        for (got, result), case in zip(ctx.noarith_encode_batch(pics), cases):
            same(got, result, case, case.name)
    finally:
        for p in pics:
            free(p)


@pytest.mark.parametrize("bpp", [2, 4])
def test_random_geometries(ctx, bpp):
    """Every draw of tests/noarith_enc_draws.py of one sample size in one call."""
    cases = [c for c in ND.DRAWS if c.dtype.itemsize == bpp]
    assert len(cases) >= 8
    pics = [picture_of(ctx, c, pad=n % 3) for n, c in enumerate(cases)]
    try:
        for (got, result), case in zip(ctx.noarith_encode_batch(pics), cases):
            same(got, result, case, case.name)
            assert result["false_zero"] == (0, 0)
    finally:
        for p in pics:
            free(p)


@pytest.mark.parametrize("bpp", [2, 4])
def test_deep_random_geometries(ctx, bpp):
    """The draws of depths 4, 5 and 6 of one sample size in one call: 57 sub-bands per picture at depth 6."""
    cases = [c for c in ND.DEEP_DRAWS if c.dtype.itemsize == bpp]
    assert sorted({c.depth for c in cases}) == [4, 5, 6] and {c.mode for c in cases} == {0, 1}
    pics = [picture_of(ctx, c, pad=n % 3) for n, c in enumerate(cases)]
    try:
        for (got, result), case in zip(ctx.noarith_encode_batch(pics), cases):
            same(got, result, case, case.name)
            assert result["false_zero"] == (0, 0)
    finally:
        for p in pics:
            free(p)


@pytest.mark.parametrize("name,short,skew", [("s16-32x16-d3-mixed-m1", 0, 1), ("s16-32x16-d3-mixed-m1", 1, 3),
                                             ("s32-extremes-d1", 0, 2), ("s32-extremes-d1", 1, 0), ("s16-window-65", 1, 1)])
def test_capacity_exact_and_one_byte_short(ctx, name, short, skew):
    """The output sits between guard blocks at every byte alignment.  Exact capacity: the bytes, no over-run.  One byte
    short: the first capacity bytes, the needed size and the over-run flag all the same.  Neither the bytes behind the
    reported size nor those behind the capacity are touched; the quant planes are left alone."""
    case = NC.BY_NAME[name]
    data, bits, stats = case.expected()
    b = case.dtype.itemsize
    words = C.sizeof(_lib.NoarithResult) // 4
    for room in ((len(data) - 1,) if short else (len(data), len(data) + 37)):
        lay = G.Layout()
        specs = [lay.plane(h, w, case.dtype, stride=(w * b + 63) // 64 * 64, footprint=None, name="quant%d" % k)
                 for k, (w, h) in enumerate(case.sizes)]
        out = lay.span(room, align=64, skew=skew, footprint=("bytes", min(room, len(data))), name="out")
        res = lay.plane(1, words, np.uint32, footprint="rect", name="result")
        block = G.GuardedBlock(ctx, lay, seed=room)
        try:
            planes = [block[s].upload(p) for s, p in zip(specs, case.planes)]
            tabs = tables_of(ctx, case, [p.stride for p in planes])
            assert ctx.noarith_encode_batch([(planes, tabs, case.depth, case.hc, case.vc, case.mode, block[out], room, block[res])]) is None
            ctx.synchronize()
            result = sa.noarith_result(block[res].download())
            assert result["bytes"] == len(data) and result["overrun"] == short
            assert np.array_equal(result["subband_bits"], bits)
            tail = block.before[out.offset + min(room, len(data)):out.offset + room]      # (the canary behind the bytes)
            block.check({out: np.concatenate([np.frombuffer(data[:room], np.uint8), tail]).reshape(1, -1)})
        finally:
            block.free()


@pytest.mark.parametrize("name", ["s16-16x8-d2-three-m1", "s32-16x8-d2-two-m0", "s16-32x16-d3-two-m0", "s32-32x16-d1-three-m1"])
def test_frame_layer(ctx, name):
    """schro_hip_encode_transform_data_noarith on a 4:2:0 device frame: the same bytes in the host buffer, the size, the
    sub-band bits; with a buffer one byte short, the status that says so and the first bytes."""
    case = NC.BY_NAME[name]
    data, bits, stats = case.expected()
    (w, h) = case.sizes[0]
    assert case.sizes[1] == ((w + 1) // 2, (h + 1) // 2)
    frame = frames.DeviceFrame(ctx, frames.frame_format(case.dtype, 1, 1), w, h).upload(frames.HostFrame(case.planes, 1, 1))
    params = frames.make_params(transform_depth=case.depth, num_refs=1, is_noarith=1, iwt_luma_width=w, iwt_luma_height=h,
                                iwt_chroma_width=case.sizes[1][0], iwt_chroma_height=case.sizes[1][1],
                                codeblock_mode_index=case.mode)
    for l in range(case.depth + 1):
        params.horiz_codeblocks[l], params.vert_codeblocks[l] = case.hc[l], case.vc[l]
    idx = [case.record_indices(k) for k in range(3)]
    try:
        bound = sa.noarith_encode_bound(case.sizes, case.depth, case.hc, case.vc, case.dtype.itemsize)
        assert bound >= len(data)
        got, nbytes, got_bits, fz, status = ctx.encode_transform_data_noarith(frame, params, idx, bound)
        assert status == 0 and nbytes == len(data) and bytes(got) == data
        assert np.array_equal(got_bits, bits) and fz == (stats["false_zero_codeblocks"], stats["false_zero_subbands"])
        got, nbytes, got_bits, fz, status = ctx.encode_transform_data_noarith(frame, params, idx, len(data) - 1)
        assert status == -3 and nbytes == len(data) and bytes(got) == data[:-1]
        assert b"takes %d bytes" % len(data) in ctx.lib.schro_hip_last_error()
    finally:
        frame.unref()


def test_refusal_through_the_context(ctx):
    """Trap (c): unlike quant indices in one sub-band are refused, the message naming picture, component and sub-band, and
    nothing is enqueued -- the output keeps its canary."""
    case = NC.BY_NAME["s16-32x16-d1-three-m1"]
    planes, tabs, depth, hc, vc, mode = pic = picture_of(ctx, case)
    out = ctx.plane(1, 4096, np.uint8).fill(0xa5)
    res = ctx.plane(1, C.sizeof(_lib.NoarithResult) // 4, np.uint32).fill(0xa5)
    try:
        tabs[2][14].quant_index ^= 1    # component 2, sub-band 2 (records 12 .. 17), its third record
        with pytest.raises(sa.SchroHipError, match="picture 0, component 2, sub-band 2: record 14 has quant index") as e:
            ctx.noarith_encode_batch([(planes, tabs, depth, hc, vc, mode, out, 4096, res)])
        assert e.value.code == -1
        ctx.synchronize()
        assert (out.download() == 0xa5).all() and (res.download() == 0xa5a5a5a5).all()
    finally:
        free(pic)
        out.free()
        res.free()


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_chain_quantise_encode_decode_dequantise(ctx, dtype):
    """quantise_batch -> noarith_encode_batch (the quant planes stay on the device) -> download -> the restated decoder ->
    dequant_batch with the decoder's arithmetic (the 16-bit Orc program on s16): the result is the reconstruction
    quantise_batch left in the coefficient planes."""
    dtype = np.dtype(dtype)
    b = dtype.itemsize
    depth, hc, vc, mode = 1, [2, 2], [2, 2], 1
    sizes = NC.iwt_sizes(32, 16, 420, depth)
    rng = np.random.default_rng(31)
    qidx = [[int(rng.integers(0, 28)) for _ in range(1 + 3 * depth)] for _ in range(3)]
    coeffs, quants, tabs, jobs = [], [], [], []
    for k, (w, h) in enumerate(sizes):
        c = ctx.upload(rng.integers(-700, 701, (h, w)).astype(dtype))
        q = ctx.plane(h, w, dtype, stride=c.stride).fill(0x11)
        tab = ctx.codeblock_layout(w, h, depth, hc, vc, c.stride, b)
        for n, t in enumerate(tab):
            t.quant_index = qidx[k][n // 4]
            assert t.width > 0 and t.height > 0
        coeffs.append(c), quants.append(q), tabs.append(tab)
        jobs.append((c, q, tab, 0))
    out = res = None
    try:
        summaries = ctx.quantise_batch(jobs)
        (data, result), = ctx.noarith_encode_batch([(quants, tabs, depth, hc, vc, mode)])
        assert result["overrun"] == 0 and result["false_zero"] == (0, 0)
        for s in summaries:
            s.free()
        got_q, indices, used = ref.decode_transform_data(bytes(data), [(h, w) for w, h in sizes], dtype, depth, hc, vc, mode)
        assert used == len(data) == result["bytes"]
        for k, (w, h) in enumerate(sizes):
            assert np.array_equal(got_q[k], quants[k].download()), k
            # the hand-over of a host decoder: every codeblock's values row-major and tight, its quant index from the stream
            recs, blob = [], []
            for n, t in enumerate(tabs[k]):
                i = n // 4
                x, y = (n % 4) % 2, (n % 4) // 2
                qi = int(indices[k][i][y, x]) if indices[k][i] is not None else 0
                cb = ref.get_codeblock(ref.subband(got_q[k], depth, i), x, y, 2, 2)
                assert cb.shape == (t.height, t.width)
                zero = indices[k][i] is None
                recs.append((t.dst_offset, t.dst_stride, t.width, t.height, -1 if zero else sum(len(v) for v in blob), b, qi))
                if not zero:
                    blob.append(np.ascontiguousarray(cb).tobytes())
            dst = ctx.plane(h, w, dtype, stride=coeffs[k].stride).fill(0x33)
            vals = ctx.upload_bytes(np.frombuffer(b"".join(blob) or b"\0" * 4, np.uint8))
            try:
                ctx.dequant_batch([(dst, vals, recs, 0)], arith=1 if b == 2 else 0)
                assert np.array_equal(dst.download(), coeffs[k].download()), k
            finally:
                dst.free()
                vals.free()
    finally:
        for p in coeffs + quants:
            p.free()
