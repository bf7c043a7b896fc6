"""GPU: the motion data of a noarith picture read on the device (schro_hip_motion_decode_batch, motion_dec.hip) against
tests/motion_dec_ref.py -- the field and the whole result bit for bit, with data, field and result between guard blocks."""
import ctypes as C

import numpy as np
import pytest

import encoder_pipeline_cases as EP
import guard_lib as G
import motion_dec_cases as DC
import motion_dec_ref as D
import motion_enc_ref as R
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

pytestmark = pytest.mark.gpu

WORDS = C.sizeof(_lib.MotionDecodeResult) // 4
RECORD = sa.MV_DTYPE.itemsize
INTACT, LIMITS, DAMAGED, WITNESS = DC.all_cases()


def same(field, result, want, name):
    want_field, want_result = want
    for key, value in want_result.items():
        assert result[key] == value, (name, key, result[key], value)
    got = np.ascontiguousarray(field).reshape(-1).view(sa.MV_DTYPE)
    if got.tobytes() != want_field.tobytes():
        bad = np.flatnonzero(got != want_field)
        raise AssertionError("%s: %d of %d records differ, first %d: %s, the restatement has %s" % (name, bad.size, got.size, bad[0], got[bad[0]],
                                                                                                   want_field[bad[0]]))


class Rig:
    """Some cases in one guarded block: per case the data at a byte skew (read only; a span of one byte where there is none),
    the field, the result and, where a length word is given, that word (read only)."""

    def __init__(self, ctx, cases, skews, seed, words=None):
        lay = G.Layout()
        self.cases, self.spans = cases, []
        self.words = words if words is not None else [None] * len(cases)
        for n, (case, skew, word) in enumerate(zip(cases, skews, self.words)):
            data = lay.span(max(len(case[1]), 1), align=64, skew=skew, footprint=None, name="data%d" % n)
            field = lay.span(case[2] * case[3] * RECORD, align=64, footprint=("bytes", case[2] * case[3] * RECORD), name="field%d" % n)
            res = lay.plane(1, WORDS, np.uint32, footprint="rect", name="result%d" % n)
            w = lay.plane(1, 1, np.uint32, footprint=None, name="word%d" % n) if word is not None else None
            self.spans.append((data, field, res, w))
        self.block = G.GuardedBlock(ctx, lay, seed=seed)
        for (data, field, res, w), case, word in zip(self.spans, cases, self.words):
            if len(case[1]):
                self.block[data].upload(np.frombuffer(case[1], np.uint8).reshape(1, -1))
            if w is not None:
                self.block[w].upload(np.array([[word]], np.uint32))

    def pictures(self):
        return [(self.block[d], len(c[1]), self.block[w] if w is not None else None, c[2], c[3], c[4], c[5], self.block[f], self.block[r])
                for (d, f, r, w), c in zip(self.spans, self.cases)]

    def check(self, wants):
        """Every picture's field and result; the data, the length words and the guard bands as they were."""
        for (data, field, res, w), case, want in zip(self.spans, self.cases, wants):
            same(self.block[field].download(), sa.motion_decode_result(self.block[res].download()), want, case[0])
        self.block.check()

    def free(self):
        self.block.free()


def run(ctx, cases, skews=None, seed=1, words=None, wants=None):
    rig = Rig(ctx, cases, skews if skews is not None else [n % 4 for n in range(len(cases))], seed, words)
    try:
        assert ctx.motion_decode_batch(rig.pictures()) is None
        ctx.synchronize()
        rig.check(wants if wants is not None else [DC.expected(c) for c in cases])
    finally:
        rig.free()


@pytest.mark.parametrize("case", INTACT + LIMITS, ids=lambda c: c[0])
def test_intact_streams_and_limits(ctx, case):
    run(ctx, [case], skews=[len(case[0]) % 4], seed=len(case[0]))


GROUPS = [DAMAGED[i:i + 8] for i in range(0, len(DAMAGED), 8)]


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=lambda g: "%s ..." % GROUPS[g][0][0])
def test_damaged_streams(ctx, group):
    """Eight damaged streams a call, the data at the four byte alignments."""
    cases = GROUPS[group]
    run(ctx, cases, skews=[(group + n) % 4 for n in range(len(cases))], seed=group)


def test_an_intact_and_a_damaged_stream_at_every_alignment(ctx):
    """One intact and one damaged stream at byte offsets 0, 1, 2 and 3 in one call."""
    a = next(c for c in INTACT if c[0] == "12x12 mixed refs 2")
    b = next(c for c in DAMAGED if c[0].startswith("20x12, payload bits"))
    run(ctx, [a, b] * 4, skews=[0, 0, 1, 1, 2, 2, 3, 3], seed=5)


def test_three_unlike_pictures_in_one_call(ctx):
    by_name = {c[0]: c for c in INTACT}
    cases = [by_name[n] for n in ("20x12", "8x4 mixed refs 1", "68x64: two superblocks per layout thread")]
    assert len({c[2:4] for c in cases}) == 3 and {c[4] for c in cases} == {1, 2} and {c[5] for c in cases} == {0, 1}
    run(ctx, cases, seed=3)
    run(ctx, cases[::-1], seed=4)


def test_eight_pictures_a_damaged_one_first_and_last(ctx):
    by_name = {c[0]: c for c in INTACT}
    middle = [by_name[n] for n in ("12x12 mixed refs 1", "global refs 2", "all DC", "extremes refs 2", "4x4 split 1 refs 2", "no DC")]
    first = next(c for c in DAMAGED if "filled: " in c[0] and " with 00" in c[0] and DC.expected(c)[1]["long_codes"])
    last = next(c for c in DAMAGED if "cut: " in c[0] and DC.expected(c)[1]["truncated"])
    run(ctx, [first] + middle + [last], seed=8)


@pytest.mark.parametrize("name", ["12x12 mixed refs 2", "global refs 1"])
def test_the_length_as_a_device_word(ctx, name):
    """bytes_on_device: len - 1, inside a payload, inside a header, 0, len, len + 1000.  min (word, data_bytes) bytes are read
    and the word keeps its value."""
    case = next(c for c in INTACT if c[0] == name)
    data, num_refs = case[1], case[4]
    sections = D.parse(data, num_refs)[0]
    longest = max((s for s in sections if s is not None), key=lambda s: s[1])
    inside_payload = longest[0] + longest[1] // 2
    # a payload of 15 bytes or more has a length code of two bytes: the cut between them lies inside a header
    end, inside_header = 0, None
    for s in sections:
        if s is not None and s[1]:
            if s[0] - end == 2:
                inside_header = s[0] - 1
            end = s[0] + s[1]
    assert inside_header is not None
    words = [len(data) - 1, inside_payload, inside_header, 0, len(data), len(data) + 1000]
    wants = [D.decode(data[:min(w, len(data))], *case[2:6]) for w in words]
    assert wants[1][1]["truncated"] and wants[2][1]["truncated"] and wants[4][1] == wants[5][1] == DC.expected(case)[1]
    run(ctx, [case] * len(words), seed=13, words=words, wants=wants)


@pytest.mark.parametrize("name", ["12x12 mixed refs 1", "12x12 mixed refs 2", "global refs 2"])
def test_frame_layer(ctx, name):
    """schro_hip_decode_motion_data_noarith: host bytes up, the host field and the result back."""
    case = next(c for c in INTACT if c[0] == name)
    _, data, nbx, nby, num_refs, hg, _ = case
    params = frames.make_params(x_num_blocks=nbx, y_num_blocks=nby, num_refs=num_refs, have_global_motion=hg, is_noarith=1)
    field, result = ctx.decode_motion_data_noarith(data, params)
    same(field, result, DC.expected(case), name)
    field, result = ctx.decode_motion_data_noarith(b"", params)
    same(field, result, D.decode(b"", nbx, nby, num_refs, hg), name + ", no bytes")


def test_own_buffers_wait_and_return_the_field(ctx):
    case = next(c for c in INTACT if c[0] == "20x12")
    (field, result), = ctx.motion_decode_batch([(case[1],) + tuple(case[2:6])])
    same(field, result, DC.expected(case), case[0])


def test_refusal_through_the_context(ctx):
    """A refusal enqueues nothing: the field and the result keep their canaries."""
    data = ctx.plane(1, 64, np.uint8).fill(0x80)
    field = ctx.plane(1, 16 * RECORD, np.uint8).fill(0xa5)
    res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)
    try:
        with pytest.raises(sa.SchroHipError, match=r"picture 0: num_refs 3") as e:
            ctx.motion_decode_batch([(data, 64, None, 4, 4, 3, 0, field, res)])
        assert e.value.code == -1
        ctx.synchronize()
        assert (field.download() == 0xa5).all() and (res.download() == 0xa5a5a5a5).all()
    finally:
        for p in (data, field, res):
            p.free()


def mode_pictures():
    """The small pictures of tests/mode_cases.py the encoder pipeline carries for the mode stage."""
    stage = EP.STAGES["mode"]
    names = sorted(stage["sequence"], key=lambda n: stage["cases"][n]["nbx"] * stage["cases"][n]["nby"])
    return [n for n in dict.fromkeys(names) if stage["cases"][n]["nbx"] * stage["cases"][n]["nby"] <= 2 * DC.SMALL][:3]


@pytest.mark.parametrize("name", mode_pictures())
def test_round_trip_on_the_device_without_a_host_wait(ctx, name):
    """mode_decision_batch -> motion_encode_batch -> motion_decode_batch on one queue, the last reading the encoder's `bytes`
    word: the field is the restatement's decode of the restated bytes, and canonical (the decision's field) wherever the
    encoder reports nothing unverified or asserted."""
    import mode_cases as MODE
    from test_gpu_mode_decision import Rig as ModeRig, case_entry, OUTPUTS, seed_of
    c = EP.STAGES["mode"]["cases"][name]
    nbx, nby, num_refs = c["nbx"], c["nby"], c["refs"]
    motion = MODE.expected(name)[0]
    bound = sa.motion_encode_bound(nbx, nby, num_refs, 0)
    rig = ModeRig(ctx, [case_entry(name)], OUTPUTS, seed=seed_of(name, 11))
    out = ctx.plane(1, bound, np.uint8).fill(0xa5)
    enc = ctx.plane(1, C.sizeof(_lib.MotionEncodeResult) // 4, np.uint32).fill(0xa5)
    field = ctx.plane(1, nbx * nby * RECORD, np.uint8).fill(0xa5)
    res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)
    try:
        rig.put_fields(0, *MODE.inputs(name)[2:])
        ctx.mode_decision_batch([rig.picture(0)])
        assert ctx.motion_encode_batch([(rig.span(0, "motion"), nbx, nby, num_refs, 0, out, bound, enc)]) is None
        # SchroHipMotionEncodeResult.bytes is the result's first word
        assert ctx.motion_decode_batch([(out, bound, enc, nbx, nby, num_refs, 0, field, res)]) is None
        ctx.synchronize()
        data, encoded = R.encode(motion, nbx, nby, num_refs, 0)
        assert sa.motion_encode_result(enc.download())["bytes"] == len(data)
        want = D.decode(data, nbx, nby, num_refs, 0)
        same(field.download(), sa.motion_decode_result(res.download()), want, name)
        if encoded["unverified"] == 0 and encoded["asserted"] == 0:
            assert want[0].tobytes() == R.canonical(motion).tobytes()
    finally:
        rig.free()
        for p in (out, enc, field, res):
            p.free()


@pytest.mark.parametrize("prec,pair", [(0, False), (2, True)])
def test_render_chain_decode_then_obmc_on_one_queue(ctx, prec, pair):
    """motion_decode_batch -> schro_hip_obmc_batch with no wait between them: the OBMC launch reads the field the decode
    left.  A verified drawn field without global motion; compared with the oracle's OBMC on the restatement's field."""
    import motion_enc_cases as MC
    import synth
    from test_gpu_obmc import check_case, make_case
    P = synth.motion_params(96, 64, 12, 8, prec, (1, 1, 1), (1, 1))
    nbx, nby = P["x_num_blocks"], P["y_num_blocks"]
    assert nbx % 4 == 0 and nby % 4 == 0
    drawn = MC.draw(900 + prec, nbx, nby, 2, 0, vmax=24 << prec)
    data, enc = R.encode(drawn, nbx, nby, 2, 0)
    assert enc["unverified"] == 0 and enc["asserted"] == 0
    want = D.decode(data, nbx, nby, 2, 0)
    assert want[0].tobytes() == R.canonical(drawn).tobytes()
    d_data = ctx.upload_bytes(np.frombuffer(data, np.uint8))
    d_mv = ctx.plane(1, nbx * nby * RECORD, np.uint8).fill(0xa5)
    d_res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)
    try:
        jobs, wanted, keep = make_case(ctx, 96, 64, 12, 8, prec, (1, 1, 1), (1, 1), 24 << prec, 910 + prec, pair=pair, mv=(want[0], d_mv))
        ctx.synchronize()
        assert ctx.motion_decode_batch([(d_data, len(data), None, nbx, nby, 2, 0, d_mv, d_res)]) is None
        ctx.obmc_batch(jobs)
        check_case(wanted, keep)
        same(d_mv.download(), sa.motion_decode_result(d_res.download()), want, "the field behind the render")
    finally:
        for p in (d_data, d_mv, d_res):
            p.free()
