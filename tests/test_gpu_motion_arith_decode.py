"""GPU: the motion data of an arithmetic-coded picture read on the device (schro_hip_motion_arith_decode_batch,
motion_arith_dec.hip) against tests/motion_arith_dec_ref.py -- the field and the whole result bit for bit -- and, on the
reference's own stream, against oracle/dirac_stream.py's fields and the reference decoder's digests.  Every call's data,
field and result lie between guard blocks (guard_lib.GuardedBlock), so the write footprint is checked with the values."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import arith_stream as AS
import guard_lib as G
import motion_arith_dec_cases as AC
import motion_arith_dec_ref as A
import noarith_twin as T
import schroedinger_amd as sa
import stream_lib as S
from schroedinger_amd import _lib, frames
from test_gpu_arith_decode import ArithChain
from test_gpu_noarith_decode import same_result
from test_gpu_noarith_twin import CLEAN

pytestmark = pytest.mark.gpu

WORDS = C.sizeof(_lib.MotionArithDecodeResult) // 4
RECORD = sa.MV_DTYPE.itemsize
INTACT, LIMITS, HOSTILE, WITNESS = AC.all_cases()
LARGE = [c for c in LIMITS if c[2] * c[3] > AC.SMALL]
ONE_BY_ONE = [c for c in INTACT + LIMITS if c[2] * c[3] <= AC.SMALL] + LARGE


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
            same(self.block[field].download(), sa.motion_arith_decode_result(self.block[res].download()), want, case[0])
        self.block.check()

    def free(self):
        self.block.free()


def run(ctx, cases, skews=None, seed=1, words=None, wants=None):
    rig = Rig(ctx, cases, skews if skews is not None else [n % 4 for n in range(len(cases))], seed, words)
    try:
        assert ctx.motion_arith_decode_batch(rig.pictures()) is None
        ctx.synchronize()
        rig.check(wants if wants is not None else [AC.expected(c) for c in cases])
    finally:
        rig.free()


# ---- the reference's stream ---------------------------------------------------------------------------------------------------

def test_stream_pictures_of_the_first_twelve_in_one_call(ctx):
    """The eleven inter pictures among the stream's first twelve, their motion data as the stream carries it, at data skews
    0 .. 3 in one call: each field is the oracle's byte for byte, the results are the restatement's."""
    numbers = [n for n in T.FIRST_TWELVE if n != 0]
    recs = {r["number"]: r for r in T.motion_pictures(numbers=set(numbers))}
    cases, wants = [], []
    for n in numbers:
        r = recs[n]
        data = A.stream_motion(n)
        cases.append(("picture %d" % n, data, r["nbx"], r["nby"], r["num_refs"], 0, "serial"))
        want = A.decode(data, r["nbx"], r["nby"], r["num_refs"], 0)
        assert want[0].tobytes() == r["mv"].tobytes()
        wants.append((r["mv"], want[1]))
    assert len(cases) == 11 and {c[4] for c in cases} == {1, 2}
    run(ctx, cases, seed=12, wants=wants)


class StreamChain(ArithChain):
    """ArithChain with its upload replaced: the field comes from motion_arith_decode_batch on the stream's motion bytes."""

    def __init__(self, ctx, rec, refs):
        ArithChain.__init__(self, ctx, rec, refs)
        if rec["num_refs"]:
            P = rec["twin"]
            self.mbytes = A.stream_motion(rec["number"])
            self.mdata = self._own(ctx.upload_bytes(np.frombuffer(self.mbytes, np.uint8)))
            self.field.free()
            self.keep.remove(self.field)
            self.field = self._own(ctx.plane(1, P["nbx"] * P["nby"] * RECORD, np.uint8).fill(0xa5))
            self.mres = self._own(ctx.plane(1, WORDS, np.uint32).fill(0xa5))
            self.geometry = (P["nbx"], P["nby"], rec["num_refs"], 0)

    def enqueue(self):
        if self.pic["motion"] is not None:
            assert self.ctx.motion_arith_decode_batch([(self.mdata, len(self.mbytes), None) + self.geometry + (self.field, self.mres)]) is None
        ArithChain.enqueue(self)


def test_stream_bytes_to_pixels(ctx):
    """Pictures 0, 3, 1, 2 in coded order: motion data and transform data decoded on the device from the stream's bytes,
    inverse wavelet and OBMC enqueued behind them on one queue, one wait at the end.  Pictures 0, 1, 2 give the reference
    decoder's own digests."""
    md5 = json.load(open(os.path.join(S.GOLDEN, "stream_md5.json")))
    recs = [r for r in AS.pictures(limit=4)]
    assert [r["number"] for r in recs] == [0, 3, 1, 2]
    chains, decoded = [], {}
    try:
        for rec in recs:
            chain = StreamChain(ctx, rec, [decoded[n] for n in rec["refs"]])
            chains.append(chain)
            decoded[rec["number"]] = chain.out
        ctx.synchronize()
        for chain in chains:
            chain.enqueue()
        ctx.synchronize()
        digests = {}
        for rec, chain in zip(recs, chains):
            same_result(sa.arith_decode_result(chain.tres.download()), dict(CLEAN, bytes_read=len(rec["arith"])), "picture %d" % rec["number"])
            if rec["num_refs"]:
                want = A.decode(chain.mbytes, *chain.geometry)
                same(chain.field.download(), sa.motion_arith_decode_result(chain.mres.download()), (rec["mv"], want[1]), "picture %d" % rec["number"])
            got = [o.download() for o in chain.out]
            for k in range(3):
                assert np.array_equal(got[k], rec["out"][k]), (rec["number"], k)
            digests[rec["number"]] = S.D.frame_md5(got)
        assert [digests[n] for n in (0, 1, 2)] == md5["reference"]
    finally:
        for chain in chains:
            chain.free()


# ---- written and hostile streams ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ONE_BY_ONE, ids=lambda c: c[0])
def test_intact_streams_and_limits(ctx, case):
    """One picture per call; the small ones at the four byte alignments in turn, the two large limits at one."""
    if case in LARGE:
        run(ctx, [case], skews=[len(case[0]) % 4], seed=len(case[0]))
    else:
        run(ctx, [case] * 4, skews=[0, 1, 2, 3], seed=len(case[0]))


def test_intact_fields_are_the_fields_written(ctx):
    """The arithmetic writer's round trip on the device: a call of every small intact stream gives the field it was written from."""
    cases = [c for c in INTACT if c[2] * c[3] <= AC.SMALL]
    wants = [(AC.field_of(c), AC.expected(c)[1]) for c in cases]
    run(ctx, cases, seed=2, wants=wants)


def test_calls_of_three_and_of_eight_unlike_pictures(ctx):
    every = [c for c in INTACT + LIMITS if c not in LARGE]
    three = [every[i:i + 3] for i in range(0, len(every), 3)]
    eight = [every[i:i + 8] for i in range(1, len(every), 8)]
    for n, cases in enumerate(three + eight):
        run(ctx, cases, seed=30 + n)
    used = [c for g in three + eight for c in g]
    assert {(4, 4)} <= {c[2:4] for c in used} and {c[4] for c in used} == {1, 2} and {c[5] for c in used} == {0, 1}
    assert any(len({c[2:6] for c in g}) >= 3 for g in eight)


def test_more_than_64_chains_in_one_launch(ctx):
    """Every small intact stream and limit in one call: the value launch has seven chains a picture."""
    cases = [c for c in INTACT + LIMITS if c[2] * c[3] <= AC.SMALL]
    assert 7 * len(cases) > 64
    run(ctx, cases, seed=64)


GROUPS = [HOSTILE[i:i + 8] for i in range(0, len(HOSTILE), 8)]


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=lambda g: "%s ..." % GROUPS[g][0][0])
def test_hostile_streams(ctx, group):
    """Eight hostile streams a call, the data at the four byte alignments."""
    cases = GROUPS[group]
    run(ctx, cases, skews=[(group + n) % 4 for n in range(len(cases))], seed=group)


@pytest.mark.parametrize("name", ["12x12 mixed refs 2", "global refs 1"])
def test_the_length_as_a_device_word(ctx, name):
    """bytes_on_device: len - 1, inside a payload, 0, len, len + 1000.  min (word, data_bytes) bytes are read and the word
    keeps its value (the guarded block checks it)."""
    case = AC.intact_by_name(name)
    data, num_refs = case[1], case[4]
    sections = A.parse(data, num_refs)[0]
    longest = max((s for s in sections if s is not None), key=lambda s: s[1])
    words = [len(data) - 1, longest[0] + longest[1] // 2, 0, len(data), len(data) + 1000]
    wants = [A.decode(data[:min(w, len(data))], *case[2:6]) for w in words]
    assert wants[1][1]["truncated"] and wants[3][1] == wants[4][1] == AC.expected(case)[1]
    run(ctx, [case] * len(words), seed=13, words=words, wants=wants)


def test_a_fresh_context_grows_its_scratch_and_nine_calls_run_without_a_wait():
    """On a context of its own: a small, a larger and a small picture three times over, nothing waited for between the
    calls, so that the queue's scratch has to grow under calls that are still in flight."""
    small, large = AC.intact_by_name("8x4 mixed refs 2"), AC.intact_by_name("draw 5 refs 2 (20x20, global 1, |v| <= 2000)")
    entry = lambda c: (0x1000, len(c[1]), None, c[2], c[3], c[4], c[5], 0x100000, 0x200000)
    assert sa.motion_arith_decode_scratch_words([entry(large)]) > sa.motion_arith_decode_scratch_words([entry(small)])
    ctx = sa.Context(0)
    rigs = []
    try:
        for n, case in enumerate([small, large, small] * 3):
            rigs.append(Rig(ctx, [case], [n % 4], seed=70 + n))
        ctx.synchronize()
        for rig in rigs:
            assert ctx.motion_arith_decode_batch(rig.pictures()) is None
        ctx.synchronize()
        for rig in rigs:
            rig.check([AC.expected(c) for c in rig.cases])
    finally:
        for rig in rigs:
            rig.free()
        ctx.close()


@pytest.mark.parametrize("name", ["12x12 mixed refs 1", "12x12 mixed refs 2", "global refs 2"])
def test_frame_layer(ctx, name):
    """schro_hip_decode_motion_data_arith: host bytes up, the host field and the result back; a length of 0; noarith refused."""
    case = AC.intact_by_name(name)
    _, data, nbx, nby, num_refs, hg, _ = case
    params = frames.make_params(x_num_blocks=nbx, y_num_blocks=nby, num_refs=num_refs, have_global_motion=hg, is_noarith=0)
    field, result = ctx.decode_motion_data_arith(data, params)
    same(field, result, AC.expected(case), name)
    field, result = ctx.decode_motion_data_arith(b"", params)
    same(field, result, A.decode(b"", nbx, nby, num_refs, hg), name + ", no bytes")
    params.is_noarith = 1
    with pytest.raises(sa.SchroHipError, match="noarith"):
        ctx.decode_motion_data_arith(data, params)


def test_own_buffers_wait_and_return_the_field(ctx):
    case = AC.intact_by_name("20x12")
    (field, result), = ctx.motion_arith_decode_batch([(case[1],) + tuple(case[2:6])])
    same(field, result, AC.expected(case), case[0])


def test_refusal_through_the_context(ctx):
    """A refusal enqueues nothing: the field and the result keep their canaries."""
    data = ctx.plane(1, 64, np.uint8).fill(0x80)
    field = ctx.plane(1, 16 * RECORD, np.uint8).fill(0xa5)
    res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)
    try:
        with pytest.raises(sa.SchroHipError, match=r"picture 0: num_refs 3") as e:
            ctx.motion_arith_decode_batch([(data, 64, None, 4, 4, 3, 0, field, res)])
        assert e.value.code == -1
        ctx.synchronize()
        assert (field.download() == 0xa5).all() and (res.download() == 0xa5a5a5a5).all()
    finally:
        for p in (data, field, res):
            p.free()


@pytest.mark.parametrize("prec,pair", [(0, False), (2, True)])
def test_render_chain_decode_then_obmc_on_one_queue(ctx, prec, pair):
    """motion_arith_decode_batch -> schro_hip_obmc_batch with no wait between them: the OBMC launch reads the field the
    decode left.  A verified drawn field without global motion; compared with the oracle's OBMC on the restatement's field."""
    import motion_enc_cases as MC
    import motion_enc_ref as R
    import synth
    from test_gpu_obmc import check_case, make_case
    P = synth.motion_params(96, 64, 12, 8, prec, (1, 1, 1), (1, 1))
    nbx, nby = P["x_num_blocks"], P["y_num_blocks"]
    assert nbx % 4 == 0 and nby % 4 == 0
    drawn = R.canonical(MC.draw(900 + prec, nbx, nby, 2, 0, vmax=24 << prec))
    data = A.write_field(drawn, nbx, nby, 2, 0)
    want = A.decode(data, nbx, nby, 2, 0)
    assert want[0].tobytes() == drawn.tobytes()
    d_data = ctx.upload_bytes(np.frombuffer(data, np.uint8))
    d_mv = ctx.plane(1, nbx * nby * RECORD, np.uint8).fill(0xa5)
    d_res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)
    try:
        jobs, wanted, keep = make_case(ctx, 96, 64, 12, 8, prec, (1, 1, 1), (1, 1), 24 << prec, 910 + prec, pair=pair, mv=(want[0], d_mv))
        ctx.synchronize()
        assert ctx.motion_arith_decode_batch([(d_data, len(data), None, nbx, nby, 2, 0, d_mv, d_res)]) is None
        ctx.obmc_batch(jobs)
        check_case(wanted, keep)
        same(d_mv.download(), sa.motion_arith_decode_result(d_res.download()), want, "the field behind the render")
    finally:
        for p in (d_data, d_mv, d_res):
            p.free()
