"""GPU: the motion data of a noarith picture written on the device (schro_hip_motion_encode_batch, motion_enc.hip) against
tests/motion_enc_ref.py byte for byte, with the output between guard blocks."""
import ctypes as C

import numpy as np
import pytest

import encoder_pipeline_cases as EP
import guard_lib as G
import motion_enc_cases as MC
import motion_enc_ref as R
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames

pytestmark = pytest.mark.gpu

WORDS = C.sizeof(_lib.MotionEncodeResult) // 4
_EXPECTED = {}


def expected(case):
    """The restatement's (bytes, result) of a case, computed once."""
    if case[0] not in _EXPECTED:
        _EXPECTED[case[0]] = R.encode(*case[1:6])
    return _EXPECTED[case[0]]


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(1, -1)


def same(got, result, case, room=None):
    """Byte for byte, naming the first differing byte and its section; then the rest of the result."""
    name, field, nbx, nby, num_refs, hg, _ = case
    data, want = expected(case)
    room = len(data) if room is None else room
    assert result["bytes"] == len(data), (name, result["bytes"], len(data))
    assert result["overrun"] == int(room < len(data)), name
    got, cut = bytes(got), data[:room]
    if got != cut:
        assert len(got) == len(cut), (name, len(got), len(cut))
        n = next(i for i, (a, b) in enumerate(zip(got, cut)) if a != b)
        raise AssertionError("%s: byte %d of %d (%s) is %02x, the reference writes %02x" % (name, n, len(data), R.section_of(data, num_refs, n),
                                                                                           got[n], data[n]))
    for key in ("section_bytes", "section_units", "asserted", "unverified", "first_unverified"):
        assert result[key] == want[key], (name, key, result[key], want[key])


class Rig:
    """Some cases in one guarded block: per case the field (read only), the output at a byte skew with `room` bytes (a span of one byte
    where the room is 0) and the result."""

    def __init__(self, ctx, cases, rooms, skews, seed):
        lay = G.Layout()
        self.cases, self.rooms, self.spans = cases, rooms, []
        for n, (case, room, skew) in enumerate(zip(cases, rooms, skews)):
            data = expected(case)[0]
            field = lay.span(case[1].nbytes, align=64, footprint=None, name="field%d" % n)
            out = lay.span(max(room, 1), align=64, skew=skew, footprint=("bytes", min(room, len(data))), name="out%d" % n)
            res = lay.plane(1, WORDS, np.uint32, footprint="rect", name="result%d" % n)
            self.spans.append((field, out, res))
        self.block = G.GuardedBlock(ctx, lay, seed=seed)
        for (field, out, res), case in zip(self.spans, cases):
            self.block[field].upload(as_bytes(case[1]))

    def pictures(self):
        return [(self.block[f], c[2], c[3], c[4], c[5], self.block[o], room, self.block[r])
                for (f, o, r), c, room in zip(self.spans, self.cases, self.rooms)]

    def check(self):
        """Every picture's bytes and result; the canaries behind the bytes, the fields and the guard bands as they were."""
        want = {}
        for (field, out, res), case, room in zip(self.spans, self.cases, self.rooms):
            data = expected(case)[0]
            result = sa.motion_encode_result(self.block[res].download())
            take = min(room, len(data))
            same(self.block[out].download()[0, :take], result, case, room)
            tail = self.block.before[out.offset + take:out.offset + max(room, 1)]      # (the canary behind the bytes)
            want[out] = np.concatenate([np.frombuffer(data[:take], np.uint8), tail]).reshape(1, -1)
        self.block.check(want)

    def free(self):
        self.block.free()


def run(ctx, cases, rooms=None, skews=None, seed=1):
    rooms = rooms if rooms is not None else [sa.motion_encode_bound(*c[2:6]) for c in cases]
    rig = Rig(ctx, cases, rooms, skews if skews is not None else [n % 4 for n in range(len(cases))], seed)
    try:
        assert ctx.motion_encode_batch(rig.pictures()) is None
        ctx.synchronize()
        rig.check()
    finally:
        rig.free()


@pytest.mark.parametrize("case", MC.all_cases(), ids=lambda c: c[0])
def test_batch_is_the_reference_byte_for_byte(ctx, case):
    run(ctx, [case], seed=len(case[0]))


def test_own_buffers_wait_and_return_the_bytes(ctx):
    case = next(c for c in MC.all_cases() if c[0] == "12x12 mixed refs 2")
    field = ctx.upload_bytes(case[1])
    try:
        (got, result), = ctx.motion_encode_batch([(field,) + tuple(case[2:6])])
        same(got, result, case)
    finally:
        field.free()


def test_three_unlike_pictures_in_one_call(ctx):
    by_name = {c[0]: c for c in MC.all_cases()}
    cases = [by_name[n] for n in ("20x12", "8x4 mixed refs 1", "68x64: two superblocks per layout thread")]
    assert len({c[2:4] for c in cases}) == 3 and {c[4] for c in cases} == {1, 2}
    run(ctx, cases, seed=3)
    run(ctx, cases[::-1], seed=4)


@pytest.mark.parametrize("name", ["12x12 mixed refs 2", "extremes refs 2", "global refs 1"])
def test_capacity_and_alignment(ctx, name):
    """Capacity bytes - 1, 1 and 0 and the exact size, the output at byte offsets 1, 2 and 3: the first `capacity` bytes, the
    size the picture needs and the over-run flag; nothing behind the capacity is touched."""
    case = next(c for c in MC.all_cases() if c[0] == name)
    n = len(expected(case)[0])
    run(ctx, [case] * 6, rooms=[n - 1, 1, 0, n, n - 1, n + 5], skews=[1, 2, 3, 3, 0, 1], seed=n)


def test_asserted_pictures_end_inside_their_buffers(ctx):
    """Split 3 and using_global without the flag: the counts are the restatement's (so are the bytes, though unspecified),
    the call returns and the guard bands are intact -- also with no room at all."""
    cases = [c for c in MC.all_cases() if c[0] in ("split 3", "using_global without the flag")]
    assert len(cases) == 2 and all(expected(c)[1]["asserted"] > 0 for c in cases)
    run(ctx, cases + cases, rooms=[sa.motion_encode_bound(*c[2:6]) for c in cases] + [3, 0], seed=9)


def test_broken_copies_are_reported(ctx):
    for case in [c for c in MC.all_cases() if c[0].startswith("broken copies")]:
        want = expected(case)[1]
        assert want["unverified"] == 1 and want["first_unverified"] >= 0
        run(ctx, [case], seed=11)


PARAMS = dict(is_noarith=1)


@pytest.mark.parametrize("name,short", [("12x12 mixed refs 2", 0), ("global refs 1", 0), ("extremes refs 1", 1)])
def test_frame_layer(ctx, name, short):
    """schro_hip_encode_motion_data_noarith on a host field: the same bytes in the host buffer, the size, the sections; with a
    buffer one byte short SCHRO_HIP_ENOMEM, the size and the first bytes."""
    case = next(c for c in MC.all_cases() if c[0] == name)
    _, field, nbx, nby, num_refs, hg, _ = case
    data, want = expected(case)
    params = frames.make_params(x_num_blocks=nbx, y_num_blocks=nby, num_refs=num_refs, have_global_motion=hg, **PARAMS)
    capacity = len(data) - 1 if short else sa.motion_encode_bound(nbx, nby, num_refs, hg)
    got, nbytes, sections, result, status = ctx.encode_motion_data_noarith(field, params, capacity)
    assert nbytes == len(data) and sections == want["section_bytes"]
    assert status == (-3 if short else 0)
    if short:
        assert b"takes %d bytes" % len(data) in ctx.lib.schro_hip_last_error()
    same(got, result, case, capacity)


def test_refusal_through_the_context(ctx):
    """A refusal enqueues nothing: the output and the result keep their canaries."""
    out = ctx.plane(1, 256, np.uint8).fill(0xa5)
    res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)
    field = ctx.upload_bytes(np.zeros(16, sa.MV_DTYPE))
    try:
        with pytest.raises(sa.SchroHipError, match=r"picture 0: num_refs 3") as e:
            ctx.motion_encode_batch([(field, 4, 4, 3, 0, out, 256, res)])
        assert e.value.code == -1
        ctx.synchronize()
        assert (out.download() == 0xa5).all() and (res.download() == 0xa5a5a5a5).all()
    finally:
        for p in (out, res, field):
            p.free()


def test_chain_mode_decision_then_motion_data_without_a_wait(ctx):
    """mode_decision_batch, then motion_encode_batch on the mode stage's `motion` on the same queue with no wait between
    them, on the smallest picture tests/encoder_pipeline_cases.py carries for the mode stage: the bytes decode back to the
    canonical form of the field the mode stage left."""
    import mode_cases as MODE
    from test_gpu_mode_decision import Rig as ModeRig, case_entry, OUTPUTS, seed_of
    stage = EP.STAGES["mode"]
    name = min(stage["sequence"], key=lambda n: stage["cases"][n]["nbx"] * stage["cases"][n]["nby"])
    c = stage["cases"][name]
    nbx, nby, num_refs = c["nbx"], c["nby"], c["refs"]
    motion = MODE.expected(name)[0]
    bound = sa.motion_encode_bound(nbx, nby, num_refs, 0)
    rig = ModeRig(ctx, [case_entry(name)], OUTPUTS, seed=seed_of(name, 7))
    out = ctx.plane(1, bound, np.uint8).fill(0xa5)
    res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)
    try:
        rig.put_fields(0, *MODE.inputs(name)[2:])
        ctx.mode_decision_batch([rig.picture(0)])
        assert ctx.motion_encode_batch([(rig.span(0, "motion"), nbx, nby, num_refs, 0, out, bound, res)]) is None
        ctx.synchronize()
        result = sa.motion_encode_result(res.download())
        assert result["overrun"] == 0 and result["asserted"] == 0 and result["unverified"] == 0
        data = bytes(out.download()[0, :result["bytes"]])
        assert data == R.encode(motion, nbx, nby, num_refs, 0)[0]
        assert R.decode(data, nbx, nby, num_refs, 0).tobytes() == R.canonical(motion).tobytes()
        rig.check({(0, nm): a for nm, a in zip(OUTPUTS, MODE.expected(name)[:4])})
    finally:
        rig.free()
        out.free()
        res.free()
