"""GPU: schro_hip_motion_decode_batch as a stream of enqueued calls, on contexts of its own: the queue's grow-only scratch
from empty through a small, a four times larger and a smaller call with no wait between them, the synchronous frame-layer
entry point behind them, and nine calls without a wait -- more tables in flight than a queue has buffers --, every field
and result bit for bit."""
import ctypes as C

import numpy as np
import pytest

import motion_dec_cases as DC
import schroedinger_amd as sa
from schroedinger_amd import _lib, frames
from test_gpu_motion_decode import same

pytestmark = pytest.mark.gpu

WORDS = C.sizeof(_lib.MotionDecodeResult) // 4
RECORD = sa.MV_DTYPE.itemsize
INTACT, LIMITS, DAMAGED, _ = DC.all_cases()


def words_of(case):
    return DC.scratch_words([dict(nbx=case[2], nby=case[3], data_bytes=len(case[1]))])


class Call:
    """One picture with buffers of its own, filled with a canary."""

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        self.data = ctx.plane(1, max(len(case[1]), 1), np.uint8)
        if len(case[1]):
            self.data.upload(np.frombuffer(case[1], np.uint8).reshape(1, -1))
        self.field = ctx.plane(1, case[2] * case[3] * RECORD, np.uint8).fill(0xa5)
        self.res = ctx.plane(1, WORDS, np.uint32).fill(0xa5)

    def enqueue(self):
        c = self.case
        assert self.ctx.motion_decode_batch([(self.data, len(c[1]), None, c[2], c[3], c[4], c[5], self.field, self.res)]) is None

    def check(self):
        same(self.field.download(), sa.motion_decode_result(self.res.download()), DC.expected(self.case), self.case[0])

    def free(self):
        for p in (self.data, self.field, self.res):
            p.free()


def test_scratch_from_empty_grown_and_reused_then_the_synchronous_entry():
    by_name = {c[0]: c for c in INTACT + LIMITS}
    small, large, smaller = by_name["12x12 mixed refs 2"], by_name["20x12"], by_name["8x4 mixed refs 1"]
    large = by_name["68x64: two superblocks per layout thread"] if words_of(large) < 4 * words_of(small) else large
    assert words_of(large) >= 4 * words_of(small) and words_of(smaller) < words_of(small)
    ctx = sa.Context(0)
    try:
        calls = [Call(ctx, c) for c in (small, large, smaller)]
        try:
            ctx.synchronize()           # (the last wait in front of the sequence)
            for call in calls:
                call.enqueue()
            # the frame layer sizes the block itself and waits
            _, data, nbx, nby, num_refs, hg, _ = small
            params = frames.make_params(x_num_blocks=nbx, y_num_blocks=nby, num_refs=num_refs, have_global_motion=hg, is_noarith=1)
            field, result = ctx.decode_motion_data_noarith(data, params)
            same(field, result, DC.expected(small), "the frame layer behind the sequence")
            again = Call(ctx, large)
            calls.append(again)
            again.enqueue()
            ctx.synchronize()
            for call in calls:
                call.check()
        finally:
            for call in calls:
                call.free()
    finally:
        ctx.close()


def test_nine_calls_without_a_wait():
    by_name = {c[0]: c for c in INTACT + LIMITS + DAMAGED}
    damaged = next(c for c in DAMAGED if "any bits" in c[0] and c[2] * c[3] >= 96)
    three = [by_name["global refs 2"], by_name["64 codes in a chunk"], damaged]
    assert len({c[2:6] for c in three}) == 3
    ctx = sa.Context(0)
    try:
        calls = [Call(ctx, three[k % 3]) for k in range(9)]
        try:
            ctx.synchronize()           # (the last wait in front of the nine calls)
            for call in calls:
                call.enqueue()
            ctx.synchronize()
            for call in calls:
                call.check()
        finally:
            for call in calls:
                call.free()
    finally:
        ctx.close()
