"""GPU: the seeded draws of tests/stats_input_draws.py on the device -- the unpack calls through tests/test_gpu_unpack.py's
`run`, the statistics calls in guarded blocks (tests/guard_lib.py) laid out by the draws' own layouts -- against the
restatements bit for bit (mssim within picture_stats_ref.mssim_bound): every destination in full, nothing written beside
it.  No draw is skipped; a call the library refuses raises and fails its test."""
import numpy as np
import pytest

import guard_lib as G
import picture_stats_cases as K
import picture_stats_ref as R
import schroedinger_amd as sa
import stats_input_draws as D
import test_gpu_unpack as T

pytestmark = pytest.mark.gpu

UNPACK = list(D.unpack_calls())
SUMS, LOWPASS, SSIM = list(D.sums_calls()), list(D.lowpass_calls()), list(D.ssim_calls())


def word(v):
    return np.array([[v & 0xffffffff]], np.uint32).view(np.uint8).reshape(1, 4)


@pytest.mark.parametrize("first", range(0, len(UNPACK), 10))
def test_unpack_draws(ctx, first):
    for n, call in enumerate(UNPACK[first:first + 10]):
        T.run(ctx, call, seed=300 + first + n)


@pytest.mark.parametrize("first", range(0, len(SUMS), 10))
def test_sums_draws(ctx, first):
    for call in SUMS[first:first + 10]:
        lay, specs = D.sums_layout(call)
        blk = G.GuardedBlock(ctx, lay, seed=len(call))
        try:
            jobs, expected = [], {}
            for e, (a, b, res) in zip(call, specs):
                pa, pb = D.sums_inputs(e)
                blk[a].upload(pa)
                if b is not None:
                    blk[b].upload(pb)
                jobs.append((blk[a], blk[b] if b is not None else None, blk[res]))
                expected[res] = np.array([R.plane_sums(pa, pb) if b is not None else R.plane_sums(pa)], np.int64).view(np.uint8).reshape(1, 16)
            assert ctx.plane_sums_batch(jobs) is None
            ctx.synchronize()
            blk.check(expected)
        finally:
            blk.free()


@pytest.mark.parametrize("first", range(0, len(LOWPASS), 6))
def test_lowpass_draws(ctx, first):
    for call in LOWPASS[first:first + 6]:
        lay, specs = D.lowpass_layout(call)
        blk = G.GuardedBlock(ctx, lay, seed=len(call))
        try:
            planes, expected = [], {}
            for n, (e, (p, c)) in enumerate(zip(call, specs)):
                a = K.lowpass_input(e["kind"], e["w"], e["h"], e["dtype"], e["seed"])
                blk[p].upload(a)
                blk[c].upload(word(n))
                out, bad = R.lowpass2(a, R.generate_coeff(e["hs"]), R.generate_coeff(e["vs"]))
                expected[p], expected[c] = out, word(n + bad)
                planes.append((blk[p], e["hs"], e["vs"], blk[c]))
            assert ctx.lowpass2_batch(planes) is None
            ctx.synchronize()
            blk.check(expected)
        finally:
            blk.free()


@pytest.mark.parametrize("first", range(0, len(SSIM), 3))
def test_ssim_draws(ctx, first):
    for call in SSIM[first:first + 3]:
        lay, specs = D.ssim_layout(call)
        blk = G.GuardedBlock(ctx, lay, seed=len(call))
        try:
            pictures, expected, want = [], {}, []
            for e, (a, b, m, scratch, result) in zip(call, specs):
                pa, pb = K.ssim_pair(e["kind"], e["w"], e["h"], e["seed"])
                blk[a].upload(pa)
                blk[b].upload(pb)
                values, counts = R.ssim_map(pa, pb)
                want.append((values, counts))
                if m is not None:
                    expected[m] = values.view(np.uint64)
                pictures.append((blk[a], blk[b], blk[m] if m is not None else None, blk[scratch], blk[result]))
            ctx.ssim_batch(pictures)
            ctx.synchronize()
            blk.check(expected)
            for n, ((values, counts), (_a, _b, _m, _s, result)) in enumerate(zip(want, specs)):
                total, got_counts = sa.Context.ssim_result(blk[result])
                assert got_counts == counts, (first, n, call[n])
                assert abs(total / values.size - R.mssim(values)) <= R.mssim_bound(values), (first, n, call[n])
        finally:
            blk.free()
