"""GPU parity: the quantiser choice (schro_hip_quant_choose_batch) against tests/quant_choose_ref.py over the seeded
cases of tests/quant_choose_draws.py.  What no transcendental touches is compared as bits (the error estimates, the
frame lambda, the error sums); the entropy estimates and their sums at a relative 1e-9 (the device's exp and log are
within 1 ulp, as the host's are: parts in 10^16, see tests/test_quant_choose_draws.py for the margins that make the
indices and the searches' branches follow); indices, evaluation counts and not_bracketed exactly."""
import numpy as np
import pytest

import quant_choose_draws as D
import quant_choose_ref as R
import schroedinger_amd as sa

pytestmark = pytest.mark.gpu

RTOL = 1e-9
NBMAX = R.MAX_BANDS


@pytest.fixture(scope="module")
def qctx(ctx):
    one, zero = D.bit_tables()
    ctx.quant_choose_tables(D.error_table(), one, zero)
    return ctx


_COUNTS = {}


def device_counts(ctx, name):
    """the three components' SchroHipHistogramCounts arrays of a drawn picture, uploaded once"""
    if name not in _COUNTS:
        pic = D.get(name)
        nb = R.n_bands(pic["depth"])
        _COUNTS[name] = [ctx.plane(nb, 105, np.uint32, stride=420).upload(pic["counts"][c]) for c in range(3)]
    return _COUNTS[name]


def spec(ctx, name, engine, target):
    pic = D.get(name)
    return dict(counts=device_counts(ctx, name), skip=pic["skip"], depth=pic["depth"], is_intra=pic["is_intra"],
                is_noarith=pic["is_noarith"], engine=engine, weight=pic["weight"], ratio=pic["ratio"], scales=pic["scales"],
                target=target)


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.all(np.abs(got[~nan] - want[~nan]) <= RTOL * np.abs(want[~nan])), (got, want)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)


def compare(row, want, depth, engine):
    nb = R.n_bands(depth)
    assert np.array_equal(row["quant_index"][:, :nb], want["quant_index"])
    assert not row["quant_index"][:, nb:].any() and not row["chosen_entropy"][:, nb:].any() and not row["chosen_error"][:, nb:].any()
    assert int(row["evaluations"]) == want["evaluations"] and int(row["not_bracketed"]) == want["not_bracketed"]
    assert int(row["reserved"]) == 0
    same_bits(row["frame_lambda"], want["frame_lambda"])
    close(row["chosen_entropy"][:, :nb], want["chosen_entropy"])
    same_bits(row["chosen_error"][:, :nb], want["chosen_error"])
    if engine == D.E:
        same_bits(row["sum"], want["sum"])
    else:
        close(row["sum"], want["sum"])


def run(ctx, specs, **kw):
    out = ctx.quant_choose_batch(specs, **kw)
    res = out[0] if isinstance(out, tuple) else out
    try:
        rows = res.download().view(sa.QUANT_CHOICE_DTYPE).reshape(-1)
        return (rows, out[1].download()) if isinstance(out, tuple) else rows
    finally:
        res.free()
        if isinstance(out, tuple):
            out[1].free()


@pytest.mark.parametrize("name", D.ESTIMATE_CASES)
def test_estimates(qctx, name):
    pic = D.get(name)
    nb = R.n_bands(pic["depth"])
    ent, err = D.estimates(name)
    rows, est = run(qctx, [spec(qctx, name, D.L, 1.0)], estimates=True)
    got_ent = est[0].reshape(3, NBMAX, 60)[:, :nb]
    got_err = est[1].reshape(3, NBMAX, 60)[:, :nb]
    close(got_ent, ent)
    same_bits(got_err, err)
    assert int(rows[0]["evaluations"]) == 1


@pytest.mark.parametrize("k", range(len(D.ENGINE_CASES)))
def test_engines(qctx, k):
    name, engine, _ = D.ENGINE_CASES[k]
    want, _ = D.expected(k)
    rows = run(qctx, [spec(qctx, name, engine, want["target"])])
    compare(rows[0], want, D.get(name)["depth"], engine)


def test_mixed_batch(qctx):
    """eight unlike pictures in one call -- depths, forms and engines mixed --, the first of them again as the last"""
    ks = [D.case_index(n, e) for n, e in D.MIXED_BATCH]
    ks.append(ks[0])
    specs = [spec(qctx, D.ENGINE_CASES[k][0], D.ENGINE_CASES[k][1], D.expected(k)[0]["target"]) for k in ks]
    rows = run(qctx, specs)
    assert len(rows) == 9
    for row, k in zip(rows, ks):
        compare(row, D.expected(k)[0], D.get(D.ENGINE_CASES[k][0])["depth"], D.ENGINE_CASES[k][1])
    assert rows[0].tobytes() == rows[8].tobytes()


def test_one_picture_of_depth_0(qctx):
    k = D.case_index("d0", D.L)
    rows = run(qctx, [spec(qctx, "d0", D.L, D.expected(k)[0]["target"])])
    compare(rows[0], D.expected(k)[0], 0, D.L)


def test_scratch_sequence(qctx):
    """the queue's grow-only scratch through small, larger, small: one picture, nine, one"""
    k = D.case_index("d3", D.B)
    one = spec(qctx, "d3", D.B, D.expected(k)[0]["target"])
    for n in (1, 9, 1):
        for row in run(qctx, [one] * n):
            compare(row, D.expected(k)[0], 3, D.B)


def test_replaced_tables_and_missing_bit_tables(ctx):
    """a context of its own: no tables -> refused; error table alone -> a picture that is not noarith is refused, a noarith
    one runs; the tables replaced -> the new ones count"""
    own = sa.Context(0)
    try:
        k = D.case_index("d0", D.L)
        s = spec(own, "d0", D.L, D.expected(k)[0]["target"])
        s["counts"] = [own.plane(1, 105, np.uint32, stride=420).upload(D.get("d0")["counts"][c]) for c in range(3)]
        with pytest.raises(sa.SchroHipError, match="no tables"):
            own.quant_choose_batch([s])
        own.quant_choose_tables(D.error_table() * 2.0)
        with pytest.raises(sa.SchroHipError, match="picture 0: is_noarith 0 needs the one-bits and zero-bits tables"):
            own.quant_choose_batch([dict(s, is_noarith=0)])
        rows = run(own, [s], estimates=True)
        same_bits(rows[1][1].reshape(3, NBMAX, 60)[:, :1], D.estimates("d0")[1] * 2.0)
        one, zero = D.bit_tables()
        own.quant_choose_tables(D.error_table(), one, zero)
        compare(run(own, [s])[0], D.expected(k)[0], 0, D.L)
    finally:
        own.close()
