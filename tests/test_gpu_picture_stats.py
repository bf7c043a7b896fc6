"""GPU: the picture statistics -- schro_hip_plane_sums_batch, schro_hip_lowpass2_batch, schro_hip_ssim_batch and the five
frame-layer calls -- against tests/picture_stats_ref.py, bit for bit: the sums as exact integers, every low-passed sample
and out-of-range count, every pixel of the SSIM map.  Only mssim is compared within a bound, the one two orders of adding
the same doubles can differ by, computed from the restatement's map (picture_stats_ref.mssim_bound).  The planes stand
around every tile and chunk length of the kernels (tests/picture_stats_cases.py names them); the write footprint of the
low-pass and of SSIM is checked with tests/guard_lib.py."""
import numpy as np
import pytest

import analysis_ref as A
import guard_lib as G
import picture_stats_cases as K
import picture_stats_ref as R
import schroedinger_amd as sa
from schroedinger_amd import frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


def sums_of(res):
    return [tuple(int(v) for v in row) for row in res.download()]


# ---- sums ----

@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_sums_of_every_size_with_long_strides(ctx, dtype):
    jobs, want, keep = [], [], []
    for n, (w, h) in enumerate(K.SUMS_SIZES):
        a = K.noise(w, h, dtype, 10 + n) if dtype == np.uint8 else K.full_range_s16(w, h, 10 + n)
        stride = (w * np.dtype(dtype).itemsize + 63) // 64 * 64 + 64 * (n % 3)          # longer than the row
        d_a = ctx.upload(a, stride=stride)
        keep.append(d_a)
        if dtype == np.uint8:
            b = K.noise(w, h, np.uint8, 500 + n)
            d_b = ctx.upload(b, stride=stride + 64)
            keep.append(d_b)
            jobs.append((d_a, d_b))
            want.append(R.plane_sums(a, b))
        else:
            jobs.append((d_a,))
            want.append(R.plane_sums(a))
        if len(jobs) == 9 or n == len(K.SUMS_SIZES) - 1:
            assert sums_of(ctx.plane_sums_batch(jobs)) == want
            jobs, want = [], []
    [p.free() for p in keep]


def test_twelve_unlike_jobs_in_one_call_and_the_largest_squared_error(ctx):
    sizes = [(1, 1), (257, 67), (3, 2), (K.SUMS_TILE_BYTES + 1, K.SUMS_TILE_ROWS + 1), (64, 1), (K.SUMS_TILE_BYTES // 2 + 1, 3),
             (65, 67), (K.SUMS_TILE_BYTES - 1, 2), (63, K.SUMS_TILE_ROWS), (2100, 5), (5, 130), (K.SUMS_TILE_BYTES, K.SUMS_TILE_ROWS - 1)]
    jobs, want = [], []
    for n, (w, h) in enumerate(sizes):
        if n % 3 == 1:                                  # s16, full range
            a = K.full_range_s16(w, h, n)
            jobs.append((ctx.upload(a),))
            want.append(R.plane_sums(a))
        elif n % 3 == 2:                                # all 255 against all 0: the largest squared error
            a, b = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
            jobs.append((ctx.upload(a), ctx.upload(b)))
            want.append((255 * w * h, 65025 * w * h))
        else:
            a, b = K.noise(w, h, np.uint8, n), K.noise(w, h, np.uint8, n + 50)
            jobs.append((ctx.upload(a, stride=(w + 127) // 64 * 64), ctx.upload(b)))
            want.append(R.plane_sums(a, b))
    first = sums_of(ctx.plane_sums_batch(jobs))
    assert first == want
    assert sums_of(ctx.plane_sums_batch(jobs)) == first         # integers: the same bits again
    [p.free() for j in jobs for p in j]


def test_the_bright_4k_plane_exact_at_the_plane_layer_and_wrapped_at_the_frame_layer(ctx):
    w, h = 4096, 2057
    planes = [ctx.plane(h, w, np.uint8).fill(255), ctx.plane(h // 2 + 1, w // 2, np.uint8).fill(0), ctx.plane(h // 2 + 1, w // 2, np.uint8).fill(0)]
    assert sums_of(ctx.plane_sums_batch([(planes[0],)])) == [(2148495360, 0)]
    got = ctx.average_luma(frames.PlaneFrame(ctx, planes, 0, 1, 1))
    assert got == R.average_luma_of_sum(2148495360, w, h) and got < 0
    [p.free() for p in planes]


def test_sums_enqueued_behind_the_pyramid_that_feeds_them(ctx):
    """downsample_batch leaves the pyramid on the device; the sums of every level and the squared error between two
    pictures' coarsest levels are enqueued behind it on the same queue, with one wait (the download) at the end."""
    ext, levels = 8, 3
    pics = [A.picture(176, 144, 1), A.picture(176, 144, 2)]
    want_levels = [[p] for p in pics]
    dev = [[ctx.upload(p)] for p in pics]
    for k in range(levels):
        jobs = []
        for n in range(2):
            src = want_levels[n][-1]
            want_levels[n].append(A.downsample(src))
            d = ctx.plane((src.shape[0] + 1) // 2 + 2 * ext, (src.shape[1] + 1) // 2 + 2 * ext, np.uint8)
            s = dev[n][-1]
            if k:           # the picture inside the apron of the level above
                s = sa.SubPlane(s, ext, ext, src.shape[0], src.shape[1])
            jobs.append((s, d, ext))
            dev[n].append(d)
        ctx.downsample_batch(jobs)
    inner = [[dev[n][0]] + [sa.SubPlane(d, ext, ext, wl.shape[0], wl.shape[1]) for d, wl in zip(dev[n][1:], want_levels[n][1:])] for n in range(2)]
    jobs = [(p,) for n in range(2) for p in inner[n]] + [(inner[0][-1], inner[1][-1])]
    res = ctx.plane_sums_batch(jobs)
    want = [R.plane_sums(wl) for n in range(2) for wl in want_levels[n]] + [R.plane_sums(want_levels[0][-1], want_levels[1][-1])]
    assert sums_of(res) == want                                 # (the one wait)
    [p.free() for n in range(2) for p in dev[n]]


# ---- low-pass ----

def run_lowpass(ctx, cases):
    planes, want = [], []
    for (w, h, dtype, kind, hs, vs, seed) in cases:
        a = K.lowpass_input(kind, w, h, dtype, seed)
        planes.append((ctx.upload(a), hs, vs))
        want.append(R.lowpass2(a, R.generate_coeff(hs), R.generate_coeff(vs)))
    counters = ctx.lowpass2_batch(planes).download()
    for n, ((d, _, _), (out, bad)) in enumerate(zip(planes, want)):
        assert np.array_equal(d.download(), out), cases[n]
        assert int(counters[n, 0]) == bad, cases[n]
        d.free()
    return sum(bad for _, bad in want)


ALL_LOWPASS = K.lowpass_cases()


@pytest.mark.parametrize("first", range(0, len(ALL_LOWPASS), 8))
def test_lowpass_eight_unlike_planes_a_call_over_every_geometry(ctx, first):
    """u8 and s16; widths 1 .. 130 by heights 1 .. 67, the 3 x 4099 and 4099 x 3 planes, one below / at / one above
    LOWPASS_ROWS, LOWPASS_CHUNK (and twice it), LOWPASS_COLS and LOWPASS_COL_ROWS; the six sigmas, unlike along the two
    axes; noise, steps and full-range s16 -- eight unlike planes in each call."""
    run_lowpass(ctx, ALL_LOWPASS[first:first + 8])


def test_the_cases_stand_around_every_chunk_and_tile_length():
    widths, heights = {c[0] for c in ALL_LOWPASS}, {c[1] for c in ALL_LOWPASS}
    for n in (K.LOWPASS_CHUNK, 2 * K.LOWPASS_CHUNK, K.LOWPASS_COLS):
        assert {n - 1, n, n + 1} <= widths, n
    for n in (K.LOWPASS_ROWS, K.LOWPASS_COL_ROWS, 2 * K.LOWPASS_COL_ROWS):
        assert {n - 1, n, n + 1} <= heights, n
    assert {(c[4]) for c in ALL_LOWPASS} | {(c[5]) for c in ALL_LOWPASS} == set(K.SIGMAS)
    assert any(c[4] != c[5] for c in ALL_LOWPASS)
    assert {(np.dtype(c[2]).name, c[3]) for c in ALL_LOWPASS} == {("uint8", "noise"), ("uint8", "steps"), ("int16", "noise"),
                                                                  ("int16", "steps"), ("int16", "full")}


@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_steps_at_a_sharpening_sigma_count_what_leaves_the_range(ctx, dtype):
    cases = [(w, h, dtype, "steps", 0.375, 0.375, 0) for (w, h) in ((64, 8), (130, 67), (K.LOWPASS_CHUNK + 1, K.LOWPASS_ROWS + 1))]
    total = run_lowpass(ctx, cases)
    assert total > 0                                    # (the restatement's count is not zero, and the device's equals it)
    quiet = [(w, h, dtype, "steps", 0.75, 5, 0) for (w, h, *_r) in cases]
    if dtype == np.uint8:
        assert run_lowpass(ctx, quiet) == 0


def test_planes_may_share_a_counter_which_is_added_to(ctx):
    a, b = K.steps(64, 8, np.uint8), K.steps(70, 9, np.int16)
    counter = ctx.plane(1, 1, np.uint32, stride=4).upload(np.array([[1000]], np.uint32))
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    assert ctx.lowpass2_batch([(d_a, 0.375, 0.375, counter), (d_b, 0.375, 0.375, counter)]) is None
    c = R.generate_coeff(0.375)
    assert int(counter.download()[0, 0]) == 1000 + R.lowpass2(a, c, c)[1] + R.lowpass2(b, c, c)[1]
    [p.free() for p in (d_a, d_b, counter)]


# ---- SSIM ----

@pytest.mark.parametrize("kind", ["same", "noisy", "unrelated"])
def test_ssim_three_unlike_pictures_in_one_call(ctx, kind):
    pairs = [K.ssim_pair(kind, w, h, 3 + n) for n, (w, h) in enumerate(K.SSIM_SIZES)]
    dev = [(ctx.upload(a), ctx.upload(b, stride=(b.shape[1] + 127) // 64 * 64)) for a, b in pairs]
    runs = []
    for _ in range(2):
        out = ctx.ssim_batch([(a, b, True) for a, b in dev])
        runs.append([(sa.Context.ssim_result(r), m.download()) for r, m, _s in out])
        [p.free() for t in out for p in t]
    for n, (a, b) in enumerate(pairs):
        values, counts = R.ssim_map(a, b)
        (total, got_counts), got_map = runs[0][n]
        assert np.array_equal(got_map.view(np.uint64), values.view(np.uint64)), (kind, K.SSIM_SIZES[n])       # bit for bit
        assert got_counts == counts
        got = total / (a.shape[0] * a.shape[1])
        want, bound = R.mssim(values), R.mssim_bound(values)
        print("ssim %s %dx%d: mssim %.17g, restatement %.17g, |difference| %.3g, bound %.3g" % (
            kind, a.shape[1], a.shape[0], got, want, abs(got - want), bound))
        assert abs(got - want) <= bound
        if kind == "same":
            assert got == 1.0 and np.all(got_map == 1.0)
        # two runs: identical bits
        assert np.float64(runs[1][n][0][0]).view(np.uint64) == np.float64(total).view(np.uint64)
        assert np.array_equal(runs[1][n][1].view(np.uint64), got_map.view(np.uint64))
    [p.free() for t in dev for p in t]


def test_ssim_in_the_sharpening_regime_counts_out_of_range_samples(ctx):
    """Width 48 is below 128: sigma 0.28, the low-pass sharpens; a picture of hard edges leaves the range."""
    a = K.steps(48, 40, np.uint8)
    b = np.ascontiguousarray(a[:, ::-1])
    values, counts = R.ssim_map(a, b)
    assert sum(counts) > 0
    (r, m, s), = ctx.ssim_batch([(ctx.upload(a), ctx.upload(b), True)])
    total, got_counts = sa.Context.ssim_result(r)
    assert got_counts == counts
    assert np.array_equal(m.download().view(np.uint64), values.view(np.uint64))
    assert abs(total / a.size - R.mssim(values)) <= R.mssim_bound(values)


# ---- frame layer ----

def device_frame(ctx, planes, h_shift, v_shift):
    f = frames.DeviceFrame(ctx, frames.frame_format(planes[0].dtype, h_shift, v_shift), planes[0].shape[1], planes[0].shape[0])
    return f.upload(frames.HostFrame(planes, h_shift, v_shift))


@pytest.mark.parametrize("h_shift,v_shift", [(1, 1), (0, 0)])
def test_the_five_frame_calls(ctx, h_shift, v_shift):
    w, h = 130, 68
    cw, ch = w >> h_shift, h >> v_shift
    pa = [K.picture(w, h, 1), K.picture(cw, ch, 2), K.picture(cw, ch, 3)]
    pb = [np.clip(p.astype(np.int32) + np.random.default_rng(9 + k).integers(-9, 10, p.shape), 0, 255).astype(np.uint8) for k, p in enumerate(pa)]
    fa, fb = device_frame(ctx, pa, h_shift, v_shift), device_frame(ctx, pb, h_shift, v_shift)
    assert ctx.average_luma(fa) == R.average_luma(pa[0])
    assert ctx.mean_squared_error(fa, fb) == R.mean_squared_error(pa, pb)
    values, _ = R.ssim_map(pa[0], pb[0])
    assert abs(ctx.ssim(fa, fb) - R.mssim(values)) <= R.mssim_bound(values)
    assert ctx.ssim(fa, fa) == 1.0
    # the score on both sides of luma > 0.01
    average = R.average_luma(pa[0])
    assert average - 16.0 > 0.01
    assert ctx.scene_change_score(fa, fb, average) == R.scene_change_score(average, pa[0], pb[0])
    assert ctx.scene_change_score(fa, fb, 16.005) == 1.0 == R.scene_change_score(16.005, pa[0], pb[0])
    assert ctx.scene_change_score(fa, fb, 16.02) == R.scene_change_score(16.02, pa[0], pb[0]) != 1.0
    # the pre-filter, u8 then s16: the chroma sigmas divided by the format's shifts (0.75 -> 0.375: the sharpening regime)
    for sigma in (0.75, 5):
        f = device_frame(ctx, pa, h_shift, v_shift)
        ctx.filter_lowpass2(f, sigma)
        for got, want in zip(f.download(), R.frame_lowpass2(pa, sigma, h_shift, v_shift)):
            assert np.array_equal(got, want), sigma
        f.unref()
    ps = [(p.astype(np.int16) - 128) * 64 for p in pa]
    f = device_frame(ctx, ps, h_shift, v_shift)
    assert ctx.average_luma(f) == R.average_luma(ps[0])
    ctx.filter_lowpass2(f, 1.5)
    for got, want in zip(f.download(), R.frame_lowpass2(ps, 1.5, h_shift, v_shift)):
        assert np.array_equal(got, want)
    [x.unref() for x in (f, fa, fb)]


# ---- footprint ----

def test_lowpass_writes_only_its_planes_rows_and_counters(ctx):
    lay = G.Layout()
    cases = [(K.LOWPASS_CHUNK + 1, K.LOWPASS_ROWS + 1, np.uint8, "steps", 0.375, 0.75, 1), (65, 9, np.int16, "full", 1.5, 0.375, 2),
             (3, 70, np.uint8, "noise", 5, 22.5, 3)]
    specs, counters = [], []
    for (w, h, dtype, *_r) in cases:
        specs.append(lay.plane(h, w, dtype, stride=(w * np.dtype(dtype).itemsize + 3) // 2 * 2 + 62, align=64, skew=2))    # padded rows, 2-aligned
        counters.append(lay.plane(1, 1, np.uint32, align=64, skew=4))
    block = G.GuardedBlock(ctx, lay, seed=5)
    planes, expected = [], {}
    for spec, cspec, (w, h, dtype, kind, hs, vs, seed) in zip(specs, counters, cases):
        a = K.lowpass_input(kind, w, h, dtype, seed)
        block[spec].upload(a)
        block[cspec].upload(np.array([[7]], np.uint32))
        out, bad = R.lowpass2(a, R.generate_coeff(hs), R.generate_coeff(vs))
        expected[spec], expected[cspec] = out, np.array([[7 + bad]], np.uint32)
        planes.append((block[spec], hs, vs, block[cspec]))
    assert ctx.lowpass2_batch(planes) is None
    block.check(expected)
    block.free()


def test_ssim_writes_only_its_scratch_result_and_map(ctx):
    w, h = 130, 67
    a, b = K.ssim_pair("noisy", w, h, 4)
    lay = G.Layout()
    sa_, sb = lay.plane(h, w, np.uint8, stride=w + 61, footprint=None), lay.plane(h, w, np.uint8, stride=w + 3, footprint=None)
    nbytes = sa.ssim_scratch_bytes(w, h)
    scratch = lay.span(nbytes, align=64, skew=16, footprint=("bytes", nbytes))
    result = lay.span(32, align=64, skew=8, footprint=("bytes", 32))
    mp = lay.plane(h, w, np.float64, stride=8 * w + 24, align=64, skew=8)
    block = G.GuardedBlock(ctx, lay, seed=6)
    block[sa_].upload(a)
    block[sb].upload(b)
    ctx.ssim_batch([(block[sa_], block[sb], block[mp], block[scratch], block[result])])
    values, counts = R.ssim_map(a, b)
    block.check({mp: values.view(np.uint64).view(np.float64)})
    total, got_counts = sa.Context.ssim_result(block[result])
    assert got_counts == counts and abs(total / (w * h) - R.mssim(values)) <= R.mssim_bound(values)
    block.free()
