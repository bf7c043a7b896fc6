"""GPU: the picture statistics -- schro_hip_plane_sums_batch, schro_hip_lowpass2_batch, schro_hip_ssim_batch and the five
frame-layer calls -- against tests/picture_stats_ref.py, bit for bit: the sums as exact integers, every low-passed sample
and out-of-range count, every pixel of the SSIM map.  Only mssim is compared within a bound, the one two orders of adding
the same doubles can differ by, computed from the restatement's map (picture_stats_ref.mssim_bound).  The planes stand
around every tile and chunk length of the kernels (tests/picture_stats_cases.py names them); the write footprint of the
low-pass and of SSIM is checked with tests/guard_lib.py.  Further down: tables of more entries than a round of the job
lookups probes, the SSIM tile arithmetic, windows of one buffer side by side, and the frame layer at 4:2:2, odd sizes and on
the second queue."""
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

def run_ssim(ctx, kind, sizes):
    """One call of all sizes, twice: every pixel of the map and the five counters bit for bit, mssim within the bound of the
    two orders of adding, the second run's bits the first's.  Returns the restatement's counters per picture."""
    pairs = [K.ssim_pair(kind, w, h, 3 + n) for n, (w, h) in enumerate(sizes)]
    dev = [(ctx.upload(a), ctx.upload(b, stride=(b.shape[1] + 127) // 64 * 64)) for a, b in pairs]
    runs = []
    for _ in range(2):
        out = ctx.ssim_batch([(a, b, True) for a, b in dev])
        runs.append([(sa.Context.ssim_result(r), m.download()) for r, m, _s in out])
        [p.free() for t in out for p in t]
    all_counts = []
    for n, (a, b) in enumerate(pairs):
        values, counts = R.ssim_map(a, b)
        (total, got_counts), got_map = runs[0][n]
        assert np.array_equal(got_map.view(np.uint64), values.view(np.uint64)), (kind, sizes[n])       # bit for bit
        assert got_counts == counts, (kind, sizes[n])
        all_counts.append(counts)
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
        assert runs[1][n][0][1] == got_counts
    [p.free() for t in dev for p in t]
    return all_counts


@pytest.mark.parametrize("kind", ["same", "noisy", "unrelated"])
def test_ssim_three_unlike_pictures_in_one_call(ctx, kind):
    run_ssim(ctx, kind, K.SSIM_SIZES)


@pytest.mark.parametrize("kind", ["same", "noisy", "unrelated"])
def test_ssim_tile_arithmetic(ctx, kind):
    """K.SSIM_GEOMETRY_SIZES in one call: pictures narrower than the result's eight words, around both tile lengths, tiles
    across and down at once, 257 tiles under the 256 lanes that add them, both branches of generate_coeff.  The narrow
    pictures sharpen (sigma = width / 256 * 1.5 is far below 0.7) and leave the range: the counters are compared exactly."""
    counts = run_ssim(ctx, kind, K.SSIM_GEOMETRY_SIZES)
    assert all(c > 0 for c in counts[K.SSIM_GEOMETRY_SIZES.index((3, 2049))])           # thousands in each of the five planes


def ssim_tiles(w, h):
    return -(-w // K.SSIM_TILE_COLS) * -(-h // K.SSIM_TILE_ROWS)


def test_the_ssim_sizes_stand_around_the_tile_lengths_the_sum_lanes_and_the_coefficient_branch():
    sizes = K.SSIM_GEOMETRY_SIZES
    widths, heights = {w for w, _h in sizes}, {h for _w, h in sizes}
    assert {K.SSIM_TILE_COLS - 1, K.SSIM_TILE_COLS, K.SSIM_TILE_COLS + 1} <= widths
    assert {K.SSIM_TILE_ROWS - 1, K.SSIM_TILE_ROWS, K.SSIM_TILE_ROWS + 1} <= heights
    assert any(w > K.SSIM_TILE_COLS and h > K.SSIM_TILE_ROWS for w, h in sizes)         # tiles across and down at once
    assert any(w > 2 * K.SSIM_TILE_COLS and h > 2 * K.SSIM_TILE_ROWS for w, h in sizes)
    assert any(ssim_tiles(w, h) > K.SSIM_SUM_LANES for w, h in sizes)                   # the strided loop's second turn
    assert all(ssim_tiles(w, h) <= K.SSIM_SUM_LANES for w, h in K.SSIM_SIZES)           # (what the first list reaches)
    assert any(w < 8 for w in widths) and (1, 1) in sizes                               # fewer lanes in the picture than result words
    below = {w for w in widths if w / 256.0 * 1.5 < 2.5}
    assert any(w + 1 in widths - below for w in below)                                  # adjacent widths, one on either side
    assert all(w / 256.0 * 1.5 < 2.5 for w, _h in K.SSIM_SIZES)


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


# ---- full tables: more entries than one round of the job lookups probes ----
# Tiny planes (K.tiny_size), so that the table is what the test is about.  Everything lies in one guarded block: what a call
# may write is its results (or planes and counters, or scratch, result and map), and every result starts as canary bytes, so
# a result that was never cleared, or an entry looked up wrongly, shows.

def test_the_full_tables_pass_one_round_of_the_lookups():
    for counts in (K.FULL_TABLE_JOBS, K.FULL_TABLE_PLANES):
        assert min(counts) == K.TABLE_ROUND + 1 and sorted(counts)[1] > 2 * K.TABLE_ROUND and max(counts) == 4 * K.TABLE_ROUND
    # SSIM hands 2 u8 and 3 s16 low-pass planes per picture to the low-pass table
    assert [2 * n > K.TABLE_ROUND for n in K.FULL_TABLE_PICTURES] == [False, True, True]
    assert all(3 * n > K.TABLE_ROUND for n in K.FULL_TABLE_PICTURES) and max(K.FULL_TABLE_PICTURES) == K.TABLE_ROUND


@pytest.mark.parametrize("njobs", K.FULL_TABLE_JOBS)
def test_sums_full_table(ctx, njobs):
    lay, specs, want = G.Layout(), [], []
    arrays = []
    for k in range(njobs):
        w, h = K.tiny_size(k)
        if k % 3 == 2:                                  # s16, full range, alone
            a, b = K.full_range_s16(w, h, 700 + k), None
        else:                                           # u8 alone, or against a second plane
            a, b = K.noise(w, h, np.uint8, 700 + k), (K.noise(w, h, np.uint8, 1700 + k) if k % 3 == 1 else None)
        sa_ = lay.plane(h, w, a.dtype, stride=K.long_stride(k, w * a.dtype.itemsize), align=2, footprint=None, name="a%d" % k)
        sb = lay.plane(h, w, np.uint8, stride=K.long_stride(k + 3, w), align=1, footprint=None, name="b%d" % k) if b is not None else None
        res = lay.span(16, align=8, footprint=("bytes", 16), name="result%d" % k)
        specs.append((sa_, sb, res))
        arrays.append((a, b))
        want.append(np.array([R.plane_sums(a, b) if b is not None else R.plane_sums(a)], np.int64))
    blk = G.GuardedBlock(ctx, lay, seed=njobs)
    try:
        jobs = []
        for (sa_, sb, res), (a, b) in zip(specs, arrays):
            blk[sa_].upload(a)
            if sb is not None:
                blk[sb].upload(b)
            jobs.append((blk[sa_], blk[sb] if sb is not None else None, blk[res]))
        expected = {res: w.view(np.uint8).reshape(1, 16) for (_a, _b, res), w in zip(specs, want)}
        for _ in range(2):                              # (the second call finds the first's sums in the results, not the canary)
            assert ctx.plane_sums_batch(jobs) is None
            ctx.synchronize()
            blk.check(expected)
    finally:
        blk.free()


@pytest.mark.parametrize("nplanes", K.FULL_TABLE_PLANES)
def test_lowpass_full_table(ctx, nplanes):
    lay, specs, inputs, expected = G.Layout(), [], [], {}
    for k in range(nplanes):
        w, h = K.tiny_size(k)
        dtype = (np.uint8, np.int16)[(k // 2 + k // 7) % 2]
        kinds = ("noise", "steps") if dtype == np.uint8 else ("noise", "steps", "full")
        a = K.lowpass_input(kinds[k % len(kinds)], w, h, dtype, 900 + k)
        hs, vs = K.sigma_pair(k)
        bps = np.dtype(dtype).itemsize
        p = lay.plane(h, w, dtype, stride=K.long_stride(k, w * bps), align=2, name="plane%d" % k)
        c = lay.span(4, align=4, footprint=("bytes", 4), name="counter%d" % k)
        out, bad = R.lowpass2(a, R.generate_coeff(hs), R.generate_coeff(vs))
        specs.append((p, c, hs, vs))
        inputs.append(a)
        expected[p] = out
        expected[c] = np.array([[(7 * k + bad) & 0xffffffff]], np.uint32).view(np.uint8).reshape(1, 4)
    assert {np.dtype(a.dtype).name for a in inputs} == {"uint8", "int16"}
    blk = G.GuardedBlock(ctx, lay, seed=nplanes)
    try:
        for _ in range(2):                              # in place: the inputs and the counters go up again
            planes = []
            for k, ((p, c, hs, vs), a) in enumerate(zip(specs, inputs)):
                blk[p].upload(a)
                blk[c].upload(np.array([[7 * k]], np.uint32).view(np.uint8).reshape(1, 4))
                planes.append((blk[p], hs, vs, blk[c]))
            ctx.synchronize()
            assert ctx.lowpass2_batch(planes) is None
            ctx.synchronize()
            blk.check(expected)
    finally:
        blk.free()


@pytest.mark.parametrize("npictures", K.FULL_TABLE_PICTURES)
def test_ssim_full_table(ctx, npictures):
    lay, specs, pairs = G.Layout(), [], []
    kinds = ("noisy", "unrelated", "same")
    for k in range(npictures):
        w, h = K.tiny_size(k + 1)
        a, b = K.ssim_pair(kinds[k % 3], w, h, 40 + k)
        sa_ = lay.plane(h, w, np.uint8, stride=K.long_stride(k, w), align=1, footprint=None, name="a%d" % k)
        sb = lay.plane(h, w, np.uint8, stride=K.long_stride(k + 2, w), align=1, footprint=None, name="b%d" % k)
        nbytes = sa.ssim_scratch_bytes(w, h)
        scratch = lay.span(nbytes, align=16, footprint=("bytes", nbytes), name="scratch%d" % k)
        result = lay.span(32, align=8, footprint=("bytes", 32), name="result%d" % k)
        mp = lay.plane(h, w, np.uint64, stride=8 * w + 8 * (k % 4), align=8, name="map%d" % k) if k % 3 != 1 else None   # (the doubles' bits)
        specs.append((sa_, sb, scratch, result, mp))
        pairs.append((a, b))
    blk = G.GuardedBlock(ctx, lay, seed=npictures)
    try:
        pictures = []
        for (sa_, sb, scratch, result, mp), (a, b) in zip(specs, pairs):
            blk[sa_].upload(a)
            blk[sb].upload(b)
            pictures.append((blk[sa_], blk[sb], blk[mp] if mp is not None else None, blk[scratch], blk[result]))
        want = [R.ssim_map(a, b) for a, b in pairs]
        expected = {mp: values.view(np.uint64) for (_a, _b, _s, _r, mp), (values, _c) in zip(specs, want) if mp is not None}
        results = []
        for _ in range(2):
            ctx.ssim_batch(pictures)
            ctx.synchronize()
            blk.check(expected)                         # the maps bit for bit, nothing written outside scratch, result and map
            results.append([blk[result].download().tobytes() for (_a, _b, _s, result, _m) in specs])
        assert results[0] == results[1]                 # the sums, the counters and the reserved word: the same bits
        for k, ((values, counts), (_a, _b, _s, result, _m)) in enumerate(zip(want, specs)):
            total, got_counts = sa.Context.ssim_result(blk[result])
            assert got_counts == counts, k
            assert abs(total / values.size - R.mssim(values)) <= R.mssim_bound(values), k
    finally:
        blk.free()


# ---- windows of one buffer, side by side ----

class Window:
    """Columns x0 .. x0 + width - 1 of every row of a plane, as the wrappers take a plane."""

    def __init__(self, plane, x0, width):
        self.dtype, self.stride, self.height, self.width = plane.dtype, plane.stride, plane.height, width
        self.ptr = plane.ptr + x0 * plane.dtype.itemsize


def test_lowpass_windows_side_by_side_share_rows_and_nothing_else(ctx):
    """Two and three windows of one u8 buffer and of one s16 buffer in one call (rects_overlap, plane_stats.cpp, lets them
    pass): each window is the restatement's low-pass of itself, the column between two windows, the padding and every other
    byte of the block keep their bytes."""
    w, h = K.LOWPASS_CHUNK + 70, K.LOWPASS_ROWS + 3
    cuts = {2: [(0, 37), (37, w - 37)], 3: [(0, 5), (6, 64), (70, w - 70)]}             # (first column, width); column 5 is nobody's
    lay, buffers = G.Layout(), []
    for dtype in (np.uint8, np.int16):
        bps = np.dtype(dtype).itemsize
        for n in (2, 3):
            stride = w * bps + 6
            spec = lay.plane(h, w, dtype, stride=stride, align=2,
                             footprint=[(x0 * bps, stride, ww * bps, h) for x0, ww in cuts[n]], name="%s x %d" % (np.dtype(dtype).name, n))
            buffers.append((spec, dtype, cuts[n]))
    counter = lay.span(4, align=4, footprint=("bytes", 4), name="counter")
    blk = G.GuardedBlock(ctx, lay, seed=77)
    try:
        planes, expected, bad_total = [], {}, 0
        for m, (spec, dtype, cut) in enumerate(buffers):
            a = K.lowpass_input("steps" if m & 1 else "noise", w, h, dtype, 60 + m)
            blk[spec].upload(a)
            want = a.copy()
            for k, (x0, ww) in enumerate(cut):
                hs, vs = K.sigma_pair(m + 2 * k)
                out, bad = R.lowpass2(np.ascontiguousarray(a[:, x0:x0 + ww]), R.generate_coeff(hs), R.generate_coeff(vs))
                want[:, x0:x0 + ww] = out
                bad_total += bad
                planes.append((Window(blk[spec], x0, ww), hs, vs, blk[counter]))
            expected[spec] = want
        blk[counter].upload(np.array([[5]], np.uint32).view(np.uint8).reshape(1, 4))
        expected[counter] = np.array([[5 + bad_total]], np.uint32).view(np.uint8).reshape(1, 4)
        assert len(planes) == 10
        sa.lowpass2_check(planes)                        # (accepted on the host too)
        assert ctx.lowpass2_batch(planes) is None
        ctx.synchronize()
        blk.check(expected)
    finally:
        blk.free()


# ---- frame layer: the other chroma format, odd sizes, the second queue ----

def frame_planes(w, h, h_shift, v_shift):
    cw, ch = (w + (1 << h_shift) - 1) >> h_shift, (h + (1 << v_shift) - 1) >> v_shift    # rounded up
    pa = [K.picture(w, h, 1), K.picture(cw, ch, 2), K.picture(cw, ch, 3)]
    pb = [np.clip(p.astype(np.int32) + np.random.default_rng(9 + k).integers(-9, 10, p.shape), 0, 255).astype(np.uint8) for k, p in enumerate(pa)]
    return pa, pb


def five_frame_calls(ctx, w, h, h_shift, v_shift):
    """The five calls on w x h frames, every value against the restatement; returns them (mssim as its bits)."""
    pa, pb = frame_planes(w, h, h_shift, v_shift)
    fa, fb = device_frame(ctx, pa, h_shift, v_shift), device_frame(ctx, pb, h_shift, v_shift)
    out = []
    average = ctx.average_luma(fa)
    assert average == R.average_luma(pa[0])
    out.append(average)
    mse = ctx.mean_squared_error(fa, fb)
    assert mse == R.mean_squared_error(pa, pb)
    out.append(mse)
    values, _ = R.ssim_map(pa[0], pb[0])
    mssim = ctx.ssim(fa, fb)
    assert abs(mssim - R.mssim(values)) <= R.mssim_bound(values)
    assert ctx.ssim(fa, fa) == 1.0
    out.append(np.float64(mssim).view(np.uint64))
    for luma in (average, 16.005, 16.02):
        score = ctx.scene_change_score(fa, fb, luma)
        assert score == R.scene_change_score(luma, pa[0], pb[0])
        out.append(score)
    for planes, sigma in ((pa, 0.75), (pa, 5), ([(p.astype(np.int16) - 128) * 64 for p in pa], 1.5)):
        f = device_frame(ctx, planes, h_shift, v_shift)
        ctx.filter_lowpass2(f, sigma)
        got = f.download()
        for g, want in zip(got, R.frame_lowpass2(planes, sigma, h_shift, v_shift)):
            assert np.array_equal(g, want), sigma
        out.append([g.tobytes() for g in got])
        f.unref()
    [x.unref() for x in (fa, fb)]
    return out


FRAME_CASES = [(130, 68, 1, 0), (131, 67, 1, 1), (131, 67, 1, 0), (131, 67, 0, 0), (1, 1, 1, 1), (1, 1, 0, 0)]


@pytest.mark.parametrize("w,h,h_shift,v_shift", FRAME_CASES)
def test_the_five_frame_calls_at_422_odd_sizes_and_one_sample(ctx, w, h, h_shift, v_shift):
    five_frame_calls(ctx, w, h, h_shift, v_shift)


def test_the_five_frame_calls_on_the_second_queue(ctx):
    """The results pass through the selected queue's scratch head: queue 0 first runs a larger SSIM, so that its scratch has
    grown and queue 1's has not; then every case on queue 0 and on queue 1 -- the same values, the same bits."""
    assert ctx.queue() == 0
    pa, pb = frame_planes(300, 200, 1, 1)
    fa, fb = device_frame(ctx, pa, 1, 1), device_frame(ctx, pb, 1, 1)
    ctx.ssim(fa, fb)
    [x.unref() for x in (fa, fb)]
    try:
        for case in FRAME_CASES:
            ctx.select_queue(0)
            first = five_frame_calls(ctx, *case)
            ctx.select_queue(1)
            assert ctx.queue() == 1
            assert five_frame_calls(ctx, *case) == first, case
    finally:
        ctx.select_queue(0)
    assert ctx.queue() == 0
