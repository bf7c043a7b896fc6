"""GPU: schro_hip_metric_scan_batch against tests/analysis_ref.py (schro_metric_scan_do_scan + schro_metric_scan_get_min),
bit for bit, tables and results: every block size class (whole dwords, a masked last dword, the 64 x 64 limit, empty
blocks), windows from 1 x 1 to 42 x 42, windows that reach the apron at all four corners, the order of ties, two pictures
of unlike sizes in one call, one scan and 5000."""
import numpy as np
import pytest

import analysis_ref as A
import schroedinger_amd as sa

pytestmark = pytest.mark.gpu

BLOCKS = [(8, 8), (12, 12), (16, 16), (16, 5), (32, 32), (64, 64), (5, 3), (4, 4), (0, 8), (8, 0)]       # (w, h)
WINDOWS = [(1, 1), (9, 9), (25, 25), (42, 42), (42, 1)]
W, H, EXT = 160, 128, 32


@pytest.fixture(scope="module")
def ctx():
    c = sa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pictures(ctx):
    frame, ref = A.picture(W, H, 21), A.picture(W, H, 22)
    return frame, ref, ctx.upload(frame), ctx.upload(ref)


def make_scans(dicts):
    scans = np.zeros(len(dicts), sa.SCAN_DTYPE)
    for s, d in zip(scans, dicts):
        for k, v in d.items():
            s[k] = v
    return scans


def check(ctx, pics):
    """pics: [(frame array, ref array, frame plane, ref plane, extension, scans)]: run them in one call, compare all."""
    out = ctx.metric_scan_batch([(df, dr, ext, scans) for (_, _, df, dr, ext, scans) in pics])
    for (frame, ref, _, _, ext, scans), (res, met) in zip(pics, out):
        got_r, got_m = res.download(), met.download()
        for k, s in enumerate(scans):
            m = A.do_scan(frame, ref, s)
            assert np.array_equal(got_m[k, :m.size], m), (k, s)
            dx, dy, metric = A.get_min(m, s)
            assert tuple(int(v) for v in got_r[k]) == (dx, dy, metric, 0), (k, s, got_r[k])
        res.free()
        met.free()


@pytest.mark.parametrize("bw,bh", BLOCKS)
def test_every_block_size_over_every_window(ctx, pictures, bw, bh):
    frame, ref, df, dr = pictures
    rng = np.random.default_rng(bw * 100 + bh)
    dicts = []
    for (sw, sh) in WINDOWS:
        x, y = int(rng.integers(0, W - max(bw, 1))), int(rng.integers(0, H - max(bh, 1)))
        # a window somewhere around the block, inside the apron
        rx = int(np.clip(x - sw // 2, -EXT, W + EXT - bw - sw + 1))
        ry = int(np.clip(y - sh // 2, -EXT, H + EXT - bh - sh + 1))
        gi, gj = int(rng.integers(0, sw)), int(rng.integers(0, sh))
        dicts.append(dict(x=x, y=y, block_width=bw, block_height=bh, ref_x=rx, ref_y=ry, scan_width=sw, scan_height=sh,
                          gravity_x=rx + gi - x, gravity_y=ry + gj - y, dx=1000 + sw, dy=-1000 - sh))
    check(ctx, [(frame, ref, df, dr, EXT, make_scans(dicts))])


@pytest.mark.parametrize("ext", [8, 32])
@pytest.mark.parametrize("dist", [4, 12])
def test_corner_scans_reach_into_the_apron(ctx, pictures, ext, dist):
    frame, ref, df, dr = pictures
    dicts = []
    out = ext - dist            # the vector that puts the window's far side on the apron's last sample
    for (bw, bh) in ((8, 8), (12, 12), (16, 16), (5, 3), (32, 32)):
        for (x, y) in ((0, 0), (W - bw, 0), (0, H - bh), (W - bw, H - bh)):
            v = out if bw >= ext else min(out, 3)       # (a smaller block keeps its window next to the picture)
            for (dx, dy) in ((0, 0), (-v if x == 0 else v, -v if y == 0 else v)):
                rx, ry, sw, sh = sa.metric_scan_setup(x, y, bw, bh, W, H, ext, dx, dy, dist)
                assert (rx, ry, sw, sh) == A.scan_setup(x, y, bw, bh, W, H, ext, dx, dy, dist) and sw > 0 and sh > 0
                dicts.append(dict(x=x, y=y, block_width=bw, block_height=bh, ref_x=rx, ref_y=ry, scan_width=sw, scan_height=sh,
                                  gravity_x=rx - x, gravity_y=ry - y, dx=rx - x, dy=ry - y))
    scans = make_scans(dicts)
    # the windows do reach -extension and width + extension - block_width (a window starts no further out than the block is
    # wide, schrometric.c:187: the 32 x 32 blocks are the ones that reach an apron of 32)
    b = scans[scans["block_width"] == 32]
    assert b["ref_x"].min() == -ext and b["ref_y"].min() == -ext
    assert (b["ref_x"] + b["scan_width"] - 1).max() == W + ext - 32 and (b["ref_y"] + b["scan_height"] - 1).max() == H + ext - 32
    assert scans["ref_x"].min() == -ext and (scans["ref_x"] + scans["scan_width"] - 1 + scans["block_width"]).max() == W + ext
    check(ctx, [(frame, ref, df, dr, ext, scans)])


def test_ties_keep_the_reference_order(ctx):
    flat = np.full((64, 96), 77, np.uint8)
    y, x = np.mgrid[0:64, 0:96]
    period = ((x % 4) * 50 + (y * 3) % 7).astype(np.uint8)      # horizontal period 4: exact minima every 4 columns
    d_flat, d_per = ctx.upload(flat), ctx.upload(period)
    base = dict(x=40, y=24, block_width=8, block_height=8, ref_x=34, ref_y=24, scan_width=13, scan_height=1, dx=555, dy=-444)
    # gravity at i = 0 (no minimum), at i = 2 (the FIRST exact minimum: x = 36), and at i = 10 (a LATER tying minimum)
    scans = make_scans([dict(base, gravity_x=-6, gravity_y=0), dict(base, gravity_x=-4, gravity_y=0),
                        dict(base, gravity_x=4, gravity_y=0), dict(base, scan_height=9, ref_y=20, gravity_x=4, gravity_y=-4)])
    (res, met), = ctx.metric_scan_batch([(d_per, d_per, 8, scans)])
    got = res.download()
    assert tuple(got[0]) == (-4, 0, 0, 0)       # the first minimum in i-outer order: ref_x + 2 - x
    assert tuple(got[1]) == (555, -444, 0, 0)   # the gravity position ties with it: the caller's vector stays
    assert tuple(got[2]) == (555, -444, 0, 0)   # ... also when the gravity position is a later minimum
    res.free(), met.free()
    check(ctx, [(period, period, d_per, d_per, 8, scans)])
    # a flat picture: everything ties, the caller's dx, dy with the gravity metric
    f2 = np.full((64, 96), 70, np.uint8)
    d_f2 = ctx.upload(f2)
    scans = make_scans([dict(base, scan_width=9, scan_height=9, ref_x=36, ref_y=20, gravity_x=gx, gravity_y=gy)
                        for gx, gy in ((-4, -4), (0, 0), (4, 4))])
    (res, met), = ctx.metric_scan_batch([(d_flat, d_f2, 8, scans)])
    for row in res.download():
        assert tuple(row) == (555, -444, 7 * 64, 0)
    res.free(), met.free()
    check(ctx, [(flat, f2, d_flat, d_f2, 8, scans)])
    [p.free() for p in (d_flat, d_per, d_f2)]


def test_two_pictures_of_unlike_sizes_in_one_call(ctx, pictures):
    frame, ref, df, dr = pictures
    f2, r2 = A.picture(37, 29, 5), A.picture(37, 29, 6)
    d2, e2 = ctx.upload(f2), ctx.upload(r2)
    s1 = make_scans([dict(x=16 * k, y=8 * k, block_width=16, block_height=16, ref_x=16 * k - 4, ref_y=8 * k - 4, scan_width=9,
                          scan_height=9, gravity_x=0, gravity_y=0, dx=0, dy=0) for k in range(6)])
    s2 = make_scans([dict(x=8 * k, y=8, block_width=min(8, 37 - 8 * k), block_height=8, ref_x=8 * k - 2, ref_y=6, scan_width=5,
                          scan_height=5, gravity_x=-2, gravity_y=-2, dx=-2, dy=-2) for k in range(5)])
    check(ctx, [(frame, ref, df, dr, 8, s1), (f2, r2, d2, e2, 8, s2)])
    check(ctx, [(f2, r2, d2, e2, 8, s2), (frame, ref, df, dr, 8, s1)])
    [p.free() for p in (d2, e2)]


@pytest.mark.parametrize("nscans", [1, 5000])
def test_one_scan_and_5000(ctx, pictures, nscans):
    frame, ref, df, dr = pictures
    rng = np.random.default_rng(nscans)
    dicts = []
    for k in range(nscans):
        bw, bh = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        x, y = int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1))
        rx, ry, sw, sh = sa.metric_scan_setup(x, y, bw, bh, W, H, 8, 0, 0, int(rng.integers(1, 3)))
        dicts.append(dict(x=x, y=y, block_width=bw, block_height=bh, ref_x=rx, ref_y=ry, scan_width=sw, scan_height=sh,
                          gravity_x=rx - x, gravity_y=ry - y, dx=rx - x, dy=ry - y))
    check(ctx, [(frame, ref, df, dr, 8, make_scans(dicts))])
