"""GPU: directed sweeps of the encoder-analysis kernels (schro_hip_metric_scan_batch, schro_hip_downsample_batch and the
rough scan over a device-made pyramid) against tests/analysis_ref.py, bit for bit.  Where tests/test_gpu_metric_scan.py and
tests/test_gpu_downsample.py pick a few sizes per class, these run a whole axis in one or two launches: every window size
(the p / scan_height magic division for all 42 divisors), every block width and height (every tail mask and window phase),
the packed minimum (metric << 11) | order at its largest metric and largest order, unlike scans in the waves of one
workgroup, planes whose rows are not dword-aligned, the downsample's register / element-wise hand-over at every column
around a tile edge, the 256-plane limit of a call, and the composition the encoder runs: a pyramid level written by the
device read by the scan."""
import numpy as np
import pytest

import analysis_ref as A
import schroedinger_amd as sa

pytestmark = pytest.mark.gpu

TABLE = sa.LIMIT_METRIC_SCAN ** 2


def make_scans(dicts):
    scans = np.zeros(len(dicts), sa.SCAN_DTYPE)
    for s, d in zip(scans, dicts):
        for k, v in d.items():
            s[k] = v
    return scans


def wanted(frame, ref, scans):
    """[(table, (dx, dy, metric))] of analysis_ref per scan."""
    out = []
    for s in scans:
        m = A.do_scan(frame, ref, s)
        out.append((m, A.get_min(m, s)))
    return out


def check_scans(ctx, pics, want=None, tag=None):
    """pics: [(frame array, ref array, frame plane, ref plane, extension, scans)], one call; tables and results of every
    scan against analysis_ref (`want`: per picture, what `wanted` gave)."""
    out = ctx.metric_scan_batch([(df, dr, ext, scans) for (_, _, df, dr, ext, scans) in pics])
    try:
        for n, ((frame, ref, _, _, ext, scans), (res, met)) in enumerate(zip(pics, out)):
            got_r, got_m = res.download(), met.download()
            for k, (s, (m, (dx, dy, metric))) in enumerate(zip(scans, want[n] if want else wanted(frame, ref, scans))):
                assert np.array_equal(got_m[k, :m.size], m), (tag, n, k, s, "table")
                assert tuple(int(v) for v in got_r[k]) == (dx, dy, metric, 0), (tag, n, k, s, got_r[k], (dx, dy, metric))
    finally:
        for res, met in out:
            res.free()
            met.free()


# ---- scan sweeps ---------------------------------------------------------------------------------------------------------

def test_scan_every_window_size(ctx):
    """All 42 x 42 window sizes in one call (every divisor of the p / scan_height division, every count of positions per
    lane), the gravity position at the window's last position."""
    W, H, ext = 128, 96, 8
    frame, ref = A.picture(W, H, 41), A.picture(W, H, 42)
    x, y, bw, bh = 60, 45, 5, 3
    dicts = []
    for sw in range(1, 43):
        for sh in range(1, 43):
            rx, ry = x - sw // 2, y - sh // 2
            dicts.append(dict(x=x, y=y, block_width=bw, block_height=bh, ref_x=rx, ref_y=ry, scan_width=sw, scan_height=sh,
                              gravity_x=rx + sw - 1 - x, gravity_y=ry + sh - 1 - y, dx=700 + sw, dy=-700 - sh))
    assert len(dicts) == 1764
    df, dr = ctx.upload(frame), ctx.upload(ref)
    check_scans(ctx, [(frame, ref, df, dr, ext, make_scans(dicts))])
    df.free(), dr.free()


def test_scan_every_block_width(ctx):
    """block_width 1 .. 64 (every tail mask, every count of dwords per row) at every byte phase of ref_x, half of the
    windows starting in an apron of 8."""
    W, H, ext = 96, 40, 8
    frame, ref = A.picture(W, H, 43), A.picture(W, H, 44)
    dicts = []
    for bw in range(1, 65):
        for ph in range(4):
            rx = ph - 8 if (bw + ph) & 1 else 16 + ph
            assert rx & 3 == ph
            x, y, ry = max(rx + 2, 0), 10 + ph, 9 + ph
            dicts.append(dict(x=x, y=y, block_width=bw, block_height=3, ref_x=rx, ref_y=ry, scan_width=6, scan_height=2,
                              gravity_x=rx + bw % 6 - x, gravity_y=ry + (bw & 1) - y, dx=-bw, dy=ph))
    scans = make_scans(dicts)
    assert len(scans) == 256 and scans["ref_x"].min() == -ext and (scans["x"] + scans["block_width"]).max() <= W
    df, dr = ctx.upload(frame), ctx.upload(ref)
    check_scans(ctx, [(frame, ref, df, dr, ext, scans)])
    df.free(), dr.free()


def test_scan_every_block_height(ctx):
    W, H, ext = 64, 96, 8
    frame, ref = A.picture(W, H, 45), A.picture(W, H, 46)
    dicts = []
    for bh in range(1, 65):
        ry = -8 + (bh & 7) if bh & 1 else 12 + (bh & 7)
        x, y, rx = 20 + (bh & 3), max(ry + 3, 0), 17 + (bh % 5)
        dicts.append(dict(x=x, y=y, block_width=12, block_height=bh, ref_x=rx, ref_y=ry, scan_width=5, scan_height=7,
                          gravity_x=rx + bh % 5 - x, gravity_y=ry + bh % 7 - y, dx=bh, dy=-bh))
    scans = make_scans(dicts)
    assert scans["ref_y"].min() < 0 and (scans["y"] + scans["block_height"]).max() <= H
    df, dr = ctx.upload(frame), ctx.upload(ref)
    check_scans(ctx, [(frame, ref, df, dr, ext, scans)])
    df.free(), dr.free()


def test_scan_packed_minimum_at_its_limits(ctx):
    """The largest metric (64 * 64 * 255 = 1 044 480, below 2^20) with the largest order (position 42 * 42 - 1, order 1764,
    below 2^11) in the wave's minimum of (metric << 11) | order."""
    W = H = 112
    big = 64 * 64 * 255
    frame = np.zeros((H, W), np.uint8)
    ref_a = np.full((H, W), 255, np.uint8)
    base = dict(x=24, y=24, block_width=64, block_height=64, ref_x=3, ref_y=3, scan_width=42, scan_height=42, dx=-1234, dy=4321)
    first = dict(base, gravity_x=3 - 24, gravity_y=3 - 24)                     # the gravity position at position 0
    last = dict(base, gravity_x=3 + 41 - 24, gravity_y=3 + 41 - 24)            # ... at position 42 * 42 - 1
    # (b): the one sample that only the last position's block covers, (3 + 41 + 63, 3 + 41 + 63)
    ref_b = ref_a.copy()
    ref_b[107, 107] = 254
    m_a, m_b = A.do_scan(frame, ref_a, first), A.do_scan(frame, ref_b, first)
    assert (m_a == big).all() and m_a.size == 1764
    assert np.flatnonzero(m_a != m_b).tolist() == [1763] and m_b[1763] == big - 1
    assert A.get_min(m_a, first) == (-1234, 4321, big)
    assert A.get_min(m_b, first) == (3 + 41 - 24, 3 + 41 - 24, big - 1)
    assert A.get_min(m_b, last) == (-1234, 4321, big - 1)
    df, da, db = ctx.upload(frame), ctx.upload(ref_a), ctx.upload(ref_b)
    check_scans(ctx, [(frame, ref_a, df, da, 0, make_scans([first, last])), (frame, ref_b, df, db, 0, make_scans([first, last]))])
    [p.free() for p in (df, da, db)]


@pytest.mark.parametrize("k", [1, 3, 8])
def test_scan_unlike_scans_in_one_workgroup(ctx, k):
    """The four waves of a workgroup each have their own job: the largest scan (which sets the launch's LDS size) beside a
    1 x 1 one, an empty block and a one-row window."""
    W, H, ext = 128, 120, 8
    frame, ref = A.picture(W, H, 47), A.picture(W, H, 48)
    rng = np.random.default_rng(k)
    kinds = [(64, 64, 42, 42), (1, 1, 1, 1), (0, 5, 3, 4), (5, 3, 42, 1)]       # (bw, bh, sw, sh)
    dicts = []
    for n in range(4 * k):
        bw, bh, sw, sh = kinds[n % 4]
        x, y = int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1))
        rx = int(np.clip(x - sw // 2, -ext, W + ext - bw - sw + 1))
        ry = int(np.clip(y - sh // 2, -ext, H + ext - bh - sh + 1))
        gi, gj = int(rng.integers(0, sw)), int(rng.integers(0, sh))
        dicts.append(dict(x=x, y=y, block_width=bw, block_height=bh, ref_x=rx, ref_y=ry, scan_width=sw, scan_height=sh,
                          gravity_x=rx + gi - x, gravity_y=ry + gj - y, dx=n, dy=-n))
    df, dr = ctx.upload(frame), ctx.upload(ref)
    check_scans(ctx, [(frame, ref, df, dr, ext, make_scans(dicts))])
    df.free(), dr.free()


def corner_scans(W, H, ext, dist):
    """The scans of tests/test_gpu_metric_scan.py's test_corner_scans_reach_into_the_apron."""
    dicts = []
    out = ext - dist
    for (bw, bh) in ((8, 8), (12, 12), (16, 16), (5, 3), (32, 32)):
        for (x, y) in ((0, 0), (W - bw, 0), (0, H - bh), (W - bw, H - bh)):
            v = out if bw >= ext else min(out, 3)
            for (dx, dy) in ((0, 0), (-v if x == 0 else v, -v if y == 0 else v)):
                rx, ry, sw, sh = sa.metric_scan_setup(x, y, bw, bh, W, H, ext, dx, dy, dist)
                assert (rx, ry, sw, sh) == A.scan_setup(x, y, bw, bh, W, H, ext, dx, dy, dist) and sw > 0 and sh > 0
                dicts.append(dict(x=x, y=y, block_width=bw, block_height=bh, ref_x=rx, ref_y=ry, scan_width=sw, scan_height=sh,
                                  gravity_x=rx - x, gravity_y=ry - y, dx=rx - x, dy=ry - y))
    return make_scans(dicts)


@pytest.mark.parametrize("which", ["frame", "ref", "both"])
def test_scan_planes_that_are_not_dword_aligned(ctx, which):
    """Views at byte offsets 1, 2 and 3 of a parent whose stride is odd: every row of the plane at another alignment, so
    the kernel's dword loads of the block and of the window are unaligned."""
    W, H, ext, stride = 160, 128, 8, 163
    frame, ref = A.picture(W, H, 49), A.picture(W, H, 50)
    scans = np.concatenate([corner_scans(W, H, ext, 4), corner_scans(W, H, ext, 12)])
    assert scans["ref_x"].min() == -ext and (scans["ref_x"] + scans["scan_width"] - 1 + scans["block_width"]).max() == W + ext
    want = [wanted(frame, ref, scans)]
    aligned = [ctx.upload(frame), ctx.upload(ref)]
    keep = list(aligned)
    for off in (1, 2, 3):
        views = []
        for n, a in enumerate((frame, ref)):
            if which in (("frame", "both"), ("ref", "both"))[n]:
                whole = A.picture(stride, H, 60 + off + n)
                whole[:, off:off + W] = a
                parent = ctx.upload(whole, stride=stride)
                keep.append(parent)
                views.append(sa.SubPlane(parent, 0, off, H, W))
                assert views[-1].stride == stride and views[-1].ptr & 3 == off
            else:
                views.append(aligned[n])
        check_scans(ctx, [(frame, ref, views[0], views[1], ext, scans)], want, tag=(which, off))
    [p.free() for p in keep]


# ---- downsample sweeps ---------------------------------------------------------------------------------------------------

def dst_view(ctx, src_shape, ext, skew=0, pad=0, fill=0x5a):
    """(parent, view): the (h + 1) // 2 + 2 * ext x (w + 1) // 2 + 2 * ext destination `skew` bytes into a pre-filled parent
    whose rows are `pad` bytes longer than skew + the destination."""
    h, w = src_shape
    dh, dw = (h + 1) // 2 + 2 * ext, (w + 1) // 2 + 2 * ext
    parent = ctx.plane(dh, dw + skew + pad, np.uint8, stride=dw + skew + pad if (skew or pad) else None).fill(fill)
    return parent, sa.SubPlane(parent, 0, skew, dh, dw)


def download_view(parent, view, skew):
    return parent.download()[:, skew:skew + view.width]


EDGE_WIDTHS = list(range(505, 521)) + list(range(1017, 1033))
EDGE_HEIGHTS = (1, 2, 15, 16, 17)

_edge = {}


def edge_pictures(kind):
    """{(w, h): (source, its downsampled picture)}, made once."""
    if kind not in _edge:
        _edge[kind] = {}
        for w in EDGE_WIDTHS:
            for h in EDGE_HEIGHTS:
                src = A.picture(w, h, 7 * w + h) if kind == "random" else A.checkerboard(w, h)
                _edge[kind][(w, h)] = (src, A.downsample(src))
    return _edge[kind]


@pytest.mark.parametrize("kind", ["random", "checkerboard"])
def test_downsample_tile_and_wave_edges(ctx, kind):
    """Source widths 505 .. 520 and 1017 .. 1032: destinations of 253 .. 260 and 509 .. 516 columns, which put the last
    register group, the first element-wise group and lane 63 on both sides of the 256-column tile edge for odd and even
    source widths at every apron phase; heights 1, 2, 15, 16, 17: destination rows around the 8-row tile.  The destinations
    start at every byte alignment (the groups' origin is (dst - apron) & 3).  One call per apron and kind of picture: the
    160 planes of a kind (a call takes at most 256)."""
    pics = edge_pictures(kind)
    keys = sorted(pics)
    srcs = {k: ctx.upload(pics[k][0]) for k in keys}
    for ext in (0, 1, 2, 3, 5, 8):
        jobs, held = [], []
        for (w, h) in keys:
            skew = (w + h) & 3
            parent, view = dst_view(ctx, (h, w), ext, skew, pad=(w + ext) % 3)
            jobs.append((srcs[(w, h)], view, ext))
            held.append((parent, view, skew))
        ctx.downsample_batch(jobs)
        for (w, h), (parent, view, skew) in zip(keys, held):
            whole = parent.download()
            assert np.array_equal(whole[:, skew:skew + view.width], A.edgeextend(pics[(w, h)][1], ext)), (kind, w, h, ext, skew)
            outside = np.ones(whole.shape, bool)
            outside[:, skew:skew + view.width] = False
            assert (whole[outside] == 0x5a).all(), (kind, w, h, ext, skew, "written outside the destination")
            parent.free()
    [p.free() for p in srcs.values()]


def test_downsample_256_planes_in_one_call(ctx):
    """The call's limit: sizes 1 x 1 to 40 x 24, mixed aprons, in both orders."""
    rng = np.random.default_rng(2560)
    shapes = [(1, 1, 0), (24, 40, 8)] + [(int(rng.integers(1, 25)), int(rng.integers(1, 41)), int(rng.choice([0, 1, 2, 3, 5, 8, 32])))
                                       for _ in range(254)]
    srcs = [A.picture(w, h, 900 + n) for n, (h, w, _) in enumerate(shapes)]
    wants = [A.edgeextend(A.downsample(s), e) for s, (_, _, e) in zip(srcs, shapes)]
    d_srcs = [ctx.upload(s) for s in srcs]
    for order in (list(range(256)), list(range(256))[::-1]):
        held = [dst_view(ctx, srcs[n].shape, shapes[n][2], skew=n & 3, pad=n % 5) for n in order]
        ctx.downsample_batch([(d_srcs[n], v, shapes[n][2]) for n, (_, v) in zip(order, held)])
        for n, (parent, view) in zip(order, held):
            assert np.array_equal(download_view(parent, view, n & 3), wants[n]), (order[0], n, shapes[n])
            parent.free()
    [p.free() for p in d_srcs]


@pytest.mark.parametrize("stride", [531, 1046])
def test_downsample_sources_that_are_views(ctx, stride):
    """Sources at byte offsets 1 .. 7 of a parent whose stride is no multiple of 4: the 8-byte source loads of the register
    path are unaligned, differently in every row."""
    w, h = stride - 9, 37
    jobs, held, wants, parents = [], [], [], []
    for off in range(1, 8):
        whole = A.picture(stride, h, 70 + off)
        parent = ctx.upload(whole, stride=stride)
        parents.append(parent)
        for ext in (0, 3):
            p, v = dst_view(ctx, (h, w), ext, skew=off & 3)
            jobs.append((sa.SubPlane(parent, 0, off, h, w), v, ext))
            held.append((p, v, off & 3))
            wants.append(A.edgeextend(A.downsample(whole[:, off:off + w]), ext))
    ctx.downsample_batch(jobs)
    for n, ((p, v, skew), want) in enumerate(zip(held, wants)):
        assert np.array_equal(download_view(p, v, skew), want), (stride, n)
        p.free()
    [p.free() for p in parents]


# ---- the pyramid into the scan ---------------------------------------------------------------------------------------------

def test_pyramid_levels_written_by_the_device_are_what_the_scan_reads(ctx):
    """What the encoder runs: four pyramid levels by downsample_batch, each with an apron of 32, level n + 1 from level n's
    picture inside its apron; at every level the rough scan over the frames the device wrote."""
    w, h, ext, levels = 176, 144, 32, 4
    rng = np.random.default_rng(176144)
    big = rng.integers(0, 256, (h + 16, w + 16), dtype=np.uint8)
    frame = np.ascontiguousarray(big[8:8 + h, 8:8 + w])
    ref = np.ascontiguousarray(big[8 + 2:8 + 2 + h, 8 - 3:8 - 3 + w])        # the frame moved by (3, -2)
    want_f, want_r = A.pyramid(frame, levels), A.pyramid(ref, levels)
    planes = [[ctx.upload(A.edgeextend(frame, ext))], [ctx.upload(A.edgeextend(ref, ext))]]
    for n in range(levels):
        jobs = []
        for chain, want in zip(planes, (want_f, want_r)):
            ph, pw = want[n].shape
            d = ctx.plane((ph + 1) // 2 + 2 * ext, (pw + 1) // 2 + 2 * ext, np.uint8).fill(0x5a)
            jobs.append((sa.SubPlane(chain[n], ext, ext, ph, pw), d, ext))
            chain.append(d)
        ctx.downsample_batch(jobs)
    P = dict(x_num_blocks=24, y_num_blocks=20, xbsep_luma=8, ybsep_luma=8)
    for shift in range(levels + 1):
        ph, pw = want_f[shift].shape
        views = [sa.SubPlane(chain[shift], 0, 0, ph + 2 * ext, pw + 2 * ext) for chain in planes]
        for distance in (4, 12):
            got = ctx.rough_scan_nohint(views[0], views[1], P, shift, distance, shift & 1, extension=ext)
            want = A.rough_scan_nohint(want_f[shift], want_r[shift], P, shift, distance, shift & 1, extension=ext)
            assert got.tobytes() == want.tobytes(), (shift, distance)
    for chain, want in zip(planes, (want_f, want_r)):
        for n, d in enumerate(chain):
            assert np.array_equal(d.download(), A.edgeextend(want[n], ext)), n
            d.free()
