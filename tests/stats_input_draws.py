"""Seeded random calls of the encoder's way in and of the picture statistics, as generators that need no device (in the
style of tests/encoder_front_draws.py): the pictures of schro_hip_unpack_batch calls and the entries of
schro_hip_plane_sums_batch, schro_hip_lowpass2_batch and schro_hip_ssim_batch calls, with the layouts (tests/guard_lib.py)
that place a call's planes in one block.  tests/test_stats_input_draws.py checks on the host that every draw is legal and
what the draws cover; tests/test_gpu_stats_input_draws.py walks them on the device."""
import numpy as np

import guard_lib as G
import picture_stats_cases as K
import schroedinger_amd as sa
import unpack_ref as U

TILE_BYTES = sa.unpack_geometry()["tile_bytes"]
EVEN_ONLY = (U.YUYV, U.UYVY, U.V216)
DEPTHS = (np.uint8, np.int16, np.int32)
SHIFTS = ((0, 0), (1, 0), (1, 1))
OFFSETS = (0, 0, 0, 1, 2, 3, 16)
UNPACK_CALLS, STATS_CALLS = 40, 30
MOST_SSIM_PICTURES = 64         # what one schro_hip_ssim_batch call takes: 192 entries of its low-pass table


def _size(rng, dst_bpp):
    """Most below 300 x 80; one in eight wide: up to 2 T + 40 bytes of destination row by at most 12 rows."""
    if rng.integers(0, 8) == 0:
        return int(rng.integers(300, (2 * TILE_BYTES + 40) // dst_bpp + 1)), int(rng.integers(1, 13))
    return int(rng.integers(1, 300)), int(rng.integers(1, 80))


def unpack_picture(rng):
    """One picture as tests/test_gpu_unpack.py's `run` takes it: a packed or (one in four) planar source, the destination
    depth, the sizes with a crop OR an extension OR neither, the chroma shifts (unlike the source's for u8 only), and what
    source and destination start and stride are off by; every second destination is aligned for 16-byte stores."""
    planar = rng.integers(0, 4) == 0
    dst = DEPTHS[int(rng.integers(0, 3))]
    if planar:
        fmt, src_dtype = None, DEPTHS[int(rng.integers(0, 3))]
        shs, svs = SHIFTS[int(rng.integers(0, 3))]
    else:
        fmt = U.PACKED[int(rng.integers(0, len(U.PACKED)))]
        if fmt == U.AY64 and dst == np.uint8:           # refused: the other two depths
            dst = DEPTHS[int(rng.integers(1, 3))]
        shs, svs = U.NATURAL[fmt][1:]
    hs, vs = (shs, svs)
    if dst == np.uint8 and rng.integers(0, 3) == 0:
        hs, vs = SHIFTS[int(rng.integers(0, 3))]
    w, h = _size(rng, np.dtype(dst).itemsize)
    mode = ("same", "crop", "extend")[int(rng.integers(0, 3))]
    dx, dy = int(rng.integers(0, 41)), int(rng.integers(0, 11))
    if mode == "crop":
        sw, sh = w + dx, h + dy
    elif mode == "extend":
        sw, sh = max(w - dx, 1), max(h - dy, 1)
    else:
        sw, sh = w, h
    if fmt in EVEN_ONLY and sw & 1:
        sw += 1
        if sw > w and sh < h:                           # (the even width became a crop: no extension beside it)
            sh = h
    unit = 2 if fmt == U.AY64 else 1                    # AY64 rows are 2-byte aligned
    p = dict(src=(fmt, sw, sh) if not planar else (src_dtype, shs, svs, sw, sh), dtype=np.dtype(dst), hs=hs, vs=vs, w=w, h=h,
             src_skew=unit * int(rng.choice(OFFSETS)), src_pad=unit * int(rng.choice(OFFSETS)),
             dst_skew=int(rng.choice(OFFSETS)), dst_pad=int(rng.choice(OFFSETS)))
    if rng.integers(0, 2) == 0:
        # the library's condition for 16-byte stores: every destination plane at a 256-byte boundary, its stride the luma
        # row rounded up to 16 bytes (`run` gives the three planes one dst_stride)
        p.update(dst_skew=0, dst_pad=0, dst_stride=-(-w * np.dtype(dst).itemsize // 16) * 16)
    return p


def vector_stores(p):
    """Whether the library stores the picture's whole 16-byte pieces as vectors: the pointers (256-byte boundaries plus
    dst_skew samples, as tests/test_gpu_unpack.py lays them out) and the strides of the three planes multiples of 16."""
    bpp = p["dtype"].itemsize
    strides = [p.get("dst_stride", (U.shifted(p["w"], p["hs"] if k else 0) + p["dst_pad"]) * bpp) for k in range(3)]
    return p["dst_skew"] * bpp % 16 == 0 and all(st % 16 == 0 for st in strides)


def unpack_calls(count=UNPACK_CALLS, seed=2208):
    """Per call: 1 .. 12 pictures."""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        yield [unpack_picture(rng) for _n in range(int(rng.integers(1, 13)))]


def _entries(rng, large=(65, 200)):
    """1 .. 40 entries; one call in six `large`: past one round of the job lookups."""
    if rng.integers(0, 6) == 0:
        return int(rng.integers(large[0], large[1] + 1))
    return int(rng.integers(1, 41))


def _plane_size(rng):
    """Below 300 x 80; one in eight long and thin: up to 2100 along one axis by at most 4 along the other."""
    if rng.integers(0, 8) == 0:
        long, thin = int(rng.integers(300, 2101)), int(rng.integers(1, 5))
        return (long, thin) if rng.integers(0, 2) else (thin, long)
    return int(rng.integers(1, 300)), int(rng.integers(1, 80))


def _pad(rng):
    return 2 * int(rng.choice(OFFSETS)) + (64 if rng.integers(0, 4) == 0 else 0)         # even: s16 strides stay even


def sums_calls(count=STATS_CALLS, seed=2311):
    """Per call: dicts of w, h, dtype (u8 / s16), second (a u8 plane to take the squared error against), pad_a, pad_b, seed."""
    rng = np.random.default_rng(seed)
    for c in range(count):
        out = []
        for n in range(_entries(rng)):
            w, h = _plane_size(rng)
            kind = int(rng.integers(0, 3))
            out.append(dict(w=w, h=h, dtype=np.dtype(np.int16 if kind == 2 else np.uint8), second=kind == 1, pad_a=_pad(rng), pad_b=_pad(rng),
                            seed=10000 * c + n))
        yield out


def lowpass_calls(count=STATS_CALLS, seed=2417):
    """Per call: dicts of w, h, dtype, kind (K.lowpass_input), hs, vs (sigmas of K.SIGMAS, unlike per axis), pad, seed."""
    rng = np.random.default_rng(seed)
    for c in range(count):
        out = []
        for n in range(_entries(rng)):
            w, h = _plane_size(rng)
            dtype = np.dtype((np.uint8, np.int16)[int(rng.integers(0, 2))])
            kinds = ("noise", "steps") if dtype == np.uint8 else ("noise", "steps", "full")
            out.append(dict(w=w, h=h, dtype=dtype, kind=kinds[int(rng.integers(0, len(kinds)))], hs=K.SIGMAS[int(rng.integers(0, 6))],
                            vs=K.SIGMAS[int(rng.integers(0, 6))], pad=_pad(rng), seed=10000 * c + n))
        yield out


def ssim_calls(count=STATS_CALLS, seed=2503):
    """Per call: dicts of w, h, kind (K.ssim_pair), map (whether the picture asks for its map), pad_a, pad_b, map_pad, seed.
    A call takes 64 pictures, whose 2 u8 and 3 s16 low-pass planes are 128 and 192 entries of the low-pass table: the large
    draw is 22 .. 64 pictures."""
    rng = np.random.default_rng(seed)
    for c in range(count):
        out = []
        for n in range(_entries(rng, large=(22, MOST_SSIM_PICTURES))):
            w, h = _plane_size(rng)
            out.append(dict(w=w, h=h, kind=("same", "noisy", "unrelated")[int(rng.integers(0, 3))], map=bool(rng.integers(0, 2)),
                            pad_a=_pad(rng), pad_b=_pad(rng), map_pad=8 * int(rng.integers(0, 4)), seed=10000 * c + n))
        yield out


# ---- a call's planes in one block (a guard_lib.Layout: offsets only, no device) -----------------------------------------

def sums_layout(call):
    """(layout, [(a, b or None, result)]): inputs with an empty footprint, the two result words a call may write."""
    lay, specs = G.Layout(), []
    for n, e in enumerate(call):
        bps = e["dtype"].itemsize
        a = lay.plane(e["h"], e["w"], e["dtype"], stride=e["w"] * bps + e["pad_a"], align=2, footprint=None, name="a%d" % n)
        b = lay.plane(e["h"], e["w"], np.uint8, stride=e["w"] + e["pad_b"], align=1, footprint=None, name="b%d" % n) if e["second"] else None
        specs.append((a, b, lay.span(16, align=8, footprint=("bytes", 16), name="result%d" % n)))
    return lay, specs


def lowpass_layout(call):
    """(layout, [(plane, counter)]): the planes are filtered in place."""
    lay, specs = G.Layout(), []
    for n, e in enumerate(call):
        p = lay.plane(e["h"], e["w"], e["dtype"], stride=e["w"] * e["dtype"].itemsize + e["pad"], align=2, name="plane%d" % n)
        specs.append((p, lay.span(4, align=4, footprint=("bytes", 4), name="counter%d" % n)))
    return lay, specs


def ssim_layout(call):
    """(layout, [(a, b, map or None, scratch, result)]); the map as the doubles' bits, which is how it is compared."""
    lay, specs = G.Layout(), []
    for n, e in enumerate(call):
        w, h = e["w"], e["h"]
        a = lay.plane(h, w, np.uint8, stride=w + e["pad_a"], align=1, footprint=None, name="a%d" % n)
        b = lay.plane(h, w, np.uint8, stride=w + e["pad_b"], align=1, footprint=None, name="b%d" % n)
        nbytes = sa.ssim_scratch_bytes(w, h)
        scratch = lay.span(nbytes, align=16, footprint=("bytes", nbytes), name="scratch%d" % n)
        result = lay.span(32, align=8, footprint=("bytes", 32), name="result%d" % n)
        m = lay.plane(h, w, np.uint64, stride=8 * w + e["map_pad"], align=8, name="map%d" % n) if e["map"] else None
        specs.append((a, b, m, scratch, result))
    return lay, specs


def sums_inputs(e):
    if e["dtype"] == np.int16:
        return K.full_range_s16(e["w"], e["h"], e["seed"]), None
    return K.noise(e["w"], e["h"], np.uint8, e["seed"]), (K.noise(e["w"], e["h"], np.uint8, e["seed"] + 5000) if e["second"] else None)
