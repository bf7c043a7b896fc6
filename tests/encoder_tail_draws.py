"""The seeded draws of the encoder tail's random-geometry tests, as generators that need no device: the low-delay slice
encoder's pictures (tests/test_gpu_encoder_fuzz.py), the quantiser's codeblock planes and the histogram's bands (the
same file) and the intra chain's pictures (tests/test_gpu_encode_chain.py).  tests/dry_run_encoder_tail_cases.py walks
them on the CPU and asserts that they cover what the tests' docstrings promise.

Every draw is a dict with a `tag`: what an assertion message carries."""
import numpy as np

import hist_cases as HC
import hist_ref as H
import lowdelay_enc_cases as K
import lowdelay_enc_ref as R
import oracle_lib as O
import quant_cases as QC

FORMATS = (420, 422, 444)
MAX_SLICES = 160                # per picture: the Python checker takes about 2.5 ms a slice


def refused_for_chroma_ll(P):
    """the library's refusal (include/schro_hip.h, lowdelay_encode_batch): the chroma LL band is not the luma LL band in the
    frame's chroma format, so the reference's chroma rectangles, cut from its reconstructed frame, would diverge"""
    d = P["transform_depth"]
    hs, vs = int(P["iwt_chroma_width"] < P["iwt_luma_width"]), int(P["iwt_chroma_height"] < P["iwt_luma_height"])
    llw, llh = P["iwt_luma_width"] >> d, P["iwt_luma_height"] >> d
    return ((llw + hs) >> hs, (llh + vs) >> vs) != (P["iwt_chroma_width"] >> d, P["iwt_chroma_height"] >> d)


def geometry(rng, depth, fmt, max_w, max_h, min_w=8, min_h=8):
    """a luma size from 8 x 8 whose rounded iwt sizes the library takes (others are redrawn, not skipped)"""
    while True:
        lw, lh = int(rng.integers(min_w, max_w + 1)), int(rng.integers(min_h, max_h + 1))
        if not refused_for_chroma_ll(K.params(lw, lh, fmt, depth, 1, 1, 1)):
            return lw, lh


def samples(P):
    return P["iwt_luma_width"] * P["iwt_luma_height"] + 2 * P["iwt_chroma_width"] * P["iwt_chroma_height"]


def slice_bytes(rng, P, nslices, bits_per_sample):
    """slice_bytes_num / slice_bytes_denom for about bits_per_sample: denominators 1 .. 7, and one above 1 does not divide
    the numerator (the running remainder is live)"""
    denom = int(rng.integers(1, 8))
    num = max(denom, int(samples(P) * bits_per_sample / 8 / nslices * denom))
    if denom > 1 and num % denom == 0:
        num += int(rng.integers(1, denom))
    return num, denom


def empty_ll_rectangles(P):
    """some slice has no LL sample in some component"""
    d = P["transform_depth"]
    return (min(P["iwt_luma_width"], P["iwt_chroma_width"]) >> d < P["n_horiz_slices"]
            or min(P["iwt_luma_height"], P["iwt_chroma_height"]) >> d < P["n_vert_slices"])


def length_field_class(P):
    """lowdelay_enc_cases.CASES["length_field"]: on the fast decoder's geometries, slices of n and n + 1 bytes whose bit
    counts differ in bit length -- the decoder sizes slice_y_length from the short slice, the encoder per slice"""
    sizes = set(R.slice_sizes(P))
    return O.lowdelay_arith(P, 2) == O.LOWDELAY_FAST16 and len(set(R.ilog2up(8 * n) for n in sizes)) > 1


# ---- B: the low-delay slice encoder ------------------------------------------------------------------------------------

KINDS = ("small", "tiny", "full", "zero")


def lowdelay_draws(scale=1, seed=0, count=40):
    """count x scale calls: depth 1 .. 4; 4:2:0 / 4:2:2 / 4:4:4; luma 8 x 8 .. 160 x 96 (rounded to the iwt sizes); slice
    counts from 1 to beyond the LL band's width and height (empty LL rectangles), at most 160 slices; a budget of
    0.1 .. 8 bits per sample as a fraction; the default matrix, WIDE, DEEP or random entries 0 .. 70; 1 .. 3 pictures of
    kinds small / tiny / full / zero; plane strides padded by 0 .. 64 even bytes; the slice buffer 0 .. 3 bytes off a word.
    Every eighth draw is 1 .. 2 x 1 .. 2 slices of a depth-1 picture of at least 96 x 64: LL rectangles of 24 x 16 and more,
    which the serial launch keeps in the queue's scratch (lowdelay_enc_cases.leaves_lds); the others mostly stay in LDS.
    Over-run draws are draws like any other."""
    rng = np.random.default_rng(1605 + seed)
    for rnd in range(count * scale):
        depth, fmt = int(rng.integers(1, 5)), FORMATS[int(rng.integers(0, 3))]
        if rnd % 8 == 7:
            depth = 1
            lw, lh = geometry(rng, depth, fmt, 160, 96, 96, 64)
            nh, nv = int(rng.integers(1, 3)), int(rng.integers(1, 3))
        else:
            lw, lh = geometry(rng, depth, fmt, 160, 96)
            P0 = K.params(lw, lh, fmt, depth, 1, 1, 1)
            llw, llh = P0["iwt_luma_width"] >> depth, P0["iwt_luma_height"] >> depth
            nh = int(rng.integers(1, min(llw + 3, 24) + 1))
            nv = int(rng.integers(1, min(llh + 3, 16, MAX_SLICES // nh) + 1))
        P0 = K.params(lw, lh, fmt, depth, 1, 1, 1)
        num, denom = slice_bytes(rng, P0, nh * nv, float(np.exp(rng.uniform(np.log(0.1), np.log(8.0)))))
        which = int(rng.integers(0, 4))
        n = 1 + 3 * depth
        matrix = [None, K.WIDE[:n], K.DEEP[:n], [int(v) for v in rng.integers(0, 71, n)]][which]
        P = K.params(lw, lh, fmt, depth, nh, nv, num, denom, matrix)
        kinds = [(KINDS[int(rng.integers(0, 4))], int(rng.integers(1, 1 << 20))) for _ in range(int(rng.integers(1, 4)))]
        pads = tuple(2 * int(v) for v in rng.integers(0, 33, 3))
        skew = int(rng.integers(0, 4))
        yield dict(P=P, kinds=kinds, pads=pads, skew=skew, fmt=fmt,
                   tag=("draw", rnd, fmt, "depth", depth, (lw, lh), "slices", (nh, nv), "bytes", (num, denom),
                        ("default", "WIDE", "DEEP", "random")[which], kinds, "pads", pads, "skew", skew))


def lowdelay_pictures(draw):
    return [K.coefficients(draw["P"], kind, seed) for kind, seed in draw["kinds"]]


# ---- C: the quantiser and the histograms -------------------------------------------------------------------------------

def quantise_draws(scale=1, seed=0, count=40):
    """count x scale calls of 1 .. 6 planes: s16 / s32; intra / inter; depth 1 .. 4; planes from one LL sample (2^depth a
    side, multiples of it or not) up to 200 x 120; 1 .. 5 codeblocks a side per level (schro_hip_codeblock_layout; never
    more than the band has samples: empty records are refused); pitches of an odd number of samples; every codeblock an
    index of its own, 0 .. 60, walked from a shuffled cycle so that a draw of 61 codeblocks holds every index;
    quant_cases.values for the data.  Intra planes send their LL band through the DC kernel, and one intra plane in
    four has an LL band whose shorter side is 1."""
    rng = np.random.default_rng(1706 + seed)
    for rnd in range(count * scale):
        dtype = (np.int16, np.int32)[int(rng.integers(0, 2))]
        b = np.dtype(dtype).itemsize
        specs, shapes = [], []
        for _ in range(int(rng.integers(1, 7))):
            depth, intra = int(rng.integers(1, 5)), int(rng.integers(0, 2))
            unit = 1 << depth
            w, h = int(rng.integers(unit, 201)), int(rng.integers(unit, 121))
            if intra and rng.integers(0, 4) == 0:           # a DC band 1 wide or 1 high
                if rng.integers(0, 2):
                    w = unit + int(rng.integers(0, unit))
                else:
                    h = unit + int(rng.integers(0, unit))
            pitch = (w + int(rng.integers(0, 6))) | 1
            hc, vc = [], []
            for level in range(depth + 1):
                shift = depth - max(level - 1, 0)           # entry 0: the LL band; entry l: the bands of level l - 1
                hc.append(int(rng.integers(1, min(5, w >> shift) + 1)))
                vc.append(int(rng.integers(1, min(5, h >> shift) + 1)))
            recs = QC.layout(w, h, depth, hc, vc, pitch * b, b)
            assert all(r[2] > 0 and r[3] > 0 for r in recs)
            cycle = rng.permutation(61)
            for n, r in enumerate(recs):
                r[4] = int(cycle[n % 61])
            spec = dict(buf=QC.values(rng, (h, pitch), dtype), records=recs, intra=intra)
            if intra:
                spec["dc"] = (hc[0] * vc[0], w >> depth, h >> depth)
            specs.append(spec)
            shapes.append((w, h, pitch, depth, "intra" if intra else "inter", hc, vc))
        yield dict(specs=specs, tag=("draw", rnd, np.dtype(dtype).name, shapes))


CONSTANTS = (0, 1, 2, 3, -3, 5, 100, -32768)        # bins 0 .. 3 are kept in registers, the others in LDS; -32768 overflows


def histogram_draws(scale=1, seed=0, count=60):
    """count x scale calls of 1 .. 8 planes: s16 / s32; every non-empty sub-band (hist_ref.band_rect) of depth 1 .. 4
    transforms of pictures 2 x 2 .. 200 x 120 -- bands 1 wide or 1 high among them --, each with the reference's
    band_skip; sub-band 0 in the DC form for about half the planes; odd pitches; hist_cases.coefficients for the data,
    and in one call of five planes whose samples are all equal: every lane of every wave meets in one bin."""
    rng = np.random.default_rng(1807 + seed)
    for rnd in range(count * scale):
        dtype = (np.int16, np.int32)[int(rng.integers(0, 2))]
        b = np.dtype(dtype).itemsize
        equal = rnd % 5 == 4
        specs, shapes = [], []
        for _ in range(int(rng.integers(1, 9))):
            while True:
                depth = int(rng.integers(1, 5))
                w, h = int(rng.integers(2, 201)), int(rng.integers(2, 121))
                pitch = (w + int(rng.integers(0, 6))) | 1
                dc = int(rng.integers(0, 2))
                bands = []
                for i in range(1 + 3 * depth):
                    off, stride, bw, bh = H.band_rect(w, h, depth, i, pitch * b, b)
                    if bw > 0 and bh > 0:
                        bands.append((off, stride, bw, bh, H.band_skip(i), int(dc and i == 0)))
                if bands:                   # (a 2 x 2 picture has bands at depth 1 only)
                    break
            if equal:
                buf = np.full((h, pitch), CONSTANTS[int(rng.integers(0, len(CONSTANTS)))], dtype)
            else:
                buf = HC.coefficients(rng, (h, pitch), dtype)
            specs.append(dict(buf=buf, bands=bands))
            shapes.append((w, h, pitch, depth, "dc" if dc else "plain", int(buf[0, 0]) if equal else "mixed"))
        yield dict(specs=specs, equal=equal, tag=("draw", rnd, np.dtype(dtype).name, shapes))


# ---- D: the intra chain ------------------------------------------------------------------------------------------------

FILTERS = tuple(range(7))       # what schro_hip_iwt_batch takes (tests/test_gpu_iwt_forward.py)
# (filter, depth, format, luma size, slices, bytes): one whose serial launch stays in LDS, one that leaves it
CHAIN_FIXED = ((0, 3, 420, (64, 32), (4, 4), (97, 3)), (1, 1, 444, (128, 128), (2, 2), (9217, 3)))


def chain_draws(scale=1, seed=0, count=10):
    """The two fixed geometries, then count x scale draws: every filter in turn, depth 1 .. 3, the three chroma formats,
    luma up to 128 x 96, 1 .. 6 x 1 .. 6 slices, a budget of 1 .. 3 bits per sample, destination strides padded by
    0 .. 64 even bytes.  `decodes` is False where no decoder returns the encoder's reconstruction -- the length_field class;
    a draw with over-run slices is the other such class, known once the checker has run."""
    rng = np.random.default_rng(1908 + seed)
    for rnd in range(len(CHAIN_FIXED) + count * scale):
        if rnd < len(CHAIN_FIXED):
            filt, depth, fmt, (lw, lh), (nh, nv), (num, denom) = CHAIN_FIXED[rnd]
            P = K.params(lw, lh, fmt, depth, nh, nv, num, denom)
        else:
            filt, depth, fmt = FILTERS[(rnd - len(CHAIN_FIXED)) % len(FILTERS)], int(rng.integers(1, 4)), FORMATS[int(rng.integers(0, 3))]
            lw, lh = geometry(rng, depth, fmt, 128, 96)
            nh, nv = int(rng.integers(1, 7)), int(rng.integers(1, 7))
            P0 = K.params(lw, lh, fmt, depth, nh, nv, 1)
            num, denom = slice_bytes(rng, P0, nh * nv, float(rng.uniform(1.0, 3.0)))
            P = K.params(lw, lh, fmt, depth, nh, nv, num, denom)
        pads = tuple(2 * int(v) for v in rng.integers(0, 33, 3))
        seeds = [int(v) for v in rng.integers(1, 1 << 20, 3)]
        yield dict(P=P, filt=filt, depth=depth, fmt=fmt, pads=pads, seeds=seeds, decodes=not length_field_class(P),
                   tag=("draw", rnd, "filter", filt, "depth", depth, fmt, (lw, lh), "slices", (nh, nv), "bytes", (num, denom),
                        "pads", pads, "seeds", seeds))


def chain_pictures(draw, pixel_range):
    """the three pixel-range pictures of a chain draw, of the iwt sizes (pixel_range: test_gpu_iwt_forward's)"""
    P = draw["P"]
    sizes = [(P["iwt_luma_height"], P["iwt_luma_width"])] + [(P["iwt_chroma_height"], P["iwt_chroma_width"])] * 2
    return [pixel_range(h, w, np.int16, s) for (h, w), s in zip(sizes, draw["seeds"])]


def chain_expected(draw, pictures):
    """(coefficients, the checker's result, the decoded pictures or None): oracle_lib's forward transform, the slice
    checker on its coefficients, and -- where a decoder returns the encoder's reconstruction -- oracle_lib's slice decoder
    and inverse transform of the checker's bytes"""
    P, depth, filt = draw["P"], draw["depth"], draw["filt"]
    coeffs = [O.forward_iwt(p, depth, filt) for p in pictures]
    res = R.encode(coeffs, P)
    if not draw["decodes"] or res["count"]:
        return coeffs, res, None, None
    planes = [np.zeros_like(c) for c in coeffs]
    O.lowdelay_decode(res["bytes"], planes, P)
    return coeffs, res, planes, [O.inverse_iwt(p, depth, filt) for p in planes]


CHAIN_SKIP_CAP = 5              # at most one draw in five may leave the decode half out
