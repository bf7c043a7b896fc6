"""Geometries and inputs shared by tests/test_lowdelay_enc_ref.py (CPU) and tests/test_gpu_lowdelay_encode.py."""
import functools

import numpy as np

import lowdelay_enc_ref as R


def params(lw, lh, fmt, depth, nh, nv, num, denom=1, quant_matrix=None):
    """The parameter dict of a lw x lh picture in chroma format fmt (420 / 422 / 444); iwt sizes by schro_params_calculate_iwt_sizes
    (schroparams.c:88-111: rounded up to a multiple of 1 << depth)."""
    cw = lw if fmt == 444 else (lw + 1) // 2
    ch = (lh + 1) // 2 if fmt == 420 else lh
    up = lambda v: (v + (1 << depth) - 1) >> depth << depth
    qm = list(quant_matrix) if quant_matrix is not None else default_matrix(depth)
    return dict(transform_depth=depth, iwt_luma_width=up(lw), iwt_luma_height=up(lh), iwt_chroma_width=up(cw),
                iwt_chroma_height=up(ch), n_horiz_slices=nh, n_vert_slices=nv, slice_bytes_num=num, slice_bytes_denom=denom,
                quant_matrix=qm + [0] * (19 - len(qm)))


def default_matrix(depth):
    """a matrix of the usual shape: finer levels quantised harder (smaller entries: base - entry is larger)"""
    qm = [4 * depth]
    for level in range(depth):
        e = 4 * (depth - 1 - level)
        qm += [e + 2, e + 2, e]
    return qm


def coefficients(P, kind, seed):
    """Three int16 planes of the iwt sizes.  small: wavelet-like, Laplacian within +-4095, the LL band smooth and larger;
    tiny: the same at a scale of 1.5; steps: small with the lower half of every plane doubled (as turns_case scales its
    last rows), so that slice rows of one picture land on unlike indices; full: uniform over all of s16; zero."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(3):
        w, h = (P["iwt_luma_width"], P["iwt_luma_height"]) if c == 0 else (P["iwt_chroma_width"], P["iwt_chroma_height"])
        if kind == "zero":
            a = np.zeros((h, w), np.int16)
        elif kind == "full":
            a = rng.integers(-32768, 32768, (h, w)).astype(np.int16)
            a.reshape(-1)[:4] = (-32768, 32767, -32768, 32767)
        else:
            scale = {"small": 40.0, "steps": 40.0, "tiny": 1.5}[kind]
            a = np.clip(np.rint(rng.laplace(0.0, scale, (h, w))), -4095, 4095).astype(np.int16)
            ll = R.subband(a, 0, P["transform_depth"], w, h)
            ll[...] = np.clip(np.rint(600 + 300 * np.sin(np.arange(ll.shape[1]) / 3.0)[None, :]
                                      + rng.normal(0, 60, ll.shape)), -4095, 4095).astype(np.int16)
            if kind == "steps":
                a[h // 2:] *= 2
        out.append(a)
    return out


# name -> (params, coefficient kind, seed, round trip: None, or why the decoder cannot return the encoder's reconstruction)
WIDE = [8, 6, 6, 4, 6, 6, 4, 6, 6, 4, 5, 5, 4]           # every entry >= 4: base indices 61 .. 64 still differ
DEEP = [70, 60, 60, 66, 50, 50, 55, 40, 40, 45, 30, 30, 35]     # base - matrix below 0 everywhere at first


def _cases():
    c = {}
    for depth in (1, 2, 3, 4):
        for fmt in (420, 422, 444):
            c["64x32_d%d_%d" % (depth, fmt)] = (params(64, 32, fmt, depth, 4, 4, 97, 3), "small", 10 * depth + fmt, None)
    c["128x64_16x8"] = (params(128, 64, 444, 3, 16, 8, 40, 1), "small", 2, None)
    c["128x64_16x8_420"] = (params(128, 64, 420, 3, 16, 8, 33, 2), "small", 3, None)         # empty chroma LL rectangles
    c["72x40_5x3"] = (params(72, 40, 422, 3, 5, 3, 700, 3), "small", 4, None)
    c["one_slice"] = (params(64, 64, 420, 2, 1, 1, 2500, 1), "small", 5, None)
    c["one_slice_444_d1"] = (params(64, 64, 444, 1, 1, 1, 9001, 2), "small", 6, None)
    c["below_zero"] = (params(64, 32, 422, 4, 4, 4, 200, 1, DEEP), "small", 7, None)
    c["full_range"] = (params(64, 32, 420, 3, 4, 4, 1500, 7), "full", 8, None)         # indices 41 .. 43
    c["full_range_big_budget"] = (params(64, 32, 422, 2, 4, 4, 3000, 1), "full", 9, "LL differences wrap")
    c["length_field"] = (params(64, 32, 422, 2, 4, 4, 63, 2), "small", 12, "the fast decoder sizes slice_y_length from the short slice")
    c["zero"] = (params(64, 32, 420, 3, 4, 4, 16, 1), "zero", 0, None)
    c["overrun"] = (params(64, 32, 420, 2, 4, 4, 5, 2), "full", 11, "over-run slices")
    # the serial launch off LDS (leaves_lds below) with more than one thread: 32 x 32 LL rectangles per component on a diagonal
    # of two slices; 3 x 5 slices of a 68 x 56 / 34 x 28 LL band, widths 22 23 23 / 11 11 12, heights 11 11 12 11 11 / 5 6 6 5 6
    c["spill_2x2"] = (params(128, 128, 444, 1, 2, 2, 9217, 3), "steps", 13, None)
    c["spill_3x5_420"] = (params(272, 224, 420, 2, 3, 5, 15001, 4), "steps", 14, None)
    return c


CASES = _cases()
SPILL_BATCH = ("spill_2x2", (("small", 43), ("full", 44), ("zero", 0)))       # geometry, the unlike pictures of one call


REFUSED_CASE = "64x32_d3_420"


def refused_params(P):
    """What tests/test_gpu_lowdelay_encode.py::test_refusals changes in the parameters of REFUSED_CASE: (the word the
    message holds, the parameters).  The last two are what the kernels index with int: the LL bands of a picture (depth 0:
    the planes themselves) above 2^28 samples, one slice's LL samples above 2^20."""
    return [("chroma LL", dict(P, iwt_chroma_width=P["iwt_chroma_width"] + 8)),
            ("slice_bytes_denom", dict(P, slice_bytes_denom=0)),
            ("slice_bytes_denom", dict(P, slice_bytes_denom=-3)),
            ("LL bands", dict(P, transform_depth=0, iwt_luma_width=32767, iwt_luma_height=32767, iwt_chroma_width=16384,
                              iwt_chroma_height=16384)),
            ("LL rectangles", dict(P, transform_depth=0, iwt_luma_width=8192, iwt_luma_height=8192, iwt_chroma_width=4096,
                                   iwt_chroma_height=4096, n_horiz_slices=1, n_vert_slices=1))]


def per_thread_samples(P):
    """What a thread of the serial launch keeps, in samples: plane_lowdelay_enc.cpp:88-103 (EncChooseLayout) -- per
    component the largest LL rectangle, the row above it from one sample to the left, the column to its left; and the
    row being reconstructed."""
    depth, nh, nv = P["transform_depth"], P["n_horiz_slices"], P["n_vert_slices"]
    at = bw_max = 0
    for c in range(3):
        w = (P["iwt_chroma_width"] if c else P["iwt_luma_width"]) >> depth
        h = (P["iwt_chroma_height"] if c else P["iwt_luma_height"]) >> depth
        bw, bh = -(-w // nh), -(-h // nv)
        at += bw * bh + bw + 1 + bh
        bw_max = max(bw_max, bw)
    return at + bw_max


def leaves_lds(P):
    """plane_lowdelay_enc.cpp:104-113: the launch keeps the samples in LDS while 64 threads' worth of them (int16) fit
    48 KB -- 384 samples per thread; beyond that they go to the queue's scratch, element k of thread t at k * T + t."""
    return per_thread_samples(P) * 2 * 64 > 48 << 10


def span_case():
    """One picture whose slices differ wildly in content against one budget, and a matrix with a wide spread: the chosen
    indices span 0 .. 64."""
    P = params(128, 64, 444, 4, 8, 8, 600, 7, WIDE)
    planes = coefficients(P, "full", 21)
    for p in planes:
        for i in range(13):
            band = R.subband(p, i, 4, 128, 64)
            for k in range(64):
                # slice k keeps values of about 2^(k / 3.7): from all zero to full range
                lim = int(2 ** (k / 3.7)) - 1 if k < 60 else 32767
                x0, x1, y0, y1 = R.codeblock(band.shape[1], band.shape[0], k % 8, k // 8, 8, 8)
                band[y0:y1, x0:x1] = np.clip(band[y0:y1, x0:x1], -lim, lim)
    return P, planes


def turns_case():
    """A picture whose anti-diagonals hold more slices than the serial launch has threads, so that a thread takes several
    slices of a diagonal in turns.  The launch has a thread per slice of the longest diagonal unless a thread's samples
    (its LL rectangles, sized for the largest of the picture, the row above and the column to the left) limit what 48 KB of
    LDS hold: 68 x 66 slices of a 69 x 1321 LL band (depth 1, 4:4:4) have rectangles of up to 2 x 21 samples, 200 int16 per
    thread, so 64 threads serve diagonals of up to 66 slices.  Most rectangles are 1 x 20, which keeps the checker quick;
    the two bottom rows of slices, the ones taken in the second turn, carry doubled values and need the whole search."""
    P = params(138, 2642, 444, 1, 68, 66, 1040, 3)
    planes = coefficients(P, "small", 33)
    first = 2 * ((P["iwt_luma_height"] // 2) * 64 // 66)
    for p in planes:
        p[first:] *= 2
    return P, planes


@functools.lru_cache(maxsize=None)
def expected(name):
    """(P, planes, the checker's result) of a case: computed once, shared, never modified"""
    if name == "span":
        P, planes = span_case()
    elif name == "large":
        P = params(960, 540, 422, 3, 30, 68, 97, 2)
        planes = coefficients(P, "small", 31)
    elif name == "turns":
        P, planes = turns_case()
    else:
        P, kind, seed, _ = CASES[name]
        planes = coefficients(P, kind, seed)
    traces = []
    res = R.encode(planes, P, traces)
    res["traces"] = traces
    for a in planes + res["recon"] + [res["bytes"], res["index"]]:
        a.setflags(write=False)
    return P, planes, res


def _one_slice_estimates(seed, index):
    """A one-slice 32 x 32 4:2:0 picture of tiny coefficients: (P without a budget, planes, the bits of its values at base
    index `index` without the header)."""
    P = params(32, 32, 420, 2, 1, 1, 8, 1, [4, 2, 2, 0, 2, 2, 0])
    planes = coefficients(P, "small" if index else "tiny", seed)
    enc = R._Encoder(planes, P)
    n, _ = R._Slice(enc, 0, 0, 1).estimate(index)
    return P, planes, n - 7 - R.ilog2up(8)


@functools.lru_cache(maxsize=None)
def exact_fit(index):
    """The two exact fits of schro_encoder_pick_slice_index, built from the checker's own estimate: a budget that the
    estimate at `index` (0: the first test, <=, stays at 0; 32: the first probe of the loop, >=, moves up) meets to the
    bit.  Returns (P, planes, result)."""
    for seed in range(400):
        P, planes, body = _one_slice_estimates(seed, index)
        for nbytes in range(1, 1 << 14):
            if 7 + R.ilog2up(8 * nbytes) + body == 8 * nbytes:
                P = dict(P, slice_bytes_num=nbytes)
                traces = []
                res = R.encode(planes, P, traces)
                if (index, 8 * nbytes) in traces[0] and (index == 0 or traces[0][0][1] > 8 * nbytes):
                    res["traces"] = traces
                    return P, planes, res
    raise AssertionError("no exact fit found")
