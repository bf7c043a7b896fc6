"""The draws of the encoder loop's tests (tests/test_gpu_encode_loop.py) and their expected values, CPU only: what
schro_encoder_render_picture -> quantise -> schro_encoder_reconstruct_picture (schroencoder.c:2430-2460, :2692-2726) leave
behind for a three-picture group, composed from the existing checkers in the reference's order, and what the product's
decoder path makes of the same quantised values.  tests/test_encode_loop_draws.py walks the draws without a device.

A draw is a group of three pictures: picture 0 intra, picture 1 inter with one reference (the reconstruction of picture
0), picture 2 inter with two (the reconstructions of pictures 0 and 1; picture_weight_1 = _2 = 1, picture_weight_bits =
1).  Per picture and component, in the reference's order:

  src        the u8 picture - 128 in an s16 plane of the iwt size, zero outside the picture
  pred       (inter) oracle_lib.motion_render's accumulator through oracle_lib.rrshift6_s16: the prediction - 128
  residual   quant_ref.subtract (src, pred)
  coeffs     oracle_lib.forward_iwt
  counts     hist_ref.counts per sub-band (picture 0: the DC form on sub-band 0)
  quant, recon, summaries   quant_ref.quantise_plane (picture 0 with the intra LL recurrence)
  enc_sum, enc_u8   the encoder side: oracle_lib.inverse_iwt (recon), frame_add of pred, convert_u8
  blob, drecs       the hand-over: the quantised values as tight row-major codeblocks (quant_cases.tight_values)
  dec_coeffs, dec_res, dec_u8   the decoder side from blob alone: oracle_lib.dequant_codeblock (+ dc_predict for
             picture 0), inverse_iwt, then motion_render with that residual (inter) or convert_u8 (picture 0)

Eight draws are named; seeded ones come on top (8 x SCHRO_FUZZ_SCALE, seeds shifted by SCHRO_FUZZ_SEED, as in
tests/test_gpu_encoder_fuzz.py).  `vectors_from_the_search` takes picture 1's vectors from the rough search's level-1
field (rough_hint_ref.rough_scan over analysis_ref.pyramid of picture 1's luma and of the reconstructed picture 0's),
all 20 bytes of every record, the records off the level's grid included."""
import functools

import numpy as np

import analysis_ref as A
import hist_cases as HC
import hist_ref as H
import oracle_lib as O
import quant_cases as QC
import quant_ref as Q
import rough_hint_cases as RC
import rough_hint_ref as R
import synth

CHROMA = {420: (1, 1), 422: (1, 0), 444: (0, 0)}
MODES = (0.2, 0.3, 0.2, 0.3)    # DC, reference 1, reference 2, both: the mix of the OBMC tests
SEARCH_LEVELS = 2
N_SEEDED = 8                    # at SCHRO_FUZZ_SCALE = 1


def _draw(w, h, fmt, filt, depth, prec, blk, hc, vc, qi, seed, style="texture", move=(2, -1), mv_range=6, vectors="synth"):
    assert w <= 128 and h <= 96 and len(hc) == len(vc) == depth + 1 and all(len(q) == 1 + 3 * depth for q in qi) and len(qi) == 3
    return dict(w=w, h=h, fmt=fmt, filt=filt, depth=depth, prec=prec, blk=blk, hc=list(hc), vc=list(vc), qi=[list(q) for q in qi],
                seed=seed, style=style, move=move, mv_range=mv_range, vectors=vectors)


# quant indices per sub-band (0 .. 3 * depth) for pictures 0, 1, 2: every form of DESIGN 4.9 in bands other than the LL
# band -- index 0, index 3, multiples of 4, other indices up to 8 and above
QI3 = ([4, 6, 7, 8, 9, 10, 12, 13, 15, 17], [5, 0, 3, 8, 7, 9, 12, 14, 16, 21], [8, 3, 5, 0, 6, 11, 12, 13, 17, 20])
QI2 = ([3, 5, 6, 8, 10, 11, 14], [6, 3, 0, 4, 9, 12, 15], [7, 8, 2, 0, 3, 13, 18])
QI1 = ([2, 3, 0, 9], [4, 7, 3, 12], [0, 5, 8, 14])
COARSE2 = ([22, 26, 26, 30, 31, 33, 36], [24, 27, 28, 29, 32, 34, 37], [25, 26, 28, 30, 33, 35, 38])

NAMED = {
    # sizes that are no multiple of 1 << depth in either direction: the zero padding and the crop matter (luma 128 x 96,
    # chroma 64 x 48 of 62 x 46: the frame layer's draw -- the chroma transform is the luma one halved)
    "dd97_420_depth3_padded": _draw(124, 92, 420, 0, 3, 2, (12, 8), [1, 1, 2, 3], [1, 1, 2, 2], QI3, 11),
    "legall_422_depth2": _draw(96, 64, 422, 1, 2, 1, (12, 8), [1, 2, 3], [1, 1, 2], QI2, 12),
    "dd137_444_depth1_padded": _draw(101, 75, 444, 2, 1, 3, (16, 8), [2, 3], [1, 2], QI1, 13),
    "haar0_420_depth3": _draw(128, 96, 420, 3, 3, 0, (16, 12), [1, 1, 1, 4], [1, 1, 1, 3], QI3, 14),
    "haar1_422_depth2_padded": _draw(90, 70, 422, 4, 2, 2, (8, 4), [1, 1, 2], [1, 2, 2], QI2, 15),
    "fidelity_444_depth2": _draw(64, 48, 444, 5, 2, 0, (12, 8), [1, 1, 2], [1, 1, 2], QI2, 16),
    # bright and dark, high contrast, coarse indices: the sums leave 0 .. 255 on both sides and both conversions saturate
    "daub97_420_saturating": _draw(118, 86, 420, 6, 2, 1, (12, 8), [1, 2, 2], [1, 1, 2], COARSE2, 17, style="contrast"),
    "vectors_from_the_search": _draw(128, 96, 420, 1, 2, 0, (8, 8), [1, 2, 2], [1, 1, 2], QI2, 18, move=(3, -2), vectors="search"),
}
COMBINE_FORM = ("dd97_420_depth3_padded", "legall_422_depth2")      # one of them with padding
FRAME_LAYER = "dd97_420_depth3_padded"


def seeded(n, seed_shift=0):
    """draw n of the seeded ones: every member random, indices of every form"""
    rng = np.random.default_rng(4200 + n + 1000 * seed_shift)
    filt, depth = int(rng.integers(0, 7)), int(rng.integers(1, 4))
    if filt == 5:
        depth = min(depth, 2)   # the fidelity filter does not shift: a third level takes coefficients past 4095 (test_range)
    w, h = int(rng.integers(40, 129)), int(rng.integers(32, 97))
    fmt = (420, 422, 444)[int(rng.integers(0, 3))]
    blk = [(8, 4), (12, 8), (16, 12), (16, 8), (8, 8)][int(rng.integers(0, 5))]
    hc = [1] + [int(rng.integers(1, 2 + l)) for l in range(1, depth + 1)]
    vc = [1] + [int(rng.integers(1, 2 + l)) for l in range(1, depth + 1)]
    qi = [[int(v) for v in np.sort(rng.integers(0, 22, 1 + 3 * depth))] for _ in range(3)]
    return _draw(w, h, fmt, filt, depth, int(rng.integers(0, 4)), blk, hc, vc, qi, 500 + n + 1000 * seed_shift,
                 move=(int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), mv_range=int(rng.integers(2, 12)))


def names(scale=1, seed_shift=0):
    return list(NAMED) + ["seeded_%d_%d" % (seed_shift, n) for n in range(N_SEEDED * scale)]


def get(name):
    if name in NAMED:
        return NAMED[name]
    _, shift, n = name.split("_")
    return seeded(int(n), int(shift))


# ---- geometry -------------------------------------------------------------------------------------------------------

def dims(d):
    """(height, width) of the three components of a picture"""
    hs, vs = CHROMA[d["fmt"]]
    c = (-(-d["h"] // (1 << vs)), -(-d["w"] // (1 << hs)))
    return [(d["h"], d["w"]), c, c]


def iwt_dims(d):
    """... and of their transforms (schro_params_calculate_iwt_sizes: each rounded up to 1 << depth)"""
    u = 1 << d["depth"]
    return [(-(-h // u) * u, -(-w // u) * u) for h, w in dims(d)]


def padded(d):
    return [a != b for a, b in zip(dims(d), iwt_dims(d))]


def motion_params(d):
    return synth.motion_params(d["w"], d["h"], d["blk"][0], d["blk"][1], d["prec"], (1, 1, 1), CHROMA[d["fmt"]])


def band_of_record(d):
    """the sub-band index of every record of schro_hip_codeblock_layout's order"""
    out = []
    for i in range(1 + 3 * d["depth"]):
        level = 0 if i == 0 else (i - 1) // 3 + 1
        out += [i] * (d["hc"][level] * d["vc"][level])
    return out


def records(d, n, k, stride):
    """the codeblock records [dst_offset, dst_stride, width, height, quant_index] of component k of picture n in a plane
    whose rows are `stride` bytes apart"""
    ih, iw = iwt_dims(d)[k]
    recs = QC.layout(iw, ih, d["depth"], d["hc"], d["vc"], stride, 2)
    bands = band_of_record(d)
    assert len(recs) == len(bands) and all(r[2] > 0 and r[3] > 0 for r in recs), (d, k)
    for r, b in zip(recs, bands):
        r[4] = d["qi"][n][b]
    return recs


def dc_of(d, n, k):
    """(dc_predict_first, dc_width, dc_height) of picture 0's planes, None for the inter pictures"""
    ih, iw = iwt_dims(d)[k]
    return (d["hc"][0] * d["vc"][0], iw >> d["depth"], ih >> d["depth"]) if n == 0 else None


def hist_bands(d, n, k, stride):
    ih, iw = iwt_dims(d)[k]
    return [H.band_rect(iw, ih, d["depth"], i, stride, 2) + (H.band_skip(i), int(n == 0 and i == 0)) for i in range(1 + 3 * d["depth"])]


# ---- inputs ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pictures(name):
    """[picture][component] u8: rough_hint_cases.texture moved by a few samples from picture to picture, noise added"""
    d = get(name)
    out = []
    first = []
    for k, (h, w) in enumerate(dims(d)):
        p = RC.texture(w, h, d["seed"] * 10 + k)
        if d["style"] == "contrast":
            p = np.clip((p.astype(np.int32) - 128) * 8 + 128, 0, 255).astype(np.uint8)
        first.append(p)
    for n in range(3):
        hs, vs = CHROMA[d["fmt"]]
        pic = []
        for k, p in enumerate(first):
            dx, dy = (d["move"][0] * n, d["move"][1] * n) if k == 0 else ((d["move"][0] * n) >> hs, (d["move"][1] * n) >> vs)
            q = RC.moved(p, dx, dy, d["seed"] * 100 + 10 * n + k, noise=3) if n else p
            q.setflags(write=False)
            pic.append(q)
        out.append(pic)
    return out


def synth_vectors(d, n):
    P = motion_params(d)
    modes = MODES if n == 2 else (MODES[0], sum(MODES[1:]), 0, 0)
    return synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], d["mv_range"] << d["prec"], d["seed"] * 7 + n, modes)


def search_params(d):
    P = motion_params(d)
    return {k: P[k] for k in ("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma")}


def search_field(d, frame, ref):
    """the level-1 field of the chain search of luma `frame` in luma `ref`, as it is"""
    assert d["prec"] == 0 and d["blk"] == (8, 8)
    return R.rough_scan(A.pyramid(frame, SEARCH_LEVELS), A.pyramid(ref, SEARCH_LEVELS), search_params(d), SEARCH_LEVELS, 0, 0)[1]


# ---- the stages (functions of their own: a test that wants to see the loop fail replaces one) ---------------------------

def source(d, pic, k):
    (h, w), (ih, iw) = dims(d)[k], iwt_dims(d)[k]
    s = np.zeros((ih, iw), np.int16)
    s[:h, :w] = pic[k].astype(np.int16) - 128
    return s


def upcomps(d, refs, k):
    return [O.UpComp(r[k], upsample=d["prec"] > 0) for r in refs] + [None] * (2 - len(refs))


def prediction(d, mv, k, refs):
    """the prediction - 128 of component k, s16, the picture's size"""
    h, w = dims(d)[k]
    u1, u2 = upcomps(d, refs, k)
    acc = O.motion_render(mv, O.MotionParams(**motion_params(d)), k, u1, u2, np.zeros((h, w), np.int16), w, h, return_acc=True)[1]
    return O.rrshift6_s16(acc)


def decoder_records(d, n, k, quant, recs):
    """(blob, records) of the hand-over: tight row-major codeblocks of two-byte values"""
    return QC.tight_values(quant, recs, 2)


def references(pics, recons, n):
    """the pictures picture n is predicted from: the RECONSTRUCTIONS of the pictures before it"""
    return recons[:n]


def dequantise(d, n, k, blob, drecs):
    ih, iw = iwt_dims(d)[k]
    out = np.zeros((ih, iw), np.int16)
    vals = np.ascontiguousarray(blob).view(np.uint8)
    for (o, st, w, h, off, size, qi) in drecs:
        assert size == 2 and o % 2 == 0 and st % 2 == 0
        view = np.lib.stride_tricks.as_strided(out.reshape(-1)[o // 2:], shape=(h, w), strides=(st, 2))
        O.dequant_codeblock(view, vals[off:off + 2 * w * h].view(np.int16).reshape(h, w), qi, n == 0, 0)
    if n == 0:
        ll = H.band_view(out, d["depth"], 0)
        ll[...] = O.dc_predict(np.ascontiguousarray(ll))
    return out


def code_picture(d, n, pic, refs, mv):
    """every stage's value for the three components of one picture: a list of dicts"""
    comps = []
    for k in range(3):
        (h, w), (ih, iw) = dims(d)[k], iwt_dims(d)[k]
        c = dict(src=source(d, pic, k))
        if refs:
            c["pred"] = prediction(d, mv, k, refs)
            c["residual"] = Q.subtract(c["src"], c["pred"])
        else:
            c["pred"], c["residual"] = None, c["src"]
        c["coeffs"] = O.forward_iwt(c["residual"], d["depth"], d["filt"])
        recs, dc = records(d, n, k, iw * 2), dc_of(d, n, k)
        c["counts"] = np.stack([H.counts(HC.band_array(c["coeffs"], b), b[4], bool(b[5])) for b in hist_bands(d, n, k, iw * 2)])
        c["quant"], c["recon"], summ = Q.quantise_plane(c["coeffs"], recs, n == 0, dc[0] if dc else 0, dc[1:] if dc else None)
        c["summaries"] = np.array(summ, np.uint32).reshape(-1, 2)
        # the encoder's local decode
        c["enc_res"] = O.inverse_iwt(c["recon"], d["depth"], d["filt"])
        c["enc_sum"] = O.frame_add(c["enc_res"], c["pred"]) if refs else c["enc_res"]
        c["enc_u8"] = O.convert_u8(c["enc_sum"], w, h)
        # the decoder, from the quantised values alone
        c["blob"], c["drecs"] = decoder_records(d, n, k, c["quant"], recs)
        c["dec_coeffs"] = dequantise(d, n, k, c["blob"], c["drecs"])
        c["dec_res"] = O.inverse_iwt(c["dec_coeffs"], d["depth"], d["filt"])
        if refs:
            u1, u2 = upcomps(d, refs, k)
            c["dec_u8"] = O.motion_render(mv, O.MotionParams(**motion_params(d)), k, u1, u2, c["dec_res"], w, h)
        else:
            c["dec_u8"] = O.convert_u8(c["dec_res"], w, h)
        comps.append(c)
    return comps


def code_group(name, refs_of=None):
    """[picture] of (components, vectors): the group coded with whatever `references` (or refs_of) hands each picture"""
    d, pics = get(name), pictures(name)
    out, recons = [], []
    for n in range(3):
        refs = (refs_of or references)(pics, recons, n)
        mv = None
        if n:
            mv = search_field(d, pics[n][0], refs[0][0]) if (d["vectors"] == "search" and n == 1) else synth_vectors(d, n)
        comps = code_picture(d, n, pics[n], refs, mv)
        out.append((comps, mv))
        recons.append([c["enc_u8"] for c in comps])
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """code_group (name), computed once per draw and process; read-only"""
    group = code_group(name)
    for comps, mv in group:
        for c in comps:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        if mv is not None:
            mv.setflags(write=False)
    return group
