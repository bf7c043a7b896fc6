"""The cases of tests/test_gpu_encoder_pipeline.py: which cases of the encoder's stages are enqueued in which order, the
scratch each of them needs, and what every call must leave.  Nothing is restated here: the inputs and the expected values
are the cached ones of the stages' own case modules (subpel_cases, split2_cases, mode_cases, hier_bm_cases,
noarith_enc_cases, noarith_dec_cases, motion_enc_cases, lowdelay_enc_cases, quant_cases) and of the rough chain of tests/test_gpu_rough_hint.py, whose
witnesses the CPU walks of those modules assert.

The scratch needs are the formulas of schroedinger_amd/csrc/plane_*.cpp.  The plane-layer batch call takes its tables
from the START of the queue's grow-only block (`batch_need`; 0 where the call takes none: the block matching and the
rough search keep everything in the caller's fields).  The frame-layer run sizes the block for those tables and, BEHIND
them, the fields and outputs it copies in and out (`frame_need`; the frame-layer runs of the entropy coders, of the VLC
decoder and of the motion-data encoder allocate their inputs and outputs elsewhere and need what their batch call needs).  A sequence is (A, B, C): A small, B at least four times A -- the
block is reallocated behind A's launches --, C smaller than B and unlike A -- its tables lie on what B left.
tests/test_encoder_pipeline_cases.py asserts that order, so that a changed case cannot make a sequence monotone without a
failure."""
import functools

import numpy as np

import hier_bm_cases as HK
import lowdelay_enc_cases as LC
import mode_cases as MC
import motion_enc_cases as ME
import noarith_dec_cases as DC
import noarith_enc_cases as NC
import quant_cases as QC
import split2_cases as S2
import subpel_cases as SP

MV_BYTES = 20                   # a SchroMotionVector
SUBPEL_ENTRY = 8 * 4            # plane_subpel.cpp: eight int32 errors per record
SPLIT2_ENTRY = 16 * 4           # SCHRO_HIP_SPLIT2_TABLE_INTS int32 per record
MODE_ENTRY = 532 * 4            # SCHRO_HIP_MODE_TABLE_INTS int32 per superblock
SB_BYTES, TRIAL_BYTES = 16, 4 * 24
CHAIN_LEVELS = 2                # the pyramid levels of the block-matching and rough chains here


def round_up(n, m=256):
    return -(-n // m) * m


def records(c):
    return c["nbx"] * c["nby"]


# ---- the motion stages with tables ------------------------------------------------------------------------------------

def _subpel_batch_need(c):
    return round_up(records(c) * SUBPEL_ENTRY) if c["prec"] > 0 else 0


def _subpel_frame_need(c):
    # subpel_host_run, one chain: the tables, the fields behind them, 256
    return round_up(records(c) * SUBPEL_ENTRY) + round_up(records(c) * MV_BYTES) + 256


def _split2_batch_need(c):
    return round_up(records(c) * SPLIT2_ENTRY)


def _split2_frame_need(c):
    n = records(c)
    return round_up(n * SPLIT2_ENTRY) + 3 * round_up(n * MV_BYTES) + round_up(n // 16 * SB_BYTES + 8) + 256


def _mode_batch_need(c):
    return round_up(records(c) * SPLIT2_ENTRY) + round_up(records(c) // 16 * MODE_ENTRY)


def _mode_frame_need(c):
    n = records(c)
    return _mode_batch_need(c) + 7 * round_up(n * MV_BYTES) + round_up(n // 16 * SB_BYTES + 8) + round_up(n // 16 * TRIAL_BYTES + 8) + 512


def _subpel_outputs(name):
    return {"field": SP.expected(name)[0]}


def _subpel_error_outputs(name):
    return {"table": SP.expected(name)[1][0]}


def _subpel_choose_outputs(name):
    return {"field": SP.fields_by_pass(name)[1]}


def _split2_outputs(name):
    motion, sb = S2.expected(name)[:2]
    return {"motion": motion, "superblocks": sb}


MODE_OUTPUTS = ("motion", "superblocks", "trials", "stats")


def _mode_outputs(name):
    return dict(zip(MODE_OUTPUTS, MC.expected(name)[:4]))


# ---- the chains of the block matching and of the rough search: a case is a picture size ------------------------------

def _size(name):
    w, h = name.split("x")
    return int(w), int(h)


CHAIN_REF_INDEX = {"40x30": 0, "101x75": 1, "64x48": 0}


def hbm_case(name):
    w, h = _size(name)
    P = HK.chain_params(w, h)
    return dict(w=w, h=h, nbx=P["x_num_blocks"], nby=P["y_num_blocks"], ref_index=CHAIN_REF_INDEX[name], ext=HK.CHAIN_EXT, params=P)


def rough_params(w, h, xb=8, yb=8):
    """(the blocks of the full picture as tests/test_gpu_rough_hint.py lays them out)"""
    return dict(x_num_blocks=-(-w // xb), y_num_blocks=-(-h // yb), xbsep_luma=xb, ybsep_luma=yb)


def rough_case(name):
    w, h = _size(name)
    P = rough_params(w, h)
    return dict(w=w, h=h, nbx=P["x_num_blocks"], nby=P["y_num_blocks"], ref_index=CHAIN_REF_INDEX[name], ext=0, params=P)


class _Lazy(dict):
    """{name: case} made on demand"""

    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, name):
        self[name] = self.make(name)
        return self[name]


def _chain_frame_need(c):
    # hbm_host_run / rough_me_host_run: a slot per level (and one more: level 0, or the hint)
    return round_up(records(c) * MV_BYTES) * (CHAIN_LEVELS + 1)


def _hbm_outputs(name):
    c = hbm_case(name)
    fields = HK.chain_reference(c["w"], c["h"], CHAIN_LEVELS, c["ref_index"])[0]
    return {"level%d" % k: fields[k] for k in range(CHAIN_LEVELS + 1)}


@functools.lru_cache(maxsize=None)
def rough_chain(name):
    """(frame, ref, the fields by level) of the rough chain: tests/rough_hint_ref.rough_scan on analysis_ref.pyramid."""
    import analysis_ref as A
    import rough_hint_cases as RH
    import rough_hint_ref as RR
    c = rough_case(name)
    frame = RH.texture(c["w"], c["h"], 7000 + c["w"])
    ref = RH.moved(frame, 5, -3, 7001 + c["w"])
    fields = RR.rough_scan(A.pyramid(frame, CHAIN_LEVELS), A.pyramid(ref, CHAIN_LEVELS), c["params"], CHAIN_LEVELS, c["ref_index"], c["ext"])
    return frame, ref, fields


def _rough_outputs(name):
    fields = rough_chain(name)[2]
    return {"level%d" % k: fields[k] for k in range(1, CHAIN_LEVELS + 1)}


# ---- the two entropy coders ---------------------------------------------------------------------------------------------

def _noarith_need(case):
    # plane_noarith_enc.cpp: three words per row piece of a codeblock, four per codeblock, two per sub-band
    pieces = cbs = 0
    for k in range(3):
        for i in range(case.nsub):
            hc, vc = case.counts(i)
            pieces += case.band(k, i).shape[0] * hc
            cbs += hc * vc
    return (3 * pieces + 4 * cbs + 2 * 3 * case.nsub) * 4


def _noarith_outputs(name):
    data, bits, stats = NC.BY_NAME[name].expected()
    return {"bytes": np.frombuffer(data, np.uint8), "subband_bits": np.asarray(bits)}


def _lowdelay_need(case):
    # plane_lowdelay_enc.cpp: the estimate's table and the reconstructed LL bands (these cases keep the serial launch in LDS)
    P = case[0]
    d = P["transform_depth"]
    r16 = lambda n: round_up(n, 16)
    ll = (P["iwt_luma_width"] >> d) * (P["iwt_luma_height"] >> d) + 2 * (P["iwt_chroma_width"] >> d) * (P["iwt_chroma_height"] >> d)
    return r16(P["n_horiz_slices"] * P["n_vert_slices"] * 130 * 4) + r16(ll * 2)


def _lowdelay_outputs(name):
    res = LC.expected(name)[2]
    return {"slices": res["bytes"], "index": res["index"], "count": np.array([res["count"]], np.uint32)}


# ---- the VLC decoder and the motion-data encoder ----------------------------------------------------------------------------

ND_RESULT_WORDS = 9 + 3 * 19 + 15       # SchroHipNoarithDecodeResult: nine counters, 3 x 19 lengths, 3 x 19 index bytes and padding
ME_SB_WORDS, ME_SECTIONS = 32, 9        # kMeSbWords, kMeSections (schro_hip_internal.h)


def _noarith_dec_need(case):
    # plane_noarith_dec.cpp: five words per chunk slot (data_bytes / 8 + sub-bands + 1), three per codeblock, eight per
    # sub-band, two per picture
    nsb = 3 * case.nsub
    ncb = 3 * sum(case.counts(i)[0] * case.counts(i)[1] for i in range(case.nsub))
    return (5 * (case.data_bytes // 8 + nsb + 1) + 3 * ncb + 8 * nsb + 2) * 4


def noarith_dec_result_words(result):
    """A result dict of tests/noarith_dec_ref.py (or of sa.noarith_decode_result) as the words of the device's block."""
    head = [result[k] for k in ("bytes_read", "error", "first_error", "compat_quant_offset", "truncated", "not_consumed", "overran",
                                "long_codes", "clamped_quant")]
    index = np.zeros(4 * 15, np.uint8)
    index[:3 * 19] = np.asarray(result["subband_quant_index"]).ravel()
    words = np.concatenate([np.array(head, np.uint32), np.asarray(result["subband_length"]).ravel().astype(np.uint32), index.view(np.uint32)])
    assert words.size == ND_RESULT_WORDS
    return words


def _noarith_dec_outputs(name):
    coeffs, quant, result = DC.BY_NAME[name].expected()
    flat = lambda planes: np.concatenate([p.ravel() for p in planes])
    return {"coeffs": flat(coeffs), "quant": flat(quant), "result": noarith_dec_result_words(result)}


@functools.lru_cache(maxsize=None)
def _motion_cases():
    return {c[0]: c for c in ME.all_cases()}


def _motion_enc_need(case):
    # plane_motion_enc.cpp: kMeSbWords words per superblock, each section's header bits and length per picture
    name, field, nbx, nby, num_refs, hg, _ = case
    return (nbx * nby // 16 * ME_SB_WORDS + 2 * ME_SECTIONS) * 4


@functools.lru_cache(maxsize=None)
def motion_enc_expected(name):
    """(bytes, result) of tests/motion_enc_ref.py, once per case"""
    import motion_enc_ref as MR
    return MR.encode(*_motion_cases()[name][1:6])


def _motion_enc_outputs(name):
    data, result = motion_enc_expected(name)
    return {"bytes": np.frombuffer(data, np.uint8), "sections": np.array(result["section_bytes"], np.int64)}


# ---- the quantiser: three unlike planes of the codeblock-geometry case ------------------------------------------------

QUANT_SPECS = {"88x72_inter": 0, "44x40_intra": 3, "two_codeblocks": 5}


@functools.lru_cache(maxsize=None)
def quant_spec(name):
    return QC.geometry_specs(np.int16, seed=11)[QUANT_SPECS[name]]


@functools.lru_cache(maxsize=None)
def _quant_expected(name):
    return QC.expected(quant_spec(name))


def _quant_outputs(name):
    q, r, s = _quant_expected(name)
    return {"quant": q, "recon": r, "summary": s}


# stage: its cases, (A, B, C), the two needs, {output: expected array} of a case
STAGES = {
    "rough": dict(cases=_Lazy(rough_case), sequence=("40x30", "101x75", "64x48"), batch_need=lambda c: 0, frame_need=_chain_frame_need,
                  outputs=_rough_outputs),
    "hbm": dict(cases=_Lazy(hbm_case), sequence=("40x30", "101x75", "64x48"), batch_need=lambda c: 0, frame_need=_chain_frame_need,
                outputs=_hbm_outputs),
    "subpel": dict(cases=SP.CASES, sequence=("block_32x32", "block_4x4", "padded_stride"), batch_need=_subpel_batch_need,
                   frame_need=_subpel_frame_need, outputs=_subpel_outputs),
    "split2": dict(cases=S2.CASES, sequence=("tiny", "block_4x4", "padded_stride"), batch_need=_split2_batch_need,
                   frame_need=_split2_frame_need, outputs=_split2_outputs),
    "mode": dict(cases=MC.CASES, sequence=("block_32x32", "clipped_padded", "one_reference"), batch_need=_mode_batch_need,
                 frame_need=_mode_frame_need, outputs=_mode_outputs),
    "noarith": dict(cases=NC.BY_NAME, sequence=("s16-16x8-d2-three-m1", "s16-grid-1026", "s16-32x16-d3-two-m0"), batch_need=_noarith_need,
                    frame_need=_noarith_need, outputs=_noarith_outputs),
    "lowdelay": dict(cases=LC.CASES, sequence=("64x32_d3_420", "128x64_16x8_420", "72x40_5x3"), batch_need=_lowdelay_need,
                     frame_need=_lowdelay_need, outputs=_lowdelay_outputs),
    # the decoder's C after B is the one to watch: its chunk and codeblock records lie on what B's 1027 chunks left
    "noarith_dec": dict(cases=DC.BY_NAME, sequence=("s16-16x8-420-d2-three-m1-c1", "s16-chain-two-steps", "s16-32x16-420-d3-two-m0-c0"),
                        batch_need=_noarith_dec_need, frame_need=_noarith_dec_need, outputs=_noarith_dec_outputs),
    "motion_enc": dict(cases=_Lazy(lambda name: _motion_cases()[name]),
                       sequence=("4x4 split 2 refs 2", "132x68: three superblocks per layout thread", "12x12 mixed refs 2"),
                       batch_need=_motion_enc_need, frame_need=_motion_enc_need, outputs=_motion_enc_outputs),
}
# what only the nine calls run: the single launches of the sub-pel stage -- pass 1 of each case, from the field and the table
# the restatement has there -- and the quantiser, which takes no scratch
LAUNCHES = {
    "subpel_error": dict(STAGES["subpel"], outputs=_subpel_error_outputs),
    "subpel_choose": dict(STAGES["subpel"], outputs=_subpel_choose_outputs),
    "quantise": dict(cases=_Lazy(quant_spec), sequence=tuple(QUANT_SPECS), outputs=_quant_outputs),
}
SCRATCH_STAGES = ("rough", "hbm", "subpel", "split2", "mode", "noarith", "lowdelay", "noarith_dec", "motion_enc")
NINE_CALL_STAGES = ("subpel_error", "subpel_choose", "subpel", "split2", "mode", "hbm", "quantise", "noarith_dec", "motion_enc")
BIG_TABLES = 4                  # SchroHipContext::kBigTables: the pinned mirrors and device buffers of a queue, used in turn
NINE = 2 * BIG_TABLES + 1


def stage(name):
    return STAGES[name] if name in STAGES else LAUNCHES[name]


def case(stage_name, name):
    return stage(stage_name)["cases"][name]


def needs(stage_name):
    """[(batch need, frame-layer need)] of A, B, C."""
    s = stage(stage_name)
    return [(s["batch_need"](s["cases"][n]), s["frame_need"](s["cases"][n])) for n in s["sequence"]]


def outputs(stage_name, name):
    return stage(stage_name)["outputs"](name)


# ---- the orders of the calls --------------------------------------------------------------------------------------------

FRAME = "frame"                 # the frame-layer entry point, synchronous


def scratch_sequence(stage_name, both_queues):
    """[(queue, case name, layer)]: A, B, C through the plane layer without a wait, A through the frame layer, B through
    the plane layer behind it -- on queue 1, or every step on queue 0 and then on queue 1 so that the two blocks go through
    the same history."""
    a, b, c = stage(stage_name)["sequence"]
    steps = [(a, "plane"), (b, "plane"), (c, "plane"), (a, FRAME), (b, "plane")]
    queues = (0, 1) if both_queues else (1,)
    return [(q, name, layer) for name, layer in steps for q in queues]


def nine_calls(stage_name, both_queues):
    """[(queue, case name)]: NINE calls that cycle through A, B, C -- call k + 4, which takes call k's table buffer, carries
    another table -- on queue 0, or dealt alternately to queues 0 and 1."""
    seq = stage(stage_name)["sequence"]
    return [(k % 2 if both_queues else 0, seq[k % 3]) for k in range(NINE)]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.tobytes() == b.tobytes()


# ---- the inter chain: original pictures in, stream bytes out ----------------------------------------------------------
#
# A chain picture has two references and goes through: the downsample pyramid of the picture and of both references
# (CHAIN_PYRAMID levels), the block matching with its level-0 pass, the sub-pel refinement of its level-0 fields, the mode
# decision on the sub-pel fields and the level-1 and level-2 fields, the prediction of the motion field it leaves, the
# residual, its wavelet coefficients, the quantiser and the noarith bytes.  Every stage function below takes what the
# stage before it left and calls that stage's own restatement or oracle; `chain_expected` strings them together, so the
# expected value of a stage is computed from the EXPECTED output of the one before and the first stage that differs on the
# device is the one named.  The extension of a picture is its block separation: the smallest every stage takes.

CHAIN_PYRAMID, CHAIN_DEPTH, CHAIN_FILT = 3, 2, 1
CHAIN_MOTIONS = ((3, -2), (-2, 1))      # what the two references are moved by, luma samples
CHAIN_FORMATS = {420: (1, 1), 422: (1, 0), 444: (0, 0)}
FILL = 0x5a                     # the fill pattern a stage's output is replaced by in the dependency witness
CHAIN_PICTURES = {
    "64x48_420": dict(w=64, h=48, fmt=420, xbsep=8, xblen=12, prec=2, hc=[1, 2, 3], vc=[1, 2, 2], mode=1, seed=11, lam=0.1, noise=3,
                      qi=([3, 5, 6, 8, 10, 11, 14], [6, 3, 0, 4, 9, 12, 15], [7, 8, 2, 0, 3, 13, 18])),
    "80x56_422": dict(w=80, h=56, fmt=422, xbsep=16, xblen=24, prec=1, hc=[1, 1, 2], vc=[1, 2, 2], mode=0, seed=12, lam=0.1, noise=3,
                      qi=([2, 3, 0, 9, 5, 7, 12], [4, 7, 3, 12, 8, 6, 10], [0, 5, 8, 14, 9, 4, 11])),
    "80x56_422_again": dict(w=80, h=56, fmt=422, xbsep=16, xblen=24, prec=1, hc=[1, 1, 2], vc=[1, 2, 2], mode=0, seed=13, lam=0.1, noise=3,
                            qi=([5, 3, 4, 9, 6, 7, 11], [4, 8, 3, 10, 8, 6, 12], [1, 5, 7, 13, 9, 4, 10])),
}
CHAIN_PAIR = ("64x48_420", "80x56_422")                         # the two unlike pictures of every batch call
CHAIN_PIPELINE = ("80x56_422", "64x48_420", "80x56_422_again")  # three deep: the middle one has the larger grid


def chain_geometry(name):
    """What the calls take of a chain picture: sizes, block and motion parameters, codeblock records."""
    import synth
    d = CHAIN_PICTURES[name]
    hs, vs = CHAIN_FORMATS[d["fmt"]]
    dims = [(d["h"], d["w"])] + [((d["h"] + vs) >> vs, (d["w"] + hs) >> hs)] * 2
    u = 1 << CHAIN_DEPTH
    blocks = HK.chain_params(d["w"], d["h"], d["xbsep"], d["xbsep"])
    motion = synth.motion_params(d["w"], d["h"], d["xblen"], d["xbsep"], d["prec"], (1, 1, 1), (hs, vs))
    assert (motion["x_num_blocks"], motion["y_num_blocks"]) == (blocks["x_num_blocks"], blocks["y_num_blocks"])
    return dict(d, name=name, shifts=(hs, vs), dims=dims, iwt=[(-(-h // u) * u, -(-w // u) * u) for h, w in dims], ext=d["xbsep"], blocks=blocks,
                mode_params=dict(blocks, mv_precision=d["prec"], h_shift=hs, v_shift=vs), motion_params=motion,
                nbx=blocks["x_num_blocks"], nby=blocks["y_num_blocks"])


def chain_records(g, k, stride):
    """the codeblock records [dst_offset, dst_stride, width, height, quant_index] of component k in a plane of that stride:
    one quant index per sub-band"""
    ih, iw = g["iwt"][k]
    recs = QC.layout(iw, ih, CHAIN_DEPTH, g["hc"], g["vc"], stride, 2)
    bands = []
    for i in range(1 + 3 * CHAIN_DEPTH):
        level = 0 if i == 0 else (i - 1) // 3 + 1
        bands += [i] * (g["hc"][level] * g["vc"][level])
    assert len(bands) == len(recs)
    for r, b in zip(recs, bands):
        r[4] = g["qi"][k][b]
    return recs


@functools.lru_cache(maxsize=None)
def chain_inputs(name):
    """((Y, U, V) of the picture, per reference (Y, U, V)); read-only."""
    import rough_hint_cases as RH
    g = chain_geometry(name)
    hs, vs = g["shifts"]
    frame = tuple(RH.texture(w, h, g["seed"] * 100 + 10 * k) for k, (h, w) in enumerate(g["dims"]))
    refs = tuple(tuple(RH.moved(p, mx >> (hs if k else 0), my >> (vs if k else 0), g["seed"] * 100 + 50 * r + k + 1, noise=g["noise"])
                       for k, p in enumerate(frame))
                 for r, (mx, my) in enumerate(CHAIN_MOTIONS))
    for a in frame + refs[0] + refs[1]:
        a.setflags(write=False)
    return frame, refs


def stage_pyramid(g, planes):
    """[level][component] of one picture: level 0 the picture itself"""
    import hier_bm_ref as HR
    return HR.pyramid3(planes, CHAIN_PYRAMID)


def stage_hbm(g, frame_pyramid, ref_pyramids):
    """[reference][level] fields"""
    import hier_bm_ref as HR
    hs, vs = g["shifts"]
    return [HR.hbm_scan(frame_pyramid, ref_pyramids[r], g["blocks"], CHAIN_PYRAMID, r, hs, vs, g["ext"], with_level0=True) for r in (0, 1)]


def stage_subpel(g, frame, refs, level0):
    import subpel_ref as SR
    return [SR.subpel_deep(frame[0], refs[r][0], g["blocks"], g["prec"], r, g["lam"], level0[r], g["ext"])[0] for r in (0, 1)]


def stage_mode(g, frame, refs, sub, level1, level2, table=False):
    """(motion, superblocks, trials, statistics); table: the mode table the metric launches leave in the scratch instead"""
    import mode_ref as MR
    out = MR.mode_decision(list(frame), [list(r) for r in refs], g["mode_params"], g["lam"], sub, level1, level2, g["ext"])
    return out[5] if table else out[:4]


def stage_prediction(g, motion, refs):
    """the prediction - 128 of every component, s16"""
    import oracle_lib as O
    out = []
    for k, (h, w) in enumerate(g["dims"]):
        u1, u2 = (O.UpComp(r[k], upsample=True) for r in refs)
        acc = O.motion_render(motion, O.MotionParams(**g["motion_params"]), k, u1, u2, np.zeros((h, w), np.int16), w, h, return_acc=True)[1]
        out.append(O.rrshift6_s16(acc))
    return out


def chain_source(g, frame):
    """the picture - 128 at the transform's size, zero beyond the picture: what the residual planes hold before the subtraction"""
    out = []
    for k, (h, w) in enumerate(g["dims"]):
        s = np.zeros(g["iwt"][k], np.int16)
        s[:h, :w] = frame[k].astype(np.int16) - 128
        out.append(s)
    return out


def stage_residual(g, source, prediction):
    import quant_ref as Q
    return [Q.subtract(s, p) for s, p in zip(source, prediction)]


def stage_coefficients(g, residual):
    import oracle_lib as O
    return [O.forward_iwt(r, CHAIN_DEPTH, CHAIN_FILT) for r in residual]


def stage_quantise(g, coeffs):
    """per component (quantised values, reconstruction, summaries)"""
    import quant_ref as Q
    out = []
    for k, c in enumerate(coeffs):
        q, r, s = Q.quantise_plane(c, chain_records(g, k, c.shape[1] * 2), 0, 0, None)
        out.append((q, r, np.array(s, np.uint32).reshape(-1, 2)))
    return out


def stage_bytes(g, quant):
    """(bytes, subband_bits, stats)"""
    import noarith_enc_ref as NR
    return NR.encode_transform_data(list(quant), CHAIN_DEPTH, g["hc"], g["vc"], g["mode"], g["qi"])


@functools.lru_cache(maxsize=None)
def chain_expected(name):
    """{stage: what it leaves} of a chain picture, each from the expected output of the stage before; read-only."""
    g = chain_geometry(name)
    frame, refs = chain_inputs(name)
    e = dict(geometry=g, frame=frame, refs=refs)
    e["frame_pyramid"] = stage_pyramid(g, frame)
    e["ref_pyramids"] = [stage_pyramid(g, r) for r in refs]
    e["hbm"] = stage_hbm(g, e["frame_pyramid"], e["ref_pyramids"])
    e["subpel"] = stage_subpel(g, frame, refs, [e["hbm"][r][0] for r in (0, 1)])
    e["mode"] = stage_mode(g, frame, refs, e["subpel"], [e["hbm"][r][1] for r in (0, 1)], [e["hbm"][r][2] for r in (0, 1)])
    e["prediction"] = stage_prediction(g, e["mode"][0], refs)
    e["source"] = chain_source(g, frame)
    e["residual"] = stage_residual(g, e["source"], e["prediction"])
    e["coefficients"] = stage_coefficients(g, e["residual"])
    e["quantise"] = stage_quantise(g, e["coefficients"])
    e["bytes"] = stage_bytes(g, [q for q, _, _ in e["quantise"]])
    return e


def chain_decoded(g, data):
    """The round trip of tests/test_gpu_noarith_encode.py::test_chain_quantise_encode_decode_dequantise on the host: the
    restated noarith decoder on the bytes, then the oracle's dequantisation of every codeblock with the quant index the
    stream carries.  Returns (quant planes, reconstruction planes, bytes read)."""
    import noarith_enc_ref as NR
    import oracle_lib as O
    got_q, indices, used = NR.decode_transform_data(bytes(data), list(g["iwt"]), np.int16, CHAIN_DEPTH, g["hc"], g["vc"], g["mode"])
    recon = []
    for k, (ih, iw) in enumerate(g["iwt"]):
        out = np.zeros((ih, iw), np.int16)
        for i in range(1 + 3 * CHAIN_DEPTH):
            hc, vc = NR.codeblock_counts(i, g["hc"], g["vc"])
            for y in range(vc):
                for x in range(hc):
                    qi = int(indices[k][i][y, x]) if indices[k][i] is not None else 0
                    src = NR.get_codeblock(NR.subband(got_q[k], CHAIN_DEPTH, i), x, y, hc, vc)
                    dst = NR.get_codeblock(NR.subband(out, CHAIN_DEPTH, i), x, y, hc, vc)
                    O.dequant_codeblock(dst, np.ascontiguousarray(src), qi, False, 0)
        recon.append(out)
    return got_q, recon, used


def filled(a):
    """an array like `a` that holds the fill pattern"""
    return np.frombuffer(bytes([FILL]) * a.nbytes, a.dtype).reshape(a.shape).copy()


def chain_dependencies(name):
    """[(producer, consumer, the consumer's expected output, its output when the producer's is replaced)]: a plane is
    replaced by the fill pattern, a field by the field-set record of tests/hier_bm_ref.py.

    The level-1 and level-2 fields of the block matching are hints of the mode decision's split-1 and split-0 trials.  In a
    true chain the sub-pel fields descend from the same search and a coarser hint does not beat them: on these pictures the
    motion field, the sums and the statistics are the same whatever the two coarser fields hold (at a lambda small enough
    for a level-1 hint to win, 0.002, every block comes out as one mode of one split, which is a poorer picture for every
    later stage).  What does change with either field is the mode table -- every candidate's error, which the metric launches
    leave in the scratch and the walk reads -- so for these two joins the witness is the restated table, not the outputs."""
    import hier_bm_ref as HR
    e = chain_expected(name)
    g, frame, refs = e["geometry"], e["frame"], e["refs"]
    n = g["nbx"] * g["nby"]
    level = lambda k: [e["hbm"][r][k] for r in (0, 1)]
    unset = lambda split: [HR.field_set(n, split, r + 1) for r in (0, 1)]
    table = stage_mode(g, frame, refs, e["subpel"], level(1), level(2), table=True)
    flat_pyramid = [e["frame_pyramid"][0]] + [tuple(filled(p) for p in lv) for lv in e["frame_pyramid"][1:]]
    out = [("pyramid", "hbm", e["hbm"], stage_hbm(g, flat_pyramid, e["ref_pyramids"])),
           ("hbm level 0", "subpel", e["subpel"], stage_subpel(g, frame, refs, unset(2))),
           ("hbm level 1", "mode table", table, stage_mode(g, frame, refs, e["subpel"], unset(1), level(2), table=True)),
           ("hbm level 2", "mode table", table, stage_mode(g, frame, refs, e["subpel"], level(1), unset(0), table=True)),
           ("subpel", "mode", e["mode"], stage_mode(g, frame, refs, unset(2), level(1), level(2))),
           ("mode", "prediction", e["prediction"], stage_prediction(g, HR.field_set(n, 2, 1), refs)),
           ("prediction", "residual", e["residual"], stage_residual(g, e["source"], [filled(p) for p in e["prediction"]])),
           ("residual", "coefficients", e["coefficients"], stage_coefficients(g, [filled(p) for p in e["residual"]])),
           ("coefficients", "quantise", e["quantise"], stage_quantise(g, [filled(p) for p in e["coefficients"]])),
           ("quantise", "bytes", e["bytes"][:2], stage_bytes(g, [filled(q) for q, _, _ in e["quantise"]])[:2])]
    return out


def flatten(x):
    """the bytes of a stage's output: arrays, bytes and nested lists of them"""
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x).tobytes()
    return b"".join(flatten(v) for v in x)
