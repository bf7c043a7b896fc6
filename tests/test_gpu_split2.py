"""GPU: the split-2 level of the mode decision on the device (mode_split2.hip) against tests/split2_ref.py: the metric
table entry for entry, all 20 bytes of every motion record, and the superblock table with its score compared as bits.

Every picture, field, table and output of every test lies in a guarded block (tests/guard_lib.py): a byte written outside
an output, or an input changed, fails the test that did it.  The upsampled images are made by upsample_batch outside the
block and compared with themselves afterwards."""
import zlib

import numpy as np
import pytest

import guard_lib as G
import hier_bm_cases as HK
import oracle_lib as O
import schroedinger_amd as sa
import split2_cases as K
import split2_ref as R
import subpel_ref as S
import synth
from schroedinger_amd import frames
from test_gpu_hier_bm import device_pyramid, free_pyramid

pytestmark = pytest.mark.gpu

MV = sa.MV_DTYPE.itemsize
ENTRY = 4 * sa.SPLIT2_TABLE_INTS
SB = sa.SB_DTYPE.itemsize


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(1, -1)


def records(c):
    return c["nbx"] * c["nby"]


def shifts(c):
    return K.FORMATS[c["fmt"]]


class Rig:
    """Some (case, source planes, reference planes) entries in one guarded block: per entry the three source planes (stride
    width + pad), the fields, the table, the motion field and the superblock table -- and, outside the block, the
    upsampled images of every component of every reference."""

    def __init__(self, ctx, entries, written, seed):
        self.ctx, self.entries = ctx, entries
        lay = G.Layout()
        self.src, self.sp = [], []
        for n, (c, src, refs) in enumerate(entries):
            self.src.append([lay.plane(p.shape[0], p.shape[1], np.uint8, stride=p.shape[1] + c["pad"], footprint=None, name="src%d_%d" % (n, k),
                                       align=64, skew=(c["pad"] + n + k) % 4) for k, p in enumerate(src)])
            sizes = {"field0": records(c) * MV, "field1": records(c) * MV, "table": records(c) * ENTRY, "motion": records(c) * MV,
                     "superblocks": records(c) // 16 * SB}
            self.sp.append({nm: lay.span(size, footprint=("bytes", size) if nm in written else None, name="%s%d" % (nm, n), align=64,
                                         skew=(8 if nm == "superblocks" else 4) * ((n + len(nm)) % 3)) for nm, size in sizes.items()})
        self.block = G.GuardedBlock(ctx, lay, seed=seed)
        self.hp, self.tmp = [], []
        for n, (c, src, refs) in enumerate(entries):
            for k, p in enumerate(src):
                self.block[self.src[n][k]].upload(p)
            ups = []
            for r in refs:
                ups.append([])
                for p in r:
                    d, hp = ctx.upload(p), ctx.hp_plane(*p.shape)
                    ctx.upsample_batch([(d, hp)])
                    ups[-1].append(hp)
                    self.tmp.append(d)
            self.hp.append(ups)
        ctx.synchronize()
        self.hp_before = [[[hp.download() for hp in r] for r in ups] for ups in self.hp]

    def span(self, n, name):
        return self.block[self.sp[n][name]]

    def put(self, n, name, a):
        self.span(n, name).upload(as_bytes(a))

    def put_fields(self, n, fields):
        for r, f in enumerate(fields):
            self.put(n, "field%d" % r, f)

    def picture(self, n, lam=None):
        c, _, refs = self.entries[n]
        return ([self.block[s] for s in self.src[n]], self.hp[n], shifts(c), c["ext"], K.params_of(c), c["lam"] if lam is None else lam,
                [self.span(n, "field%d" % r) for r in range(len(refs))], self.span(n, "motion"), self.span(n, "superblocks"))

    def check(self, expected):
        """expected: {(n, name): array}; whatever is not named keeps what it held."""
        extra = ["upsampled image %d.%d.%d changed" % (n, r, k) for n, ups in enumerate(self.hp) for r, ref in enumerate(ups) for k, hp in enumerate(ref)
                 if not np.array_equal(hp.download(), self.hp_before[n][r][k])]
        self.block.check({self.sp[n][nm]: as_bytes(a) for (n, nm), a in expected.items()}, extra=extra)

    def free(self):
        self.block.free()
        for p in [hp for ups in self.hp for r in ups for hp in r] + self.tmp:
            p.free()


def case_entry(name):
    src, refs, _ = K.inputs(name)
    return K.CASES[name], src, refs


def seed_of(name, k=0):
    return k + (zlib.crc32(name.encode()) & 0xfff0)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_metric_launch(ctx, name):
    """The table entry for entry -- the markers of the blocks outside the picture and of the reference a picture does not
    have included -- and the fields, the motion field and the superblock table left as they were."""
    motion, sb, table, _ = K.expected(name)
    rig = Rig(ctx, [case_entry(name)], ("table",), seed=seed_of(name))
    try:
        rig.put_fields(0, K.inputs(name)[2])
        ctx.split2_metric_batch([rig.picture(0)], [rig.span(0, "table")])
        ctx.synchronize()
        rig.check({(0, "table"): table})
    finally:
        rig.free()


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_choice_launch(ctx, name):
    """From the restatement's table: all 20 bytes of every motion record and the superblock table, the score as bits; the
    table and the fields are left alone."""
    motion, sb, table, _ = K.expected(name)
    rig = Rig(ctx, [case_entry(name)], ("motion", "superblocks"), seed=seed_of(name, 1))
    try:
        rig.put_fields(0, K.inputs(name)[2])
        rig.put(0, "table", table)
        ctx.split2_choose_batch([rig.picture(0)], [rig.span(0, "table")])
        ctx.synchronize()
        rig.check({(0, "motion"): motion, (0, "superblocks"): sb})
    finally:
        rig.free()


def run_stage(ctx, entries, fields, want, seed):
    """schro_hip_split2_batch over the entries in one call."""
    rig = Rig(ctx, entries, ("motion", "superblocks"), seed=seed)
    try:
        for n, f in enumerate(fields):
            rig.put_fields(n, f)
        ctx.split2_batch([rig.picture(n) for n in range(len(entries))])
        ctx.synchronize()
        expected = {}
        for n, (motion, sb) in enumerate(want):
            expected[n, "motion"], expected[n, "superblocks"] = motion, sb
        rig.check(expected)
    finally:
        rig.free()


def test_stage(ctx):
    """Three unlike pictures -- geometry, chroma format and number of references -- in one call, and in the other order."""
    names = K.THREE_UNLIKE
    assert len({K.CASES[n]["fmt"] for n in names}) == 3 and {K.CASES[n]["refs"] for n in names} == {1, 2}
    for order, seed in ((names, 3), (names[::-1], 4)):
        run_stage(ctx, [case_entry(n) for n in order], [K.inputs(n)[2] for n in order], [K.expected(n)[:2] for n in order], seed)


@pytest.mark.parametrize("n", range(K.N_DRAWS))
def test_random_draw(ctx, n):
    c, src, refs, fields, motion, sb, _ = K.draw(n)
    run_stage(ctx, [(c, src, refs)], [fields], [(motion, sb)], seed=100 + n)


def test_rounding(ctx):
    """The crafted tables at lambda 0.1: the records equal the unfused restatement's, and so differ from the fused one's."""
    fields, table, plain, sb, fused = K.rounding()
    c = dict(K.ROUNDING)
    flat = [np.zeros((h, w), np.uint8) for (w, h) in K._sizes(c)]       # (the choice reads no picture: only its size)
    rig = Rig(ctx, [(c, flat, [flat, flat])], ("motion", "superblocks"), seed=77)
    try:
        rig.put_fields(0, fields)
        rig.put(0, "table", table)
        ctx.split2_choose_batch([rig.picture(0)], [rig.span(0, "table")])
        ctx.synchronize()
        got = rig.span(0, "motion").download().reshape(-1).view(sa.MV_DTYPE)
        assert got.tobytes() != fused.tobytes()
        rig.check({(0, "motion"): plain, (0, "superblocks"): sb})
    finally:
        rig.free()


# ---- behind the sub-pel refinement, and into the renderer ---------------------------------------------------------------

CHAIN_SIZE, CHAIN_LEVELS, CHAIN_PREC, CHAIN_LAMBDA = (101, 75), 2, 2, 0.1


def chain_expected():
    """(params, the sub-pel fields, motion, superblocks) of the restatements chained: block matching with level 0, the
    sub-pel refinement of both references, the split-2 level."""
    (w, h), ext = CHAIN_SIZE, HK.CHAIN_EXT
    frame, ref = HK.chain_pictures(w, h)
    P = HK.chain_params(w, h)
    level0 = [HK.chain_reference(w, h, CHAIN_LEVELS, r)[0][0] for r in (0, 1)]
    sub = [S.subpel_deep(frame[0], ref[0], P, CHAIN_PREC, r, CHAIN_LAMBDA, level0[r], ext)[0] for r in (0, 1)]
    P2 = dict(P, mv_precision=CHAIN_PREC, h_shift=1, v_shift=1)
    motion, sb, _ = R.split2(frame, [ref, ref], P2, CHAIN_LAMBDA, sub, ext)
    return P2, level0, sub, motion, sb


def run_chain(ctx, render):
    """hbm_batch (with_level0) of both references, subpel_batch with its level-0 fields as sources, split2_batch on the
    sub-pel fields -- and, with `render`, obmc_batch in its prediction-only form on the motion field -- on one queue, no
    download in between."""
    (w, h), ext = CHAIN_SIZE, HK.CHAIN_EXT
    frame, ref = HK.chain_pictures(w, h)
    P2, level0, sub_want, motion, sb = chain_expected()
    P = HK.chain_params(w, h)
    fl, fv = device_pyramid(ctx, frame, CHAIN_LEVELS, ext)
    rl, rv = device_pyramid(ctx, ref, CHAIN_LEVELS, ext)
    hp = [ctx.hp_plane(*p.shape) for p in ref]
    ctx.upsample_batch([(rv[0][k], hp[k]) for k in range(3)])
    n = P["x_num_blocks"] * P["y_num_blocks"]
    lay = G.Layout()
    hbm = [[lay.span(n * MV, footprint=("bytes", n * MV), name="hbm_r%d_l%d" % (r, k), align=64, skew=4 * r) for k in range(CHAIN_LEVELS + 1)]
           for r in (0, 1)]
    sub = [lay.span(n * MV, footprint=("bytes", n * MV), name="subpel_r%d" % r, align=64, skew=8 - 4 * r) for r in (0, 1)]
    mot = lay.span(n * MV, footprint=("bytes", n * MV), name="motion", align=64, skew=4)
    sbs = lay.span(n // 16 * SB, footprint=("bytes", n // 16 * SB), name="superblocks", align=64, skew=8)
    MP = synth.motion_params(w, h, 12, 8, CHAIN_PREC, (1, 1, 1), (1, 1))
    assert (MP["x_num_blocks"], MP["y_num_blocks"]) == (P["x_num_blocks"], P["y_num_blocks"])
    pred = [lay.plane(p.shape[0], p.shape[1], np.int16, stride=p.shape[1] * 2 + (2, 0, 6)[k], name="prediction%d" % k) for k, p in enumerate(frame)] \
        if render else []
    block = G.GuardedBlock(ctx, lay, seed=9 + render)
    try:
        levels = [(fv[k], rv[k], ext) for k in range(CHAIN_LEVELS + 1)]
        ctx.hbm_batch([(levels, 1, 1, P, r, [block[s] for s in hbm[r]]) for r in (0, 1)], True)
        ctx.subpel_batch([(fv[0][0], hp[0], ext, P, CHAIN_PREC, r, CHAIN_LAMBDA, block[hbm[r][0]], block[sub[r]]) for r in (0, 1)])
        ctx.split2_batch([(fv[0], [hp, hp], (1, 1), ext, P2, CHAIN_LAMBDA, [block[sub[0]], block[sub[1]]], block[mot], block[sbs])])
        if render:
            ctx.obmc_batch([sa.obmc_plane(block[mot], MP, k, hp[k], hp[k], None, block[pred[k]], prediction_only=2) for k in range(3)])
        ctx.synchronize()
        expected = {sub[r]: as_bytes(sub_want[r]) for r in (0, 1)}
        expected.update({hbm[r][0]: as_bytes(level0[r]) for r in (0, 1)})
        expected.update({mot: as_bytes(motion), sbs: as_bytes(sb)})
        if render:
            # the oracle's render of the restatement's motion, as tests/encode_loop_draws.py has its predictions
            for k in range(3):
                u = O.UpComp(ref[k], upsample=True)
                ch, cw = frame[k].shape
                acc = O.motion_render(motion, O.MotionParams(**MP), k, u, u, np.zeros((ch, cw), np.int16), cw, ch, return_acc=True)[1]
                expected[pred[k]] = O.rrshift6_s16(acc)
        block.check(expected)
    finally:
        block.free()
        for p in hp:
            p.free()
        free_pyramid(fl + rl)


def test_behind_subpel(ctx):
    run_chain(ctx, False)


def test_into_obmc(ctx):
    """The device motion field of test_behind_subpel goes straight into obmc_batch, prediction only, for Y, U and V: the
    first rendered prediction with no vector from the host."""
    run_chain(ctx, True)


def test_frame_layer(ctx):
    """schro_mode_decision_split2_hip: a 4:2:0 picture (its upsampled frames keep chroma as (U, V) pair images), a 4:4:4 one
    (three plane images) and one with a single reference."""
    for name in ("clipped_padded_both", "format_444", "one_reference", "block_32x32_420"):
        c = K.CASES[name]
        src, refs, fields = K.inputs(name)
        motion, sb, _, _ = K.expected(name)
        hs, vs = shifts(c)
        fmt = frames.frame_format(np.uint8, hs, vs)
        planes = [ctx.upload(np.pad(p, c["ext"], mode="edge")) for p in src]
        ups, plain = [], []
        try:
            for r in refs:
                d = frames.DeviceFrame(ctx, fmt, c["w"], c["h"]).upload(frames.HostFrame(r, hs, vs))
                u = frames.DeviceFrame(ctx, fmt, c["w"], c["h"], upsampled=True)
                sa.check(ctx.lib.schro_upsampled_hipframe_upsample(u.ptr(), d.ptr()))
                plain.append(d)
                ups.append(u)
            got, got_sb = ctx.mode_decision_split2(planes, ups, K.params_of(c), c["lam"], fields, extension=c["ext"], h_shift=hs, v_shift=vs)
            assert got.tobytes() == motion.tobytes(), name
            assert got_sb.tobytes() == sb.tobytes(), name
        finally:
            for p in planes:
                p.free()
            for f in ups + plain:
                f.unref()


def test_a_refused_call_writes_nothing(ctx):
    """Refusals with a context: the second picture of the call is bad; nothing is touched, whichever of the three calls."""
    entry = case_entry(K.REFUSED_CASE)
    c = entry[0]
    rig = Rig(ctx, [entry, entry], ("table", "motion", "superblocks"), seed=5)
    try:
        good = [rig.picture(n) for n in (0, 1)]
        SRC, REFS, SHIFTS, EXT, PARAMS, LAM, FIELDS, MOTION, SBS = range(9)

        def second(index, value):
            a = list(good[1])
            a[index] = value
            return [good[0], tuple(a)]

        def spoilt(member, value):
            if member == "stride":
                return second(SRC, [sa.SubPlane(good[1][SRC][0], 0, 0, c["h"], c["w"], stride=c["w"] + value)] + good[1][SRC][1:])
            if member in ("nbx", "nby", "xb", "yb", "prec"):
                key = {"nbx": "x_num_blocks", "nby": "y_num_blocks", "xb": "xbsep_luma", "yb": "ybsep_luma", "prec": "mv_precision"}[member]
                return second(PARAMS, dict(good[1][PARAMS], **{key: value}))
            if member == "refs":
                return second(REFS, (good[1][REFS] * 2)[:value])
            if member == "no_component":
                return second(SRC, [None if k == value else p for k, p in enumerate(good[1][SRC])])
            if member == "no_image":
                return second(REFS, [[None if (r, k) == value else p for k, p in enumerate(ref)] for r, ref in enumerate(good[1][REFS])])
            if member == "no_field":
                return second(FIELDS, [None if r == value else f for r, f in enumerate(good[1][FIELDS])])
            if member in ("no_motion", "no_superblocks"):
                return second(MOTION if member == "no_motion" else SBS, None)
            return second({"ext": EXT, "lam": LAM, "shifts": SHIFTS}[member], value)

        tabs = [rig.span(n, "table") for n in (0, 1)]
        for member, value, word in K.REFUSED_MEMBERS:
            for call in (lambda p: ctx.split2_batch(p), lambda p: ctx.split2_metric_batch(p, tabs), lambda p: ctx.split2_choose_batch(p, tabs)):
                with pytest.raises(sa.SchroHipError, match="picture 1"):
                    call(spoilt(member, value))
        # one table for two pictures; a table that is the other picture's motion field
        for call in (ctx.split2_metric_batch, ctx.split2_choose_batch):
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                call(good, [tabs[0], tabs[0]])
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                call(good, [tabs[0], good[0][MOTION]])
        # a motion field that is the first picture's field; two pictures with one motion field or one superblock table
        for pictures in (second(MOTION, good[0][FIELDS][0]), second(MOTION, good[0][MOTION]), second(SBS, good[0][SBS])):
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                ctx.split2_batch(pictures)
        ctx.synchronize()
        rig.check({})
    finally:
        rig.free()
