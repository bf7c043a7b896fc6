"""GPU: schro_mode_decision entire on the device (mode_decision.hip) against tests/mode_ref.py: the mode table entry for
entry, all 20 bytes of every motion record, the superblock and trial tables with their scores compared as bits, and the
three statistics as bits.

Every picture, field, table and output of every test lies in a guarded block (tests/guard_lib.py): a byte written outside
an output, or an input changed, fails the test that did it.  The upsampled images are made by upsample_batch outside the
block and compared with themselves afterwards."""
import zlib

import numpy as np
import pytest

import guard_lib as G
import hier_bm_cases as HK
import mode_cases as C
import mode_ref as M
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
ENTRY2 = 4 * sa.SPLIT2_TABLE_INTS
ENTRY = 4 * sa.MODE_TABLE_INTS
SB = sa.SB_DTYPE.itemsize
TRIALS = 4 * sa.MODE_TRIAL_DTYPE.itemsize
OUTPUTS = ("motion", "superblocks", "trials", "stats")


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(1, -1)


def records(c):
    return c["nbx"] * c["nby"]


def shifts(c):
    return K.FORMATS[c["fmt"]]


def test_the_constants_are_the_restatement_s():
    assert (sa.MODE_TABLE_INTS, sa.MODE_CANDIDATES, sa.MODE_CANDIDATE_INTS, sa.MODE_ZERO_TRIAL) == (M.M_INTS, M.M_CANDS, M.M_CAND_INTS, M.M_ZERO_BI)
    assert sa.MODE_TRIAL_DTYPE == M.TRIAL_DTYPE


class Rig:
    """Some (case, source planes, reference planes) entries in one guarded block: per entry the three source planes (stride
    width + pad), the sub-pel, level-1 and level-2 fields, the two tables and the four outputs -- and, outside the block,
    the upsampled images of every component of every reference."""

    def __init__(self, ctx, entries, written, seed):
        self.ctx, self.entries = ctx, entries
        lay = G.Layout()
        self.src, self.sp = [], []
        for n, (c, src, refs) in enumerate(entries):
            self.src.append([lay.plane(p.shape[0], p.shape[1], np.uint8, stride=p.shape[1] + c["pad"], footprint=None, name="src%d_%d" % (n, k),
                                       align=64, skew=(c["pad"] + n + k) % 4) for k, p in enumerate(src)])
            sizes = {"table2": records(c) * ENTRY2, "table": records(c) // 16 * ENTRY, "motion": records(c) * MV, "superblocks": records(c) // 16 * SB,
                     "trials": records(c) // 16 * TRIALS, "stats": 24}
            for r in (0, 1):
                for kind in ("field", "level1_", "level2_"):
                    sizes["%s%d" % (kind, r)] = records(c) * MV
            self.sp.append({nm: lay.span(size, footprint=("bytes", size) if nm in written else None, name="%s%d" % (nm, n), align=64,
                                         skew=(8 if nm in ("superblocks", "trials", "stats") else 4) * ((n + len(nm)) % 3)) for nm, size in sizes.items()})
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

    def put_fields(self, n, fields, level1, level2):
        for r in range(len(fields)):
            self.put(n, "field%d" % r, fields[r])
            self.put(n, "level1_%d" % r, level1[r])
            self.put(n, "level2_%d" % r, level2[r])

    def tables(self, ns):
        return [self.span(n, nm) for n in ns for nm in ("table2", "table")]

    def picture(self, n):
        c, _, refs = self.entries[n]
        nr = range(len(refs))
        return ([self.block[s] for s in self.src[n]], self.hp[n], shifts(c), c["ext"], K.params_of(c), c["lam"], [self.span(n, "field%d" % r) for r in nr],
                [self.span(n, "level1_%d" % r) for r in nr], [self.span(n, "level2_%d" % r) for r in nr], self.span(n, "motion"),
                self.span(n, "superblocks"), self.span(n, "trials"), self.span(n, "stats"))

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
    src, refs = C.inputs(name)[:2]
    return C.CASES[name], src, refs


def seed_of(name, k=0):
    return k + (zlib.crc32(name.encode()) & 0xfff0)


def outputs(n, out):
    return {(n, nm): out[k] for k, nm in enumerate(OUTPUTS)}


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_metric_launch(ctx, name):
    """Both tables entry for entry -- the markers of quadrants outside the picture, of SADs nothing may ask for and of the
    reference a picture does not have included -- and everything else left as it was."""
    out = C.expected(name)
    rig = Rig(ctx, [case_entry(name)], ("table2", "table"), seed=seed_of(name))
    try:
        rig.put_fields(0, *C.inputs(name)[2:])
        ctx.mode_metric_batch([rig.picture(0)], rig.tables([0]))
        ctx.synchronize()
        rig.check({(0, "table2"): out[4], (0, "table"): out[5]})
    finally:
        rig.free()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_choice_launch(ctx, name):
    """From the restatement's tables: all 20 bytes of every motion record, the superblock and the trial table with the
    scores as bits, the statistics as bits; the tables, the fields and the images are left alone."""
    out = C.expected(name)
    rig = Rig(ctx, [case_entry(name)], OUTPUTS, seed=seed_of(name, 1))
    try:
        rig.put_fields(0, *C.inputs(name)[2:])
        rig.put(0, "table2", out[4])
        rig.put(0, "table", out[5])
        ctx.mode_choose_batch([rig.picture(0)], rig.tables([0]))
        ctx.synchronize()
        rig.check(outputs(0, out))
    finally:
        rig.free()


def run_stage(ctx, entries, inputs, want, seed):
    """schro_hip_mode_decision_batch over the entries in one call."""
    rig = Rig(ctx, entries, OUTPUTS, seed=seed)
    try:
        for n, (fields, level1, level2) in enumerate(inputs):
            rig.put_fields(n, fields, level1, level2)
        ctx.mode_decision_batch([rig.picture(n) for n in range(len(entries))])
        ctx.synchronize()
        expected = {}
        for n, out in enumerate(want):
            expected.update(outputs(n, out))
        rig.check(expected)
    finally:
        rig.free()


def test_stage(ctx):
    """Three unlike pictures -- geometry, chroma format and number of references -- in one call, and in the other order."""
    names = C.THREE_UNLIKE
    assert len({C.CASES[n]["fmt"] for n in names}) == 3 and {C.CASES[n]["refs"] for n in names} == {1, 2}
    for order, seed in ((names, 3), (names[::-1], 4)):
        run_stage(ctx, [case_entry(n) for n in order], [C.inputs(n)[2:] for n in order], [C.expected(n) for n in order], seed)


@pytest.mark.parametrize("n", range(C.N_DRAWS))
def test_random_draw(ctx, n):
    c, (src, refs, fields, level1, level2), out = C.draw(n)
    run_stage(ctx, [(c, src, refs)], [(fields, level1, level2)], [out], seed=100 + n)


def test_crafted_tables(ctx):
    """Rule 7 and an invalid split-0 trial, certain by construction (tests/mode_cases.py): the walk from tables made by
    hand.  No pair of vectors is measured, so the pictures are only their sizes.  At lambda 0.1 these scores are where a
    fused multiply-add would round otherwise: the result equals the unfused restatement's."""
    fields, level1, level2, table2, table, out, stats = C.crafted()
    c = dict(C.CRAFTED)
    assert stats["rule7"] > 0
    flat = [np.zeros((h, w), np.uint8) for (w, h) in K._sizes(c)]
    rig = Rig(ctx, [(c, flat, [flat, flat])], OUTPUTS, seed=78)
    try:
        rig.put_fields(0, fields, level1, level2)
        rig.put(0, "table2", table2)
        rig.put(0, "table", table)
        ctx.mode_choose_batch([rig.picture(0)], rig.tables([0]))
        ctx.synchronize()
        rig.check(outputs(0, out))
    finally:
        rig.free()


@pytest.mark.parametrize("split", [1, 0])
def test_rounding(ctx, split):
    """Crafted candidates that tie in exact arithmetic at split 1 and at split 0 (tests/mode_cases.py): the records equal
    the unfused restatement's, and so differ from the fused one's."""
    fields, level1, level2, table2, table, plain, fused = C.rounding(split)
    c = dict(C.CRAFTED)
    flat = [np.zeros((h, w), np.uint8) for (w, h) in K._sizes(c)]
    rig = Rig(ctx, [(c, flat, [flat, flat])], OUTPUTS, seed=90 + split)
    try:
        rig.put_fields(0, fields, level1, level2)
        rig.put(0, "table2", table2)
        rig.put(0, "table", table)
        ctx.mode_choose_batch([rig.picture(0)], rig.tables([0]))
        ctx.synchronize()
        got = rig.span(0, "motion").download().reshape(-1).view(sa.MV_DTYPE)
        assert got.tobytes() != fused[0].tobytes()
        rig.check(outputs(0, plain))
    finally:
        rig.free()


def test_fused_scores_would_differ(ctx):
    """A case on real pictures whose fused restatement gives other score bits: the device gives the unfused ones."""
    for name in ("lambda_small", "precision_1", "format_444", "lambda_10", "padded_x"):
        c = C.CASES[name]
        out = C.expected(name)
        src, refs, fields, level1, level2 = C.inputs(name)
        P = C.params_of(c)
        fused = M.choose(out[4], out[5], P, c["w"], c["h"], c["lam"], fields, level1, level2, M.picture_reader(src, refs, P, c["ext"]), fused=True)
        if fused[2].tobytes() != out[2].tobytes():
            break
    else:
        raise AssertionError("no case separates the fused from the unfused score")
    run_stage(ctx, [case_entry(name)], [C.inputs(name)[2:]], [out], seed=79)


def test_agreement_with_the_split2_stage(ctx):
    """One reference, every level-1 and level-2 record INT_MAX.  The sub-pel records are hints of split 1 too
    (schromotionest.c:1908-1917), so split 1 is still tried there; what must agree with schro_hip_split2_batch on the same
    inputs is the split-2 trial of the first superblock, bit for bit.  With every
    sub-pel metric INT_MAX as well no hint is left, split 1 is invalid everywhere, and the stage leaves exactly
    schro_hip_split2_batch's motion field and superblock table."""
    name = "all_int_max"
    c = C.CASES[name]
    src, refs, fields, level1, level2 = C.inputs(name)
    P = C.params_of(c)
    bare = [f.copy() for f in fields]
    for f in bare:
        f["metric"] = C.INT_MAX
    for sub, exact in ((fields, False), (bare, True)):
        out = M.mode_decision(src, refs, P, c["lam"], sub, level1, level2, c["ext"])
        assert (out[2]["state"][:, 1] == 0).all() == exact
        rig = Rig(ctx, [case_entry(name)], OUTPUTS, seed=80 + exact)
        try:
            rig.put_fields(0, sub, level1, level2)
            pic = rig.picture(0)
            ctx.split2_batch([pic[:7] + pic[9:11]])
            ctx.synchronize()
            motion2 = rig.span(0, "motion").download().reshape(-1).view(sa.MV_DTYPE).copy()
            sb2 = rig.span(0, "superblocks").download().reshape(-1).view(sa.SB_DTYPE).copy()
            ctx.mode_decision_batch([pic])
            ctx.synchronize()
            rig.check(outputs(0, out))
            motion = rig.span(0, "motion").download().reshape(-1).view(sa.MV_DTYPE)
            sb = rig.span(0, "superblocks").download().reshape(-1).view(sa.SB_DTYPE)
            trials = rig.span(0, "trials").download().reshape(-1).view(sa.MODE_TRIAL_DTYPE).reshape(-1, 4)
            # (a superblock's split-2 trial predicts from its neighbours as finally decided: only the first one, which
            # has none, must agree where split 1 is alive)
            rows = slice(None) if exact else slice(0, 1)
            for k in ("error", "entropy", "score"):
                assert trials[k][rows, 0].tobytes() == sb2[k][rows].tobytes(), k
            if exact:
                assert motion.tobytes() == motion2.tobytes() and sb.tobytes() == sb2.tobytes()
            else:
                assert motion.tobytes() != motion2.tobytes()
        finally:
            rig.free()


# ---- behind the block matching and the sub-pel refinement, and into the renderer ---------------------------------------

CHAIN_SIZE, CHAIN_LEVELS, CHAIN_PREC, CHAIN_LAMBDA = (101, 75), 2, 2, 0.1


def chain_expected():
    """(params, the block matching's fields per reference, the sub-pel fields, the restatement's outputs) of the
    restatements chained."""
    (w, h), ext = CHAIN_SIZE, HK.CHAIN_EXT
    frame, ref = HK.chain_pictures(w, h)
    P = HK.chain_params(w, h)
    hbm = [HK.chain_reference(w, h, CHAIN_LEVELS, r)[0] for r in (0, 1)]
    sub = [S.subpel_deep(frame[0], ref[0], P, CHAIN_PREC, r, CHAIN_LAMBDA, hbm[r][0], ext)[0] for r in (0, 1)]
    P2 = dict(P, mv_precision=CHAIN_PREC, h_shift=1, v_shift=1)
    out = M.mode_decision(frame, [ref, ref], P2, CHAIN_LAMBDA, sub, [hbm[0][1], hbm[1][1]], [hbm[0][2], hbm[1][2]], ext)
    return P2, hbm, sub, out


def test_chain_into_obmc(ctx):
    """hbm_batch (with level 0) of both references, subpel_batch on its level-0 fields, mode_decision_batch on the sub-pel
    fields and the level-1 and level-2 fields, obmc_batch in its prediction-only form on the motion field -- on one queue,
    no vector from the host: the rendered prediction equals the oracle's render of the restatement's field."""
    (w, h), ext = CHAIN_SIZE, HK.CHAIN_EXT
    frame, ref = HK.chain_pictures(w, h)
    P2, hbm_want, sub_want, out = chain_expected()
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
    trs = lay.span(n // 16 * TRIALS, footprint=("bytes", n // 16 * TRIALS), name="trials", align=64, skew=16)
    sts = lay.span(24, footprint=("bytes", 24), name="stats", align=64, skew=8)
    MP = synth.motion_params(w, h, 12, 8, CHAIN_PREC, (1, 1, 1), (1, 1))
    assert (MP["x_num_blocks"], MP["y_num_blocks"]) == (P["x_num_blocks"], P["y_num_blocks"])
    pred = [lay.plane(p.shape[0], p.shape[1], np.int16, stride=p.shape[1] * 2 + (2, 0, 6)[k], name="prediction%d" % k) for k, p in enumerate(frame)]
    block = G.GuardedBlock(ctx, lay, seed=11)
    try:
        levels = [(fv[k], rv[k], ext) for k in range(CHAIN_LEVELS + 1)]
        ctx.hbm_batch([(levels, 1, 1, P, r, [block[s] for s in hbm[r]]) for r in (0, 1)], True)
        ctx.subpel_batch([(fv[0][0], hp[0], ext, P, CHAIN_PREC, r, CHAIN_LAMBDA, block[hbm[r][0]], block[sub[r]]) for r in (0, 1)])
        ctx.mode_decision_batch([(fv[0], [hp, hp], (1, 1), ext, P2, CHAIN_LAMBDA, [block[sub[0]], block[sub[1]]], [block[hbm[0][1]], block[hbm[1][1]]],
                                  [block[hbm[0][2]], block[hbm[1][2]]], block[mot], block[sbs], block[trs], block[sts])])
        ctx.obmc_batch([sa.obmc_plane(block[mot], MP, k, hp[k], hp[k], None, block[pred[k]], prediction_only=2) for k in range(3)])
        ctx.synchronize()
        expected = {sub[r]: as_bytes(sub_want[r]) for r in (0, 1)}
        for r in (0, 1):
            for k in range(CHAIN_LEVELS + 1):
                expected[hbm[r][k]] = as_bytes(hbm_want[r][k])      # (the level-1 and level-2 fields the stage took its hints from)
        expected.update({mot: as_bytes(out[0]), sbs: as_bytes(out[1]), trs: as_bytes(out[2]), sts: as_bytes(out[3])})
        for k in range(3):
            u = O.UpComp(ref[k], upsample=True)
            ch, cw = frame[k].shape
            acc = O.motion_render(out[0], O.MotionParams(**MP), k, u, u, np.zeros((ch, cw), np.int16), cw, ch, return_acc=True)[1]
            expected[pred[k]] = O.rrshift6_s16(acc)
        block.check(expected)
    finally:
        block.free()
        for p in hp:
            p.free()
        free_pyramid(fl + rl)


def test_frame_layer(ctx):
    """schro_mode_decision_hip: a 4:2:0 picture (its upsampled frames keep chroma as (U, V) pair images), a 4:4:4 one
    (three plane images) and one with a single reference."""
    for name in ("clipped_padded", "format_444", "one_reference_padded"):
        c = C.CASES[name]
        src, refs, fields, level1, level2 = C.inputs(name)
        out = C.expected(name)
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
            got = ctx.mode_decision(planes, ups, K.params_of(c), c["lam"], fields, level1, level2, extension=c["ext"], h_shift=hs, v_shift=vs)
            for k, nm in enumerate(OUTPUTS):
                assert got[k].tobytes() == out[k].tobytes(), (name, nm)
        finally:
            for p in planes:
                p.free()
            for f in ups + plain:
                f.unref()


def test_a_refused_call_writes_nothing(ctx):
    """Refusals with a context: the second picture of the call is bad; nothing is touched, whichever of the three calls."""
    name = "precision_1"
    entry = case_entry(name)
    rig = Rig(ctx, [entry, entry], ("table2", "table") + OUTPUTS, seed=6)
    try:
        good = [rig.picture(n) for n in (0, 1)]
        tabs = rig.tables([0, 1])

        def second(index, value):
            a = list(good[1])
            a[index] = value
            return [good[0], tuple(a)]
        calls = (lambda p: ctx.mode_decision_batch(p), lambda p: ctx.mode_metric_batch(p, tabs), lambda p: ctx.mode_choose_batch(p, tabs))
        for index, value, word in C.REFUSED:
            for call in calls:
                with pytest.raises(sa.SchroHipError, match="(?=.*picture 1).*" + word):
                    call(second(index, value(good)))
        for call in (ctx.mode_metric_batch, ctx.mode_choose_batch):
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                call(good, [tabs[0], tabs[1], tabs[2], tabs[1]])
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                call(good, [tabs[0], tabs[1], tabs[2], good[0][C.TRIALS]])
        ctx.synchronize()
        rig.check({})
    finally:
        rig.free()
