"""GPU: sub-pel motion refinement on the device (subpel.hip) against tests/subpel_ref.py: the error tables entry for
entry, and all 20 bytes of every record of every field.

Every picture, field and table of every test lies in a guarded block (tests/guard_lib.py): a byte written outside a field
or table, or an input changed, fails the test that did it.  The upsampled images are made by upsample_batch outside the
block and compared with themselves afterwards."""
import zlib

import numpy as np
import pytest

import guard_lib as G
import hier_bm_cases as HK
import schroedinger_amd as sa
import subpel_cases as K
import subpel_ref as R
from schroedinger_amd import frames
from test_gpu_hier_bm import device_pyramid, free_pyramid

pytestmark = pytest.mark.gpu

MV = sa.MV_DTYPE.itemsize


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(1, -1)


def records(c):
    return c["nbx"] * c["nby"]


class Rig:
    """Some (case, picture, reference) entries in one guarded block: per entry the source plane (stride w + pad) and the
    named byte spans `spans[k]` -- {name: (bytes, written)} -- and, outside the block, the upsampled reference."""

    def __init__(self, ctx, entries, spans, seed):
        self.ctx, self.entries = ctx, entries
        lay = G.Layout()
        self.src, self.sp = [], []
        for k, ((c, src, ref), names) in enumerate(zip(entries, spans)):
            self.src.append(lay.plane(c["h"], c["w"], np.uint8, stride=c["w"] + c["pad"], footprint=None, name="src%d" % k, align=64,
                                      skew=(c["pad"] + k) % 4))
            self.sp.append({nm: lay.span(n, footprint=("bytes", n) if wr else None, name="%s%d" % (nm, k), align=64, skew=4 * ((k + len(nm)) % 3))
                            for nm, (n, wr) in names.items()})
        self.block = G.GuardedBlock(ctx, lay, seed=seed)
        self.hp, self.tmp = [], []
        for k, (c, src, ref) in enumerate(entries):
            self.block[self.src[k]].upload(src)
            d, hp = ctx.upload(ref), ctx.hp_plane(c["h"], c["w"])
            ctx.upsample_batch([(d, hp)])
            self.hp.append(hp)
            self.tmp.append(d)
        ctx.synchronize()
        self.hp_before = [hp.download() for hp in self.hp]

    def span(self, k, name):
        return self.block[self.sp[k][name]]

    def put(self, k, name, a):
        self.span(k, name).upload(as_bytes(a))

    def chain(self, k, src_field, field, prec=None, lam=None):
        c = self.entries[k][0]
        return (self.block[self.src[k]], self.hp[k], c["ext"], K.params_of(c), c["prec"] if prec is None else prec, c["ref_index"],
                c["lam"] if lam is None else lam, self.span(k, src_field) if src_field else None, self.span(k, field))

    def check(self, expected):
        """expected: {(k, name): array}; whatever is not named keeps what it held."""
        extra = ["upsampled image %d changed" % k for k, hp in enumerate(self.hp) if not np.array_equal(hp.download(), self.hp_before[k])]
        self.block.check({self.sp[k][nm]: as_bytes(a) for (k, nm), a in expected.items()}, extra=extra)

    def free(self):
        self.block.free()
        for p in self.hp + self.tmp:
            p.free()


def case_entry(name):
    src, ref, _ = K.inputs(name)
    return K.CASES[name], src, ref


PASS_CASES = sorted(n for n in K.CASES if K.CASES[n]["prec"] > 0)


@pytest.mark.parametrize("name", PASS_CASES)
def test_error_launch(ctx, name):
    """Every pass of the case from the field the restatement has in front of it: the table entry for entry -- -1 for the
    inadmissible and the skipped -- and the field left as it was."""
    c = K.CASES[name]
    fields, (_, tables, _) = K.fields_by_pass(name), K.expected(name)
    n = records(c)
    spans = {}
    for p in range(1, c["prec"] + 1):
        spans["field%d" % p] = (n * MV, False)
        spans["table%d" % p] = (n * 32, True)
    rig = Rig(ctx, [case_entry(name)], [spans], seed=zlib.crc32(name.encode()) & 0xffff)
    try:
        for p in range(1, c["prec"] + 1):
            rig.put(0, "field%d" % p, fields[p - 1])
            ctx.subpel_error_batch([rig.chain(0, None, "field%d" % p)], p, [rig.span(0, "table%d" % p)])
        ctx.synchronize()
        rig.check({(0, "table%d" % p): tables[p - 1] for p in range(1, c["prec"] + 1)})
    finally:
        rig.free()


@pytest.mark.parametrize("name", PASS_CASES)
def test_choice_launch(ctx, name):
    """Every pass of the case from the restatement's tables: all 20 bytes of every record; the tables are left alone."""
    c = K.CASES[name]
    fields, (_, tables, _) = K.fields_by_pass(name), K.expected(name)
    n = records(c)
    spans = {}
    for p in range(1, c["prec"] + 1):
        spans["field%d" % p] = (n * MV, True)
        spans["table%d" % p] = (n * 32, False)
    rig = Rig(ctx, [case_entry(name)], [spans], seed=1 + (zlib.crc32(name.encode()) & 0xffff))
    try:
        for p in range(1, c["prec"] + 1):
            rig.put(0, "field%d" % p, fields[p - 1])
            rig.put(0, "table%d" % p, tables[p - 1])
            ctx.subpel_choose_batch([rig.chain(0, None, "field%d" % p)], p, [rig.span(0, "table%d" % p)])
        ctx.synchronize()
        rig.check({(0, "field%d" % p): fields[p] for p in range(1, c["prec"] + 1)})
    finally:
        rig.free()


def test_choice_rounds_the_product_and_then_the_sum(ctx):
    """The crafted tables at lambda 0.1: the records equal the unfused restatement's, and so differ from the fused one's."""
    src, start, table, plain, fused = K.rounding()
    c = dict(K.ROUNDING)
    n = records(c)
    rig = Rig(ctx, [(c, src, src)], [{"field": (n * MV, True), "table": (n * 32, False)}], seed=77)
    try:
        rig.put(0, "field", start)
        rig.put(0, "table", table)
        ctx.subpel_choose_batch([rig.chain(0, None, "field")], 1, [rig.span(0, "table")])
        ctx.synchronize()
        got = rig.span(0, "field").download().reshape(-1).view(sa.MV_DTYPE)
        assert got.tobytes() != fused.tobytes()
        rig.check({(0, "field"): plain})
    finally:
        rig.free()


def run_stage(ctx, names_or_entries, want, starts, in_place, seed):
    """schro_hip_subpel_batch over the entries in one call; source != destination, or in place."""
    entries = names_or_entries
    spans = []
    for (c, _, _) in entries:
        n = records(c) * MV
        spans.append({"field": (n, True)} if in_place else {"start": (n, False), "field": (n, True)})
    rig = Rig(ctx, entries, spans, seed=seed)
    try:
        for k, f in enumerate(starts):
            rig.put(k, "field" if in_place else "start", f)
        ctx.subpel_batch([rig.chain(k, "field" if in_place else "start", "field") for k in range(len(entries))])
        ctx.synchronize()
        rig.check({(k, "field"): f for k, f in enumerate(want)})
    finally:
        rig.free()


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in_place"])
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_whole_stage(ctx, name, in_place):
    run_stage(ctx, [case_entry(name)], [K.expected(name)[0]], [K.inputs(name)[2]], in_place, seed=2 + (zlib.crc32(name.encode()) & 0xfff))


def test_three_unlike_chains_in_one_call(ctx):
    names = K.THREE_UNLIKE
    assert sorted(K.CASES[n]["prec"] for n in names)[0] == 0 and len({K.CASES[n]["prec"] for n in names}) == 3
    run_stage(ctx, [case_entry(n) for n in names], [K.expected(n)[0] for n in names], [K.inputs(n)[2] for n in names], False, seed=3)
    run_stage(ctx, [case_entry(n) for n in reversed(names)], [K.expected(n)[0] for n in reversed(names)], [K.inputs(n)[2] for n in reversed(names)],
              True, seed=4)


@pytest.mark.parametrize("n", range(K.N_DRAWS))
def test_random_draw(ctx, n):
    c, src, ref, start, field, _ = K.draw(n)
    run_stage(ctx, [(c, src, ref)], [field], [start], bool(n & 1), seed=100 + n)


def test_frame_layer_two_references(ctx):
    """schro_encoder_motion_predict_subpel_deep_hip: a picture, two upsampled reference frames, two host fields."""
    names = ("partial_blocks_12", "padded_stride")
    for name in names:
        c = K.CASES[name]
        src, ref0, start = K.inputs(name)
        ref1 = K.RH.moved(src, -1, 2, c["seed"] + 5000)
        refs = (ref0, ref1)
        w, h, ext = c["w"], c["h"], c["ext"]
        P = dict(K.params_of(c), mv_precision=c["prec"])
        starts = [start, K.start_field(dict(c, ref_index=1 - c["ref_index"], seed=c["seed"] + 1), src.astype(np.int32), ref1.astype(np.int32))]
        if c["ref_index"] == 1:             # (field r refines dx[r], dy[r])
            refs, starts = refs[::-1], starts[::-1]
        want = [R.subpel_deep(src, refs[r], K.params_of(c), c["prec"], r, 0.1, starts[r], ext)[0] for r in (0, 1)]
        d_src = ctx.upload(np.pad(src, ext, mode="edge"))
        ups, plain = [], []
        try:
            for r in (0, 1):
                chroma = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
                d = frames.DeviceFrame(ctx, sa.FORMAT_U8_420, w, h).upload(frames.HostFrame([refs[r], chroma, chroma], 1, 1))
                u = frames.DeviceFrame(ctx, sa.FORMAT_U8_420, w, h, upsampled=True)
                sa.check(ctx.lib.schro_upsampled_hipframe_upsample(u.ptr(), d.ptr()))
                plain.append(d)
                ups.append(u)
            got = ctx.subpel_deep(d_src, ups, P, 0.1, starts, extension=ext)
            for r in (0, 1):
                assert as_bytes(got[r]).tobytes() == as_bytes(want[r]).tobytes(), (name, r)
        finally:
            d_src.free()
            for f in ups + plain:
                f.unref()


@pytest.mark.parametrize("size", [(101, 75)])
def test_hbm_hands_its_level_0_field_over_on_the_device(ctx, size):
    """hbm_batch (with_level0) of both references, then subpel_batch with fields[0] as its source on the same queue, no
    download between: the two restatements chained."""
    (w, h), ext, n_levels, prec, lam = size, HK.CHAIN_EXT, 2, 2, 0.1
    frame, ref = HK.chain_pictures(w, h)
    P = HK.chain_params(w, h)
    level0 = [HK.chain_reference(w, h, n_levels, r)[0][0] for r in (0, 1)]
    want = [R.subpel_deep(frame[0], ref[0], P, prec, r, lam, level0[r], ext)[0] for r in (0, 1)]
    fl, fv = device_pyramid(ctx, frame, n_levels, ext)
    rl, rv = device_pyramid(ctx, ref, n_levels, ext)
    hp = ctx.hp_plane(h, w)
    ctx.upsample_batch([(rv[0][0], hp)])
    n = P["x_num_blocks"] * P["y_num_blocks"] * MV
    lay = G.Layout()
    hbm = [[lay.span(n, footprint=("bytes", n), name="hbm_r%d_l%d" % (r, k), align=64, skew=4 * r) for k in range(n_levels + 1)] for r in (0, 1)]
    sub = [lay.span(n, footprint=("bytes", n), name="subpel_r%d" % r, align=64, skew=8 - 4 * r) for r in (0, 1)]
    block = G.GuardedBlock(ctx, lay, seed=9)
    try:
        levels = [(fv[k], rv[k], ext) for k in range(n_levels + 1)]
        ctx.hbm_batch([(levels, 1, 1, P, r, [block[s] for s in hbm[r]]) for r in (0, 1)], True)
        ctx.subpel_batch([(fv[0][0], hp, ext, P, prec, r, lam, block[hbm[r][0]], block[sub[r]]) for r in (0, 1)])
        ctx.synchronize()
        expected = {sub[r]: as_bytes(want[r]) for r in (0, 1)}
        expected.update({hbm[r][0]: as_bytes(level0[r]) for r in (0, 1)})
        block.check(expected)
    finally:
        block.free()
        hp.free()
        free_pyramid(fl + rl)


def test_a_refused_call_writes_nothing(ctx):
    """Refusals with a context: the second chain of the call is bad; neither field is touched, whichever of the three calls."""
    entry = case_entry(K.REFUSED_CASE)
    c = entry[0]
    n = records(c)
    spans = {"start": (n * MV, False), "field": (n * MV, True), "table": (n * 32, True)}
    rig = Rig(ctx, [entry, entry], [spans, spans], seed=5)
    try:
        good = [rig.chain(k, "start", "field") for k in (0, 1)]
        SRC, EXT, PARAMS, PREC, REF, LAM, START, FIELD = 0, 2, 3, 4, 5, 6, 7, 8

        def second(index, value):
            a = list(good[1])
            a[index] = value
            return [good[0], tuple(a)]

        def spoilt(member, value):
            if member == "stride":
                return second(SRC, sa.SubPlane(good[1][SRC], 0, 0, c["h"], c["w"], stride=c["w"] + value))
            if member in ("nbx", "nby", "xb", "yb"):
                key = {"nbx": "x_num_blocks", "nby": "y_num_blocks", "xb": "xbsep_luma", "yb": "ybsep_luma"}[member]
                return second(PARAMS, dict(good[1][PARAMS], **{key: value}))
            return second({"prec": PREC, "ref_index": REF, "ext": EXT, "lam": LAM}[member], value)

        tabs = [rig.span(k, "table") for k in (0, 1)]
        for member, value in K.REFUSED_MEMBERS:
            for call in (lambda ch: ctx.subpel_batch(ch), lambda ch: ctx.subpel_error_batch(ch, 1, tabs), lambda ch: ctx.subpel_choose_batch(ch, 1, tabs)):
                with pytest.raises(sa.SchroHipError, match="chain 1"):
                    call(spoilt(member, value))
        # a pass beyond the chain's precision; one table for two chains; a table that is the other chain's field
        with pytest.raises(sa.SchroHipError, match="pass 2 is outside"):
            ctx.subpel_error_batch(good, 2, tabs)
        with pytest.raises(sa.SchroHipError, match="pass 0 is outside"):
            ctx.subpel_choose_batch(good, 0, tabs)
        for call in (ctx.subpel_error_batch, ctx.subpel_choose_batch):
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                call(good, 1, [tabs[0], tabs[0]])
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                call(good, 1, [tabs[0], good[0][FIELD]])
        # a source field that is the first chain's field; two chains with one field
        for call in (second(START, good[0][FIELD]), second(FIELD, good[0][FIELD])):
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                ctx.subpel_batch(call)
        ctx.synchronize()
        rig.check({})
    finally:
        rig.free()
