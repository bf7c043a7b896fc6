"""GPU: hierarchical block matching on the device (hier_bm.hip) against tests/hier_bm_ref.py, record for record: all 20
bytes of every record of every field, the records off the level's grid and off the plane included.

Every plane and field of every test lies in a guarded block (tests/guard_lib.py): a byte written outside a field, or a
plane or hint field changed, fails the test that did it."""
import zlib

import numpy as np
import pytest

import analysis_ref as A
import guard_lib as G
import hier_bm_cases as K
import hier_bm_ref as R
import schroedinger_amd as sa

pytestmark = pytest.mark.gpu

MV = sa.MV_DTYPE.itemsize


def as_bytes(field):
    return np.ascontiguousarray(field).view(np.uint8).reshape(1, -1)


class Entries:
    """The planes and fields of some entries in one guarded block: per entry the three components of frame and ref (luma
    stride w + pad), the hint field (an input, or none) and the field (written whole)."""

    def __init__(self, ctx, entries, seed):
        self.ctx, self.entries = ctx, entries
        lay = G.Layout()
        self.specs = []
        for k, (c, frame, ref, hint) in enumerate(entries):
            n = c["nbx"] * c["nby"] * MV
            s = dict(frame=[], ref=[])
            for which, planes in (("frame", frame), ("ref", ref)):
                for m, p in enumerate(planes):
                    pad = c["pad"] if m == 0 else (c["pad"] + m) // 2
                    s[which].append(lay.plane(p.shape[0], p.shape[1], np.uint8, stride=p.shape[1] + pad, footprint=None,
                                              name="%s%d_%d" % (which, k, m), align=64, skew=(pad + m + (which == "ref")) % 4))
            s["hint"] = lay.span(n, footprint=None, name="hint%d" % k, align=64, skew=4 * (k % 3)) if hint is not None else None
            s["field"] = lay.span(n, footprint=("bytes", n), name="field%d" % k, align=64, skew=4 * ((k + 1) % 3))
            self.specs.append(s)
        self.block = G.GuardedBlock(ctx, lay, seed=seed)
        for (c, frame, ref, hint), s in zip(entries, self.specs):
            for m in range(3):
                self.block[s["frame"][m]].upload(frame[m])
                self.block[s["ref"][m]].upload(ref[m])
            if hint is not None:
                self.block[s["hint"]].upload(as_bytes(hint))

    def args(self):
        out = []
        for (c, _, _, hint), s in zip(self.entries, self.specs):
            hs, vs = K.FORMATS[c["fmt"]]
            out.append(([self.block[p] for p in s["frame"]], [self.block[p] for p in s["ref"]], c["ext"], hs, vs, K.params_of(c), c["shift"],
                        c["h_range"], c["ref_index"], self.block[s["hint"]] if hint is not None else None, self.block[s["field"]]))
        return out

    def run_and_check(self, fields):
        try:
            self.ctx.hbm_level_batch(self.args())
            self.ctx.synchronize()
            self.block.check({s["field"]: as_bytes(f) for s, f in zip(self.specs, fields)})
        finally:
            self.block.free()


def case_entry(name):
    return (K.CASES[name],) + K.inputs(name)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_named_case(ctx, name):
    field, _ = K.expected(name)
    Entries(ctx, [case_entry(name)], seed=zlib.crc32(name.encode()) & 0xffff).run_and_check([field])


def test_three_unlike_entries_in_one_call(ctx):
    names = K.THREE_UNLIKE
    assert len({(K.CASES[n]["shift"], K.CASES[n]["ref_index"], K.CASES[n]["fmt"]) for n in names}) == 3
    Entries(ctx, [case_entry(n) for n in names], seed=3).run_and_check([K.expected(n)[0] for n in names])


@pytest.mark.parametrize("n", range(K.N_DRAWS))
def test_random_draw(ctx, n):
    c, frame, ref, hint, field = K.draw(n)
    Entries(ctx, [(c, frame, ref, hint)], seed=100 + n).run_and_check([field])


# ---- the chain ------------------------------------------------------------------------------------------------------

def device_pyramid(ctx, planes, n_levels, ext):
    """[level][component]: DevicePlanes by Context.downsample_batch, each with `ext` samples of apron (level 0: the
    uploaded planes, edge-extended on the host); and the views of the pictures inside them."""
    levels = [[ctx.upload(A.edgeextend(p, ext)) for p in planes]]
    for _ in range(n_levels):
        src = [sa.SubPlane(p, ext, ext, p.height - 2 * ext, p.width - 2 * ext) for p in levels[-1]]
        dst = [ctx.plane((s.height + 1) // 2 + 2 * ext, (s.width + 1) // 2 + 2 * ext, np.uint8) for s in src]
        ctx.downsample_batch([(s, d, ext) for s, d in zip(src, dst)])
        levels.append(dst)
    views = [[sa.SubPlane(p, ext, ext, p.height - 2 * ext, p.width - 2 * ext) for p in lv] for lv in levels]
    return levels, views


def free_pyramid(levels):
    for lv in levels:
        for p in lv:
            p.free()


@pytest.mark.parametrize("with_level0", [False, True], ids=["levels", "with_level0"])
@pytest.mark.parametrize("n_levels", [1, 2, 3, 4])
@pytest.mark.parametrize("size", K.CHAIN_SIZES)
def test_chain_on_the_device_pyramid(ctx, size, n_levels, with_level0):
    """The pyramid and the search never leave the device: downsample_batch of all three components, then hbm_batch on its
    planes, both references of the picture as two chains of one launch; the fields are downloaded at the end."""
    (w, h), ext = size, K.CHAIN_EXT
    frame, ref = K.chain_pictures(w, h)
    want = [K.chain_reference(w, h, n_levels, r)[0] for r in (0, 1)]
    P = K.chain_params(w, h)
    fl, fv = device_pyramid(ctx, frame, n_levels, ext)
    rl, rv = device_pyramid(ctx, ref, n_levels, ext)
    first = 0 if with_level0 else 1
    lay = G.Layout()
    n = P["x_num_blocks"] * P["y_num_blocks"] * MV
    specs = [[lay.span(n, footprint=("bytes", n) if k >= first else None, name="field_r%d_l%d" % (r, k), align=64, skew=4 * r)
              for k in range(n_levels + 1)] for r in (0, 1)]
    block = G.GuardedBlock(ctx, lay, seed=n_levels)
    try:
        levels = [(fv[k], rv[k], ext) if k >= first else None for k in range(n_levels + 1)]
        ctx.hbm_batch([(levels, 1, 1, P, r, [block[s] if k >= first else None for k, s in enumerate(specs[r])]) for r in (0, 1)], with_level0)
        ctx.synchronize()
        # (a field the call does not own keeps the canary: its footprint is empty)
        block.check({specs[r][k]: as_bytes(want[r][k]) for r in (0, 1) for k in range(first, n_levels + 1)})
    finally:
        block.free()
        free_pyramid(fl + rl)


@pytest.mark.parametrize("size,n_levels,with_level0", [((128, 96), 3, True), ((101, 75), 4, True), ((101, 75), 2, False)])
def test_frame_layer_chain(ctx, size, n_levels, with_level0):
    (w, h), ext = size, K.CHAIN_EXT
    frame, ref = K.chain_pictures(w, h)
    want = K.chain_reference(w, h, n_levels, 1)[0]
    fl, _ = device_pyramid(ctx, frame, n_levels, ext)
    rl, _ = device_pyramid(ctx, ref, n_levels, ext)
    try:
        got = ctx.hbm_scan(fl, rl, K.chain_params(w, h), 1, with_level0=with_level0, extension=ext, h_shift=1, v_shift=1)
        assert len(got) == n_levels + 1 and (got[0] is None) == (not with_level0)
        for k in range(0 if with_level0 else 1, n_levels + 1):
            assert as_bytes(got[k]).tobytes() == as_bytes(want[k]).tobytes(), k
    finally:
        free_pyramid(fl + rl)


@pytest.mark.parametrize("name", ["padded_grid_shift0", "chroma_422", "ref_1_shift0", "nohint_top"])
def test_frame_layer_level(ctx, name):
    c, frame, ref, hint = case_entry(name)
    ext = c["ext"]
    hs, vs = K.FORMATS[c["fmt"]]
    fa, fb = ([ctx.upload(A.edgeextend(p, ext)) for p in planes] for planes in (frame, ref))
    try:
        got = ctx.hbm_scan_hint(fa, fb, K.params_of(c), c["shift"], c["h_range"], c["ref_index"], hint, extension=ext, h_shift=hs, v_shift=vs)
        assert as_bytes(got).tobytes() == as_bytes(K.expected(name)[0]).tobytes()
    finally:
        for p in fa + fb:
            p.free()


def test_a_refused_call_writes_nothing(ctx):
    """Refusals with a context: the second entry of the call is bad; neither field is touched."""
    good = case_entry(K.REFUSED_CASE)
    c = good[0]
    ent = Entries(ctx, [good, good], seed=5)
    try:
        args = ent.args()
        FRAME, EXT, HS, PARAMS, SHIFT, RANGE, REF, HINT, FIELD = 0, 2, 3, 5, 6, 7, 8, 9, 10

        def second(index, value):
            a = list(args[1])
            a[index] = value
            return [args[0], tuple(a)]

        def spoilt(member, value):
            if member == "stride":
                planes = list(args[1][FRAME])
                planes[0] = sa.SubPlane(planes[0], 0, 0, c["h"], c["w"], stride=c["w"] + value)
                return second(FRAME, planes)
            if member in ("nbx", "nby", "xb", "yb"):
                key = {"nbx": "x_num_blocks", "nby": "y_num_blocks", "xb": "xbsep_luma", "yb": "ybsep_luma"}[member]
                return second(PARAMS, dict(args[1][PARAMS], **{key: value}))
            return second({"h_range": RANGE, "shift": SHIFT, "ref_index": REF, "ext": EXT, "h_shift": HS}[member], value)

        for member, value in K.REFUSED_MEMBERS:
            with pytest.raises(sa.SchroHipError, match="entry 1"):
                ctx.hbm_level_batch(spoilt(member, value))
        # a hint field that is the output field; two entries with one field
        for call in (second(HINT, args[1][FIELD]), second(FIELD, args[0][FIELD])):
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                ctx.hbm_level_batch(call)
        ctx.synchronize()
        ent.block.check({s["field"]: ent.block[s["field"]].initial() for s in ent.specs})
    finally:
        ent.block.free()
