"""GPU: the hierarchical rough motion search on the device (rough_hint.hip) against tests/rough_hint_ref.py, record for
record: all 20 bytes of every record of every field, the records off the level's grid included.

Every plane and field of every test lies in a guarded block (tests/guard_lib.py): a byte written outside a field, or a
plane or hint field changed, fails the test that did it."""
import zlib

import numpy as np
import pytest

import analysis_ref as A
import guard_lib as G
import rough_hint_cases as K
import rough_hint_draws as D
import rough_hint_ref as R
import schroedinger_amd as sa

pytestmark = pytest.mark.gpu

MV = sa.MV_DTYPE.itemsize


def as_bytes(field):
    return np.ascontiguousarray(field).view(np.uint8).reshape(1, -1)


class Pictures:
    """The planes and fields of some pictures in one guarded block: per picture frame, ref (stride w + pad), the hint
    field (an input) and the field (written whole)."""

    def __init__(self, ctx, pictures, seed):
        self.ctx, self.pictures = ctx, pictures
        lay = G.Layout()
        self.specs = []
        for k, c in enumerate(pictures):
            n = c["nbx"] * c["nby"] * MV
            stride = c["w"] + c["pad"]
            self.specs.append(dict(
                frame=lay.plane(c["h"], c["w"], np.uint8, stride=stride, footprint=None, name="frame%d" % k, align=64, skew=c["pad"] % 4),
                ref=lay.plane(c["h"], c["w"], np.uint8, stride=stride, footprint=None, name="ref%d" % k, align=64, skew=(c["pad"] + 1) % 4),
                hint=lay.span(n, footprint=None, name="hint%d" % k, align=64, skew=4 * (k % 3)),
                field=lay.span(n, footprint=("bytes", n), name="field%d" % k, align=64, skew=4 * ((k + 1) % 3))))
        self.block = G.GuardedBlock(ctx, lay, seed=seed)
        for c, s in zip(pictures, self.specs):
            self.block[s["frame"]].upload(c["frame"])
            self.block[s["ref"]].upload(c["ref"])
            self.block[s["hint"]].upload(as_bytes(c["hint"]))

    def args(self):
        return [(self.block[s["frame"]], self.block[s["ref"]], c["ext"], K.params_of(c), c["shift"], c["dist"], c["ref_index"],
                 self.block[s["hint"]], self.block[s["field"]]) for c, s in zip(self.pictures, self.specs)]

    def run_and_check(self, fields):
        try:
            self.ctx.rough_hint_batch(self.args())
            self.ctx.synchronize()
            self.block.check({s["field"]: as_bytes(f) for s, f in zip(self.specs, fields)})
        finally:
            self.block.free()


def case_picture(name):
    frame, ref, hint = K.inputs(name)
    return dict(K.CASES[name], frame=frame, ref=ref, hint=hint)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_named_case(ctx, name):
    field, _ = K.expected(name)
    Pictures(ctx, [case_picture(name)], seed=zlib.crc32(name.encode()) & 0xffff).run_and_check([field])


def test_three_unlike_pictures_in_one_call(ctx):
    names = ["ref_1_shift2", "block_16x8", "shift3_odd"]
    assert len({(K.CASES[n]["shift"], K.CASES[n]["ref_index"]) for n in names}) == 3
    Pictures(ctx, [case_picture(n) for n in names], seed=3).run_and_check([K.expected(n)[0] for n in names])


@pytest.mark.parametrize("n", range(D.N_DRAWS))
def test_random_draw(ctx, n):
    Pictures(ctx, D.draw(n), seed=100 + n).run_and_check([f for f, _ in D.expected(n)])


# ---- the chain ------------------------------------------------------------------------------------------------------

def chain_params(w, h, xb=8, yb=8):
    """The blocks of the full picture (level 0), as the encoder lays them out."""
    return dict(x_num_blocks=-(-w // xb), y_num_blocks=-(-h // yb), xbsep_luma=xb, ybsep_luma=yb)


def chain_pictures(w, h, seed):
    frame = K.texture(w, h, seed)
    return frame, K.moved(frame, 5, -3, seed + 1)


_chain_reference = {}


def chain_reference(w, h, n_levels, ref_index, ext):
    """The fields of tests/rough_hint_ref.rough_scan on analysis_ref.pyramid, computed once per geometry."""
    key = (w, h, n_levels, ref_index, ext)
    if key not in _chain_reference:
        frame, ref = chain_pictures(w, h, 7000 + w)
        fields = R.rough_scan(A.pyramid(frame, n_levels), A.pyramid(ref, n_levels), chain_params(w, h), n_levels, ref_index, ext)
        _chain_reference[key] = (frame, ref, fields)
    return _chain_reference[key]


def device_pyramid(ctx, plane, n_levels, ext):
    """[level 0, level 1 .. n_levels]: DevicePlanes by Context.downsample_batch, each with `ext` samples of apron."""
    levels = [ctx.upload(plane)]
    src = levels[0]
    for _ in range(n_levels):
        h, w = (src.height + 1) // 2, (src.width + 1) // 2
        dst = ctx.plane(h + 2 * ext, w + 2 * ext, np.uint8)
        ctx.downsample_batch([(src, dst, ext)])
        levels.append(dst)
        src = sa.SubPlane(dst, ext, ext, h, w)
    return levels


@pytest.mark.parametrize("size", [(128, 96), (101, 75)])
@pytest.mark.parametrize("n_levels", [1, 2, 3, 4])
def test_chain_on_the_device_pyramid(ctx, size, n_levels):
    """The pyramid and the search never leave the device: downsample_batch, then rough_me_batch on its planes, both
    references of the picture as two chains of one launch; the fields are downloaded at the end."""
    (w, h), ext = size, 32 if n_levels == 3 else 0
    frame, ref, want0 = chain_reference(w, h, n_levels, 0, ext)
    want1 = chain_reference(w, h, n_levels, 1, ext)[2]
    P = chain_params(w, h)
    fl, rl = device_pyramid(ctx, frame, n_levels, ext), device_pyramid(ctx, ref, n_levels, ext)
    lay = G.Layout()
    n = P["x_num_blocks"] * P["y_num_blocks"] * MV
    specs = [[lay.span(n, footprint=("bytes", n), name="field_r%d_l%d" % (r, k + 1), align=64, skew=4 * r) for k in range(n_levels)]
             for r in (0, 1)]
    block = G.GuardedBlock(ctx, lay, seed=n_levels)
    try:
        levels = []
        for k in range(1, n_levels + 1):
            hh, ww = fl[k].height - 2 * ext, fl[k].width - 2 * ext
            levels.append((sa.SubPlane(fl[k], ext, ext, hh, ww), sa.SubPlane(rl[k], ext, ext, hh, ww), ext))
        ctx.rough_me_batch([(levels, P, r, [block[s] for s in specs[r]]) for r in (0, 1)])
        ctx.synchronize()
        block.check({specs[r][k]: as_bytes((want0, want1)[r][k + 1]) for r in (0, 1) for k in range(n_levels)})
    finally:
        block.free()
        for p in fl + rl:
            p.free()


@pytest.mark.parametrize("size,n_levels", [((128, 96), 3), ((101, 75), 4), ((101, 75), 1)])
def test_frame_layer_chain(ctx, size, n_levels):
    (w, h), ext = size, 32 if n_levels == 3 else 0
    frame, ref, want = chain_reference(w, h, n_levels, 0, ext)
    fl, rl = device_pyramid(ctx, frame, n_levels, ext), device_pyramid(ctx, ref, n_levels, ext)
    try:
        got = ctx.rough_scan(fl, rl, chain_params(w, h), 0, extension=ext)
        assert got[0] is None and len(got) == n_levels + 1
        for k in range(1, n_levels + 1):
            assert as_bytes(got[k]).tobytes() == as_bytes(want[k]).tobytes(), k
    finally:
        for p in fl + rl:
            p.free()


@pytest.mark.parametrize("name", ["partial_blocks", "ref_1_shift2", "beyond_the_picture"])
def test_frame_layer_hint_level(ctx, name):
    c = case_picture(name)
    ext = c["ext"]
    fa, fb = (ctx.upload(A.edgeextend(c[k], ext)) for k in ("frame", "ref"))
    try:
        got = ctx.rough_scan_hint(fa, fb, K.params_of(c), c["shift"], c["dist"], c["ref_index"], c["hint"], extension=ext)
        assert as_bytes(got).tobytes() == as_bytes(K.expected(name)[0]).tobytes()
    finally:
        fa.free()
        fb.free()


def test_a_refused_call_writes_nothing(ctx):
    """Refusals with a context: the second picture of the call is bad; neither field is touched."""
    good = case_picture(K.REFUSED_CASE)
    pics = Pictures(ctx, [good, dict(good)], seed=5)
    try:
        args = pics.args()
        FRAME, PARAMS, SHIFT, DIST, REF, HINT, FIELD = 0, 3, 4, 5, 6, 7, 8

        def second(index, value):
            a = list(args[1])
            a[index] = value
            return [args[0], tuple(a)]

        def spoilt(member, value):
            if member == "stride":
                return second(FRAME, sa.SubPlane(args[1][FRAME], 0, 0, good["h"], good["w"], stride=good["w"] + value))
            if member in ("nbx", "nby", "xb", "yb"):
                key = {"nbx": "x_num_blocks", "nby": "y_num_blocks", "xb": "xbsep_luma", "yb": "ybsep_luma"}[member]
                return second(PARAMS, dict(args[1][PARAMS], **{key: value}))
            return second({"dist": DIST, "shift": SHIFT, "ref_index": REF}[member], value)

        bad = [spoilt(member, value) for member, value in K.REFUSED_MEMBERS]
        for call in bad:
            with pytest.raises(sa.SchroHipError, match="picture 1"):
                ctx.rough_hint_batch(call)
        # a hint field that is the output field; two pictures with one field
        for call in (second(HINT, args[1][FIELD]), second(FIELD, args[0][FIELD])):
            with pytest.raises(sa.SchroHipError, match="overlaps"):
                ctx.rough_hint_batch(call)
        ctx.synchronize()
        pics.block.check({s["field"]: pics.block[s["field"]].initial() for s in pics.specs})
    finally:
        pics.block.free()
