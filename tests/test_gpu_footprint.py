"""GPU: every entry point writes its output region and nothing else, and reads nothing outside its inputs.

Each case puts every output and every input of one call in a guarded block (tests/guard_lib.py: seeded random bytes,
guards of at least max (4096, 2 x stride) bytes around and between the planes), runs the call once, checks the payloads
against the oracle and then checks that no byte outside the declared footprints changed -- inputs included.  The leads
and strides are chosen to send the planes to each kernel the dispatch picks between: 256-byte, 8- / 16-byte and
sample-aligned leads; rows without padding, rounded to 64 and with odd padding.  The random bytes in the inputs'
padding also make the oracle comparison fail for an output that gives weight to a byte outside its input.

The frame layer gets the same check on the allocation schro_hip_frame_new_and_alloc makes (Y, U, V back to back, each
rounded up to 256 bytes): the stride padding of every component and the gaps between them must keep their canary.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest

import guard_lib as G
import oracle_lib as O
import schroedinger_amd as sa
import synth
import test_gpu_dequant as TD
import test_gpu_lowdelay as TL
import test_gpu_obmc as TO
import test_gpu_pack as TP
from schroedinger_amd import _lib, frames
from test_gpu_mixed_batches import KINDS

pytestmark = pytest.mark.gpu

LEADS = {"a256": (256, 0), "a16": (64, 16), "a8": (64, 8)}      # (alignment, skew) of a plane's first byte


def r64(n):
    return (n + 63) // 64 * 64


def stride_of(kind, row, unit):
    """'tight': exactly the row bytes; 'r64': rounded to 64; 'odd': rounded to 64 plus an odd number of samples."""
    return {"tight": row, "r64": r64(row), "odd": r64(row) + 3 * unit}[kind]


def lead_of(name, unit):
    return LEADS[name] if name in LEADS else (256, unit)         # 'unit': the smallest alignment the call accepts


class Call:
    """The guarded planes of one call: inputs (uploaded, empty footprint) and outputs (footprint: their rectangle)."""

    def __init__(self, gap=0):
        self.L, self.uploads = G.Layout(gap), []

    def inp(self, a, stride="r64", lead="a256", name=None):
        a = np.ascontiguousarray(a)
        unit = a.dtype.itemsize
        s = self.L.plane(a.shape[0], a.shape[1], a.dtype, stride_of(stride, a.shape[1] * unit, unit),
                         *lead_of(lead, unit), footprint=None, name=name)
        self.uploads.append((s, a))
        return s

    def out(self, h, w, dtype, stride="r64", lead="a256", name=None, footprint="rect", init=None):
        unit = np.dtype(dtype).itemsize
        s = self.L.plane(h, w, dtype, stride_of(stride, w * unit, unit), *lead_of(lead, unit), footprint=footprint, name=name)
        if init is not None:
            self.uploads.append((s, init))
        return s

    def span(self, data, align=256, skew=0, name=None):
        s = self.L.span(len(data), align, skew, name=name)
        self.uploads.append((s, np.frombuffer(bytes(data), np.uint8).reshape(1, -1)))
        return s

    def build(self, ctx, seed):
        self.B = G.GuardedBlock(ctx, self.L, seed)
        for s, a in self.uploads:
            self.B[s].upload(a)
        return self.B

    def __getitem__(self, s):
        return self.B[s]

    def check(self, expected, extra=None):
        try:
            self.B.check(expected, extra)
        finally:
            self.B.free()


# ---- iiwt_batch ---------------------------------------------------------------------------------------------------

def coeffs(h, w, dtype, depth, filt, seed):
    return O.forward_iwt(synth.image_s(h, w, dtype, seed=seed), depth, filt)


def run_iiwt(ctx, planes, depth, filt, seed=1, gap=0):
    """planes: (h, w, dtype, src stride kind, src lead, dst stride kind, dst lead) -- one call, every plane in one block;
    gap: extra bytes between the regions."""
    c, todo = Call(gap), []
    for n, (h, w, dt, ss, sl, ds, dl) in enumerate(planes):
        co = coeffs(h, w, dt, depth, filt, seed + n)
        s = c.inp(co, ss, sl, name="src%d" % n)
        d = c.out(h, w, dt, ds, dl, name="dst%d" % n)
        todo.append((s, d, co))
    c.build(ctx, seed)
    ctx.iiwt_batch([(c[s], c[d]) for s, d, _ in todo], depth, filt)
    c.check({d: O.inverse_iwt(co, depth, filt) for _, d, co in todo})


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, 6])
def test_iiwt_register_small_tiles(ctx, filt):
    # s16, sub-band widths that are multiples of 4, 8-byte aligned: the register kernel; sizes around its tile borders
    for depth, (h, w) in [(1, (22, 24)), (1, (34, 504)), (1, (50, 520)), (2, (136, 248)), (3, (48, 64)), (4, (240, 320))]:
        for ss, sl, ds, dl in [("tight", "a256", "tight", "a8"), ("r64", "a8", "r64", "a16"), ("r64", "a16", "tight", "a256")]:
            run_iiwt(ctx, [(h, w, np.int16, ss, sl, ds, dl)], depth, filt, seed=h + w + depth)


def test_iiwt_register_large_tiles(ctx):
    # two 3840 x 2160 planes: level 0 has 2 x 8 x 135 = 2160 tiles of 248 columns x 8 row pairs -- at least the 2048
    # below which a level takes the small form (plane_iiwt.cpp, level_is_small)
    run_iiwt(ctx, [(2160, 3840, np.int16, "tight", "a256", "r64", "a8"), (2160, 3840, np.int16, "r64", "a16", "tight", "a256")],
             3, 0, seed=5)


@pytest.mark.parametrize("filt", range(7))
def test_iiwt_lds_kernels(ctx, filt):
    # s32; the fidelity filter; sub-band widths that are not multiples of 4; leads and strides of 2 bytes
    for depth in (1, 2, 3):
        run_iiwt(ctx, [(48, 72, np.int32, "tight", "unit", "odd", "a16"), (40, 104, np.int32, "r64", "a8", "tight", "a256")],
                 depth, filt, seed=30 + depth)
        run_iiwt(ctx, [(40, 104, np.int16, "odd", "a256", "tight", "unit"),
                       (16 << depth >> 1, 36 << depth >> 1, np.int16, "tight", "a8", "r64", "a8")], depth, filt, seed=40 + depth)


@pytest.mark.parametrize("filt", [3, 4])
def test_iiwt_haar_s32(ctx, filt):
    run_iiwt(ctx, [(40, 72, np.int32, "tight", "unit", "odd", "a256"), (18, 34, np.int32, "r64", "a8", "tight", "unit")], 1, filt)
    run_iiwt(ctx, [(64, 96, np.int32, "odd", "a256", "tight", "a16")], 2, filt)
    # depth 3, widths a multiple of 32, 16-byte aligned rows: iiwt_haar3_s32_kernel -- and beside it a plane that is not
    run_iiwt(ctx, [(72, 96, np.int32, "tight", "a16", "tight", "a256"), (264, 480, np.int32, "r64", "a256", "r64", "a16")], 3, filt)
    run_iiwt(ctx, [(72, 96, np.int32, "tight", "a16", "odd", "a8"), (48, 40, np.int32, "tight", "a256", "tight", "unit")], 3, filt)


def run_combine(ctx, h, w, depth, filt, dtype, oh, ow, with_pred, lead="a256", stride="r64", seed=3):
    c = Call()
    co = coeffs(h, w, dtype, depth, filt, seed)
    res = O.inverse_iwt(co, depth, filt).astype(np.int64)
    s = c.inp(co, stride, lead)
    pred = None
    if with_pred:
        pred = synth.picture_u8(oh, ow, seed=seed + 1, blur=False)
        p = c.L.plane(oh, ow, np.uint8, (ow + 7) // 8 * 8 if stride == "tight" else r64(ow) + 8, footprint=None, name="pred")
        c.uploads.append((p, pred))
    d = c.out(oh, ow, np.uint8, stride, lead if lead != "unit" else "a8", name="out")
    c.build(ctx, seed)
    ctx.iiwt_batch([(c[s], c[d], c[p] if with_pred else None)], depth, filt)
    want = np.clip(res[:oh, :ow] + (pred if with_pred else 128), 0, 255).astype(np.uint8)
    c.check({d: want})


@pytest.mark.parametrize("with_pred", [True, False])
def test_iiwt_combine_direct(ctx, with_pred):
    # s16, register filters, 8-byte aligned: the register kernel's combine epilogue; pictures inside the transform
    # whose width is no multiple of 8
    for (h, w, depth, filt, oh, ow) in [(64, 96, 2, 0, 61, 93), (144, 176, 3, 1, 141, 173), (240, 320, 3, 6, 233, 317),
                                        (48, 64, 1, 2, 47, 57), (1088, 1920, 3, 0, 1080, 1917)]:
        for stride in ("tight", "r64"):
            run_combine(ctx, h, w, depth, filt, np.int16, oh, ow, with_pred, stride=stride, seed=h + w)


@pytest.mark.parametrize("with_pred", [True, False])
def test_iiwt_combine_scratch_route(ctx, with_pred):
    # s32, the fidelity filter, an unaligned coefficient plane: a residual plane in the scratch and the convert kernel
    run_combine(ctx, 64, 96, 2, 0, np.int32, 61, 93, with_pred)
    run_combine(ctx, 64, 96, 3, 3, np.int32, 57, 90, with_pred, stride="odd")
    run_combine(ctx, 64, 96, 2, 5, np.int16, 63, 95, with_pred)
    run_combine(ctx, 64, 96, 2, 0, np.int16, 61, 93, with_pred, lead="unit")


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("filt", [0, 3, 5])
def test_iiwt_in_two_calls(ctx, filt, dtype):
    # the levels above 0 on the level-1 view into a guarded LL plane, then level 0 (the combine form) reading that LL
    # plane and a guarded prediction
    h, w, depth = 112, 208, 3
    c = Call()
    co = coeffs(h, w, dtype, depth, filt, 7)
    s = c.inp(co, "r64", "a256", name="coeffs")
    ll = c.out(h // 2, w // 2, dtype, "tight", "a8", name="ll")
    pred = synth.picture_u8(h - 3, w - 5, seed=8, blur=False)
    p = c.L.plane(h - 3, w - 5, np.uint8, r64(w - 5), footprint=None, name="pred")
    c.uploads.append((p, pred))
    d = c.out(h - 3, w - 5, np.uint8, "odd", "a256", name="out")
    c.build(ctx, 7)
    src = c[s]
    view = types.SimpleNamespace(ptr=src.ptr, stride=src.stride << 1, width=w >> 1, height=h >> 1, dtype=src.dtype)
    ctx.iiwt_batch([(view, c[ll])], depth - 1, filt)
    ll_want = O.inverse_iwt(np.ascontiguousarray(co[0::2, :w // 2]), depth - 1, filt)
    d.footprint = None                               # (the first call writes the LL plane alone)
    c.B.check({ll: ll_want})
    c.B.before = c.B.raw()                           # the LL plane is the second call's input, `out` its output
    ll.footprint, d.footprint = None, "rect"
    ctx.iiwt_batch([(src, c[d], c[p])], 1, filt, ll=[c[ll]])
    res = O.inverse_iwt(co, depth, filt).astype(np.int64)
    c.check({d: np.clip(res[:h - 3, :w - 5] + pred, 0, 255).astype(np.uint8)})


# ---- convert, add, shift right, DC prediction --------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_convert_u8(ctx, dtype):
    for (h, w, oh, ow) in [(48, 64, 45, 61), (1088, 1920, 1080, 1920), (9, 21, 9, 21), (34, 100, 33, 97)]:
        for ss, sl, ds, dl in [("r64", "a256", "tight", "a256"), ("odd", "unit", "odd", "unit"), ("tight", "a16", "r64", "a8")]:
            c = Call()
            a = synth.full_range(h, w, dtype, seed=h + w)
            s = c.inp(a, ss, sl)
            d = c.out(oh, ow, np.uint8, ds, dl)
            c.build(ctx, h)
            ctx.convert_u8_batch([(c[s], c[d])])
            c.check({d: O.convert_u8(a, ow, oh)})


@pytest.mark.parametrize("sdt", [np.int16, np.uint8])
def test_add(ctx, sdt):
    rng = np.random.default_rng(5)
    for (h, w) in ((48, 64), (37, 53), (5, 7), (270, 1920)):
        for ds, dl, ss, sl in [("r64", "a256", "tight", "a256"), ("odd", "unit", "odd", "unit"), ("tight", "a8", "r64", "a16")]:
            c = Call()
            dst = rng.integers(-32768, 32768, (h, w)).astype(np.int16)
            src = (rng.integers(-32768, 32768, (h + 2, w + 3)).astype(np.int16) if sdt == np.int16
                   else rng.integers(0, 256, (h + 2, w + 3)).astype(np.uint8))
            d = c.out(h, w, np.int16, ds, dl, init=dst)
            s = c.inp(src, ss, sl)
            c.build(ctx, w)
            ctx.add_batch([(c[d], c[s])])
            c.check({d: O.frame_add(dst, src)})


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_shift_right(ctx, dtype):
    c, todo = Call(), []
    for n, (h, w) in enumerate([(1, 1), (7, 13), (64, 520), (270, 481), (5, 24)]):
        for st, ld in [("tight", "a256"), ("odd", "unit"), ("r64", "a16")]:
            a = synth.full_range(h, w, dtype, seed=3 + n)
            todo.append((c.out(h, w, dtype, st, ld, init=a), a))
    c.build(ctx, 9)
    ctx.shift_right_batch([c[s] for s, _ in todo], 3)
    c.check({s: O.shift_right(a, 3) for s, a in todo})


@pytest.mark.parametrize("kernel", ["skew", "barrier"])
@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_dc_predict(ctx, dtype, kernel, monkeypatch):
    # the sizes of test_dc_predict_strips (dc_skew_kernel) and rows that are not whole 16-byte pieces; "barrier":
    # dc_predict_kernel (SCHRO_HIP_DC_SKEW=0, the experiments build)
    if kernel == "barrier":
        monkeypatch.setenv("SCHRO_HIP_DC_SKEW", "0")
    E = 16 // np.dtype(dtype).itemsize
    shapes = [(1, E), (3, 2 * E), (64, 64), (65, 136), (129, 5 * E), (540, 960), (1100, 40), (70, 16 * 40 + E),
              (63, 256), (128, 16 * 33), (66, 16 * 32 - E), (5, 7), (33, 3 * E + 1), (17, 1)]
    c, todo = Call(), []
    for n, (h, w) in enumerate(shapes):
        a = synth.full_range(h, w, dtype, seed=50 + n) if n % 2 else synth.image_s(h, w, dtype, seed=20 + n) * 5
        st, ld = [("tight", "a16"), ("r64", "a256"), ("odd", "unit")][n % 3]
        todo.append((c.out(h, w, dtype, st, ld, init=a), a))
    c.build(ctx, 11)
    ctx.dc_predict_batch([c[s] for s, _ in todo])
    c.check({s: O.dc_predict(a) for s, a in todo})


# ---- packers ------------------------------------------------------------------------------------------------------

PACK_LEADS = [("tight", "a256"), ("r64", "a16"), ("odd", "a8"), ("odd", "unit")]


def run_pack(ctx, call, cases, fmt_of, oracle, seed, gap=0):
    """cases: (planes, hs, vs, W, H, fmt); every source an input, every dst (H rows of the format's row bytes) an output."""
    c, jobs, want = Call(gap), [], {}
    for n, (pl, hs, vs, W, H, fmt) in enumerate(cases):
        src = [c.inp(p, "odd" if n % 2 else "r64", "a256" if n % 3 else "unit") for p in pl]
        st, ld = PACK_LEADS[n % len(PACK_LEADS)]
        d = c.out(H, G.packed_row_bytes(fmt, W), np.uint8, st, ld, name="dst%d" % n)
        jobs.append((src, hs, vs, d, W, H, fmt))
        want[d] = oracle(pl, hs, vs, W, H, fmt)
    c.build(ctx, seed)
    call([tuple([[c[s] for s in j[0]], j[1], j[2], c[j[3]]] + list(j[4:6]) + ([j[6]] if fmt_of else [])) for j in jobs])
    c.check(want)


@pytest.mark.parametrize("fmt", [sa.FORMAT_YUYV, sa.FORMAT_UYVY, sa.FORMAT_AYUV])
def test_pack_u8(ctx, fmt):
    cases = []
    for (w, h) in [(16, 8), (17, 9), (34, 20), (2, 2), (1, 1), (200, 37), (1030, 5)]:
        for hs, vs in [(0, 0), (1, 0), (1, 1)]:
            pl = [synth.picture_u8(h, w, seed=w), synth.picture_u8(-(-h >> vs), -(-w >> hs), seed=w + 1),
                  synth.picture_u8(-(-h >> vs), -(-w >> hs), seed=w + 2)]
            for (W, H) in [(w, h), (w + 5, h + 3), (max(w - 3, 1), max(h - 2, 1))]:
                if G.packed_row_bytes(fmt, W):
                    cases.append((pl, hs, vs, W, H, fmt))
    run_pack(ctx, ctx.pack_u8_batch, cases, True, lambda pl, hs, vs, W, H, f: O.pack_u8(pl, hs, vs, f, W, H), 21)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
def test_pack_v210(ctx, dtype):
    cases = []
    for (w, h) in [(12, 4), (13, 3), (6, 2), (1, 1), (50, 9), (96, 16), (1920, 8), (3842, 3)]:
        for (hs, vs) in ([(0, 0), (1, 0), (1, 1)] if dtype == np.uint8 else [(1, 0)]):
            pl = pack_planes(w, h, hs, vs, dtype, w + h)
            for (W, H) in [(w, h), (w + 7, h + 2), (max(w - 5, 1), max(h - 1, 1))]:
                cases.append((pl, hs, vs, W, H, sa.FORMAT_V210))
    run_pack(ctx, ctx.pack_v210_batch, cases, False, lambda pl, hs, vs, W, H, f: O.pack_v210(pl, hs, vs, W, H), 22)


def pack_planes(w, h, hs, vs, dtype, seed):
    return TP.planes(w, h, hs, vs, seed) if dtype == np.uint8 else TP.signed_planes(w, h, dtype, seed)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
@pytest.mark.parametrize("fmt,hs", [(sa.FORMAT_V216, 1), (sa.FORMAT_ARGB, 0), (sa.FORMAT_AY64, 0)])
def test_pack_wide(ctx, fmt, hs, dtype):
    cases = []
    for (w, h) in [(12, 4), (13, 3), (2, 2), (1, 1), (51, 9), (97, 16), (1921, 8), (3842, 3)]:
        pl = TP.wide_planes(w, h, hs, dtype, w + h)
        for (W, H) in [(w, h), (w + 7, h + 2), (max(w - 5, 1), max(h - 1, 1))]:
            if G.packed_row_bytes(fmt, W):
                cases.append((pl, hs, 0, W, H, fmt))
    run_pack(ctx, ctx.pack_wide_batch, cases, True, lambda pl, hs, vs, W, H, f: O.pack_wide(pl, hs, vs, W, H, f), 23)


@pytest.mark.parametrize("filt", [3, 4])
def test_iiwt_pack_v210(ctx, filt):
    # the fused iiwt_haar3_v210_kernel (s32 Haar, depth 3, 4:2:2, multiples of 48 x 8) and the two-pass route
    for (w, h, depth, dtype, ow, oh, f) in [(48, 8, 3, np.int32, None, None, filt), (1104, 72, 3, np.int32, None, None, filt),
                                            (96, 32, 2, np.int32, None, None, filt), (96, 32, 3, np.int16, None, None, filt),
                                            (96, 32, 3, np.int32, 90, 30, filt), (96, 32, 3, np.int32, None, None, 1)]:
        ow, oh = ow or w, oh or h
        for st, ld in [("tight", "a256"), ("odd", "a8")]:
            c = Call()
            dims = [(h, w), (h, w >> 1), (h, w >> 1)]
            co = [O.forward_iwt((synth.image_s(a, b, dtype, seed=5 + k).astype(np.int64) * 3).astype(dtype), depth, f)
                  for k, (a, b) in enumerate(dims)]
            src = [c.inp(x, "r64", "a256") for x in co]
            d = c.out(oh, G.packed_row_bytes(sa.FORMAT_V210, ow), np.uint8, st, ld)
            c.build(ctx, w + h)
            ctx.iiwt_pack_v210_batch([([c[s] for s in src], 1, 0, c[d], ow, oh)], depth, f)
            px = [O.inverse_iwt(x, depth, f) for x in co]
            want = O.pack_v210([p[:oh, :(ow if k == 0 else -(-ow >> 1))] for k, p in enumerate(px)], 1, 0, ow, oh)
            c.check({d: want})


# ---- low-delay slices, dequantisation ------------------------------------------------------------------------------

@pytest.mark.parametrize("bpp", [2, 4])
@pytest.mark.parametrize("geo", TL.GEOMETRIES, ids=lambda g: "%dx%d" % g[:2] if isinstance(g, tuple) else None)
def test_lowdelay(ctx, geo, bpp, slice_kernel):
    run_lowdelay(ctx, geo, bpp)


def run_lowdelay(ctx, geo, bpp, gap=0):
    w, h, chroma, depth, sw, sh, num, den, override = geo
    P = synth.lowdelay_params(w, h, chroma, depth, sw, sh, num, den)
    if override:
        P["n_horiz_slices"], P["n_vert_slices"] = override
    dt = np.int16 if bpp == 2 else np.int32
    c, pics = Call(gap), []
    for n in range(2):
        q = synth.quantised_planes(P, seed=w + depth + 11 * n, scale=0.7 + 0.4 * n)
        data = O.lowdelay_write(q, P, bpp, synth.lowdelay_base_index(P, seed=h + n, lo=0, hi=44), pad_bit=n & 1)
        sl = c.span(data.tobytes(), align=256, skew=n, name="slices%d" % n)
        st = ["r64", "odd", "tight"][(n + h) % 3]
        planes = [c.out(P["iwt_chroma_height"] if k else P["iwt_luma_height"], P["iwt_chroma_width"] if k else P["iwt_luma_width"],
                        dt, st if k != 1 else "tight", "a256" if k else ("unit" if n else "a16"), name="p%d.%d" % (n, k)) for k in range(3)]
        pics.append((sl, planes, data))
    B = c.build(ctx, w)
    ctx.lowdelay_batch([(TL.Offset(B[sl], 0, data.size), [B[p] for p in planes]) for sl, planes, data in pics], P)
    want = {}
    for sl, planes, data in pics:
        start = [B[p].initial().copy() for p in planes]     # what the oracle does not write keeps the canary
        O.lowdelay_decode(data, start, P)
        want.update(zip(planes, start))
    c.check(want)


slice_kernel = TL.slice_kernel


@pytest.mark.parametrize("dtype,arith", [(np.int16, 0), (np.int16, 1), (np.int32, 0)])
@pytest.mark.parametrize("use_plan", [False, True])
def test_dequant(ctx, dtype, arith, use_plan):
    # the footprint is the union of the codeblock rectangles, zero codeblocks included
    run_dequant(ctx, dtype, arith, use_plan, [(64, 96, 2, 100, 1), (144, 176, 3, 3000, 0), (48, 40, 1, 40000, 0),
                                              (96, 160, 3, 90, 1)], 11)


def run_dequant(ctx, dtype, arith, use_plan, shapes, seed, gap=0):
    """shapes: (h, w, depth, value span, intra) per plane of one call."""
    rng = np.random.default_rng(seed)
    it = np.dtype(dtype).itemsize
    c, todo = Call(gap), []
    for n, (h, w, depth, span, intra) in enumerate(shapes):
        quant = rng.integers(-span, span + 1, (h, w)).astype(np.int32)
        quant[rng.random((h, w)) < 0.5] = 0
        records = TD.synthetic_records(h, w, depth, rng)
        st, ld = [("r64", "a256"), ("odd", "unit"), ("tight", "a8"), ("odd", "a16")][n % 4]
        stride = stride_of(st, w * it, it)
        blob, cbs = TD.pack_codeblocks((h, w), it, stride, depth, quant, records)
        fp = [(cb[0], cb[1], cb[2] * it, cb[3]) for cb in cbs]
        d = c.L.plane(h, w, dtype, stride, *lead_of(ld, it), footprint=fp, name="dst%d" % n)
        v = c.span(blob.tobytes(), align=256, skew=0, name="values%d" % n)
        todo.append((d, v, cbs, intra, depth, quant, records))
    B = c.build(ctx, seed + 2)
    jobs = [(B[d], B[v], cbs, intra) for d, v, cbs, intra, *_ in todo]
    if use_plan:
        plan = ctx.dequant_plan(jobs, arith)
        plan.run(jobs)
        ctx.synchronize()
        plan.free()
    else:
        ctx.dequant_batch(jobs, arith)
    want = {}
    import dirac_stream as D
    for d, v, cbs, intra, depth, quant, records in todo:
        ref = B[d].initial().copy()
        for (index, x0, y0, x1, y1, zero, qi) in records:
            band, qb = D.subband_view(ref, depth, index), D.subband_view(quant, depth, index)
            if x1 > x0 and y1 > y0:
                O.dequant_codeblock(band[y0:y1, x0:x1], None if zero else qb[y0:y1, x0:x1], qi, intra, arith)
        want[d] = ref
    c.check(want)


# ---- upsample -----------------------------------------------------------------------------------------------------

class GuardedHp(sa.HpPlane):
    """A half-pel image in a guarded block: HpPlane's download, the block's memory."""

    def __init__(self, block, spec, height, width, pair, stride):
        self.ctx, self.dtype, self.pair = block.ctx, np.dtype(np.uint8), pair
        self.comp_height, self.comp_width = height, width
        self.height, self.width = 2 * height, 2 * width
        self.ptr, self.stride, self.nbytes = block.ptr + spec.offset, stride, spec.width
        # (the bands of 4 rows the library addresses lie inside the span the layout reserved)
        assert stride % 512 == 0 and stride * (-(-height // 4)) <= spec.width, (stride, height, spec.width)

    def free(self):
        pass


def hp_span(c, ctx, h, w, pair, footprint=True, name=None):
    """A span for the half-pel image of an h x w component (a pair image: of two); returns (spec, GuardedHp arguments)."""
    st = C.c_int(0)
    n = (ctx.lib.schro_hip_upsampled_pair_bytes if pair else ctx.lib.schro_hip_upsampled_bytes)(w, h, C.byref(st))
    return c.L.span(n, align=128, footprint=("bytes", n) if footprint else None, name=name, stride=st.value), (h, w, pair, st.value)


def check_hp(hp, want_planes, name):
    got = hp.download()
    got = got if hp.pair else (got,)
    errs = []
    for g, up in zip(got, want_planes):
        for pl in range(4):
            if not np.array_equal(g[pl >> 1::2, pl & 1::2], up.plane(pl)):
                errs.append("%s: half-pel plane %d differs from the oracle" % (name, pl))
    return errs


def test_upsample(ctx):
    # single and pair images in one call; widths that are no multiple of 16, heights that are no multiple of 4;
    # sources at every lead
    run_upsample(ctx, [(1, 1), (5, 7), (33, 47), (66, 130), (135, 241), (18, 16), (64, 200)], 17)


def run_upsample(ctx, sizes, seed, gap=0):
    """A single and a pair image of every (h, w) of `sizes`, all in one call."""
    c, todo = Call(gap), []
    for n, (h, w) in enumerate(sizes):
        a = synth.picture_u8(h, w, seed=n, blur=False)
        st, ld = [("tight", "unit"), ("odd", "a256"), ("r64", "a8")][n % 3]
        s = c.inp(a, st, ld)
        d, geo = hp_span(c, ctx, h, w, False, name="hp%d" % n)
        todo.append(((s,), d, geo, (a,)))
        b = synth.picture_u8(h, w, seed=100 + n, blur=False)
        su, sv = c.inp(b, "r64", "unit"), c.inp(a[::-1].copy(), st, "a16")
        dp, geo = hp_span(c, ctx, h, w, True, name="pair%d" % n)
        todo.append(((su, sv), dp, geo, (b, a[::-1].copy())))
    B = c.build(ctx, seed)
    hps = [(GuardedHp(B, d, *geo), src, pics) for src, d, geo, pics in todo]
    ctx.upsample_batch([((B[src[0]], B[src[1]]) if len(src) == 2 else B[src[0]], hp) for hp, src, _ in hps])
    errs = []
    for hp, _, pics in hps:
        errs += check_hp(hp, [O.UpComp(p) for p in pics], "hp")
    c.check({}, errs)


# ---- obmc_batch ---------------------------------------------------------------------------------------------------

class Alloc:
    """make_case's allocator: hands out the guarded planes planned for `out` and the residual, in order."""

    def __init__(self, block, planned):
        self.block, self.planned = block, list(planned)

    def __call__(self, role, height, width, dtype):
        r, s = self.planned.pop(0)
        assert r == role and (s.height, s.width, s.dtype) == (height, width, np.dtype(dtype)), (role, s.name)
        return self.block[s]


class GRef(TO.Ref):
    """A reference whose pictures (and half-pel images) live in a guarded block: inputs of the OBMC call."""

    def __init__(self, ctx, c, w, h, chroma, upsampled, pair, seed):
        self.w, self.h, self.chroma, self.upsampled = w, h, chroma, upsampled
        self.pair = pair = pair and upsampled and chroma[0] == 1
        self.np = [synth.picture_u8(*TO.comp_size(w, h, k, chroma)[::-1], seed=seed + k) for k in range(3)]
        self.up = [O.UpComp(p, upsample=upsampled) for p in self.np]
        self.src = [c.inp(p, "odd", "unit") for p in self.np]
        self.hp = []
        if upsampled:
            for k in range(3):
                cw, ch = TO.comp_size(w, h, k, chroma)
                if pair and k == 2:
                    break
                self.hp.append(hp_span(c, ctx, ch, cw, pair and k == 1, footprint=False))
        self.keep = []

    def bind(self, ctx, B):
        if not self.upsampled:
            self.dev = [B[s] for s in self.src]
            return
        hps = [GuardedHp(B, s, *geo) for s, geo in self.hp]
        jobs = [(B[self.src[0]], hps[0])]
        jobs += [((B[self.src[1]], B[self.src[2]]), hps[1])] if self.pair else [(B[self.src[1]], hps[1]), (B[self.src[2]], hps[2])]
        ctx.upsample_batch(jobs)
        self.dev = [hps[0], hps[1], hps[1]] if self.pair else hps


def obmc_case(ctx, kind, seed, out_stride="tight", out_lead="a256", gap=0, **over):
    """Plan, build and set up one picture of a KINDS entry in a guarded block; returns (jobs, finish)."""
    a = dict(KINDS[kind], **over)
    w, h, chroma, prec = a["w"], a["h"], a["chroma"], a["prec"]
    P = synth.motion_params(w, h, a["xblen"], a["xbsep"], prec, a["weights"], chroma, yblen=a.get("yblen"), ybsep=a.get("ybsep"))
    modes = (0.05, 0.45, 0.15, 0.35)
    if a.get("one_ref"):
        modes = (modes[0], sum(modes[1:]), 0, 0)
    mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], a["mv_range"], seed, modes)
    c = Call(gap)
    mvs = c.span(mv.tobytes(), name="vectors")
    refs = [GRef(ctx, c, w, h, chroma, prec > 0, a.get("pair", False), seed + 10 * (r + 1)) for r in range(1 if a.get("one_ref") else 2)]
    po, res_dt = a.get("prediction_only", 0), a.get("res_dtype", np.int16)
    planned = []
    for k in range(3):
        cw, ch = TO.comp_size(w, h, k, chroma)
        if not po and a.get("residual", True):
            it = np.dtype(res_dt).itemsize
            planned.append(("residual", c.L.plane(ch + 8, cw + 16, res_dt, stride_of("odd" if k else "r64", (cw + 16) * it, it),
                                                  256, 0 if k != 2 else it, footprint=None, name="residual%d" % k)))
        odt = np.int16 if po == 2 else np.uint8
        it = np.dtype(odt).itemsize
        planned.append(("out", c.L.plane(ch, cw, odt, stride_of(out_stride, cw * it, it), *lead_of(out_lead, it), name="out%d" % k)))
    B = c.build(ctx, seed)
    for r in refs:
        r.bind(ctx, B)
    if len(refs) == 1:
        refs.append(None)
    B.before = B.raw()                  # (the half-pel images are the call's inputs from here on)
    kw = {k: v for k, v in a.items() if k in ("res_dtype", "pair", "yblen", "ybsep", "prediction_only", "residual", "one_ref")}
    jobs, want, keep = TO.make_case(ctx, w, h, a["xblen"], a["xbsep"], prec, a["weights"], chroma, a["mv_range"], seed,
                                    refs=refs, mv=(mv, B[mvs]), alloc=Alloc(B, planned), **kw)

    def finish():
        c.check({o.spec: ref for ref, o, k in want})
    return jobs, finish


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_obmc_every_kind(ctx, kind):
    for n, (st, ld, over) in enumerate([("tight", "a256", {}), ("r64", "unit", {}), ("odd", "a8", {"w": 93, "h": 67}),
                                        ("tight", "unit", {"w": 133, "h": 69})]):
        jobs, finish = obmc_case(ctx, kind, 500 + n, st, ld, **over)
        ctx.obmc_batch(jobs)
        finish()


def test_obmc_several_kinds_in_one_call(ctx):
    rng = np.random.default_rng(77)
    names = sorted(KINDS)
    for rnd in range(4):
        cases = [obmc_case(ctx, names[int(i)], 600 + 10 * rnd + n, ["tight", "r64", "odd"][n % 3], ["a256", "unit", "a8"][(n + rnd) % 3])
                 for n, i in enumerate(rng.choice(len(names), 5, replace=False))]
        ctx.obmc_batch([j for jobs, _ in cases for j in jobs])
        for _, finish in cases:
            finish()


# ---- the frame layer ------------------------------------------------------------------------------------------------

class FrameGuard:
    """The allocation of a device frame (frame.cpp: Y, U, V back to back, each rounded up to 256 bytes).  With a seed it is
    filled with a canary; without one, the frame's bytes as they are (an input of the next call).  check () asserts that
    only the declared rows (or a half-pel image's bytes) changed."""

    def __init__(self, ctx, frame, seed=None):
        self.ctx, self.f = ctx, frame
        f = frame.c
        self.base = f.components[0].data
        self.parts = []
        end = 0
        for k in range(3):
            d = f.components[k]
            if d.data and d.length:
                off = d.data - self.base
                self.parts.append((k, off, d.stride, d.height, d.length))
                end = off + (d.length + 255) // 256 * 256
        self.total = end
        if seed is None:
            self.snapshot()
        else:
            self.before = G.canary(end, seed)
            sa.check(ctx.lib.schro_hip_upload_2d(ctx.h, self.base, end, self.before.ctypes.data_as(C.c_void_p), end, end, 1))

    def raw(self):
        out = np.empty(self.total, np.uint8)
        sa.check(self.ctx.lib.schro_hip_download_2d(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.total, self.base,
                                                    self.total, self.total, 1))
        return out

    def snapshot(self):
        """The frame's bytes now are what the next call must leave alone outside its footprint (after an upload)."""
        self.before = self.raw()

    def check(self, row_bytes=None):
        """row_bytes: per component what its call writes -- the bytes of each row, (bytes, rows) for the first rows only,
        None the whole component (a half-pel image); row_bytes None: nothing (an input)."""
        after = self.raw()
        L = G.Layout()
        for n, (k, off, stride, height, length) in enumerate(self.parts):
            rb = 0 if row_bytes is None else row_bytes[n]
            rows = height
            if isinstance(rb, tuple):
                rb, rows = rb
            fp = ("bytes", length) if rb is None else ([(0, stride, rb, rows)] if rb else None)
            L.specs.append(G.Spec("component%d" % k, off, height, max(stride, 1), np.uint8, max(stride, 1), fp, length))
        L.end = self.total
        mask = L.footprint()[:self.total]
        bad = np.flatnonzero((self.before != after) & ~mask)
        if bad.size:
            s, row, col = L.locate(int(bad[0]))
            raise AssertionError("STRAY WRITE -- %s: %d stray bytes, first at (row,col)=(%d,%d): canary 0x%02x, found 0x%02x"
                                 % (s.name, bad.size, row, col, self.before[bad[0]], after[bad[0]]))


def frame_dims(w, h, hs, vs):
    cw, ch = -(-w // (1 << hs)), -(-h // (1 << vs))
    return [(h, w), (ch, cw), (ch, cw)]


def check_half_pel(frame, pix):
    hp = frame.download()
    for k in range(3):
        upk = O.UpComp(pix[k])
        for pl in range(4):
            assert np.array_equal(hp[k][pl >> 1::2, pl & 1::2], upk.plane(pl)), (k, pl)


# (w, h, hs, vs): component lengths that are multiples of 256 (no gap between components) and ones that are not
FRAME_SIZES = [(128, 64, 1, 1), (176, 144, 1, 0), (97, 35, 1, 1), (120, 45, 0, 0)]


@pytest.mark.parametrize("w,h,hs,vs", FRAME_SIZES)
def test_frame_layer(ctx, w, h, hs, vs):
    lib = ctx.lib
    depth, filt = 3, 0
    pd = frame_dims(w, h, hs, vs)
    ih0, iw0 = -(-h // 16) * 16, -(-w // 16) * 16                   # (the chroma of the iwt-size frame holds its iwt size)
    iw = [(ih0, iw0), (ih0 >> vs, iw0 >> hs), (ih0 >> vs, iw0 >> hs)]
    fmt16, fmt8 = frames.frame_format(np.int16, hs, vs), frames.frame_format(np.uint8, hs, vs)
    params = frames.make_params(wavelet_filter_index=filt, transform_depth=depth, iwt_luma_width=iw[0][1],
                                iwt_luma_height=iw[0][0], iwt_chroma_width=iw[1][1], iwt_chroma_height=iw[1][0])
    coeffs = [O.forward_iwt(synth.image_s(a, b, np.int16, seed=3 + k), depth, filt) for k, (a, b) in enumerate(iw)]
    frame = frames.DeviceFrame(ctx, fmt16, iw[0][1], iw[0][0])
    row16 = [2 * b for a, b in iw]
    row8 = [b for a, b in pd]
    g = FrameGuard(ctx, frame, 1)
    sa.check(lib.schro_frame_inverse_iwt_transform_hip(frame.ptr(), frames.HostFrame(coeffs, hs, vs).ptr(), C.byref(params)))
    res = [O.inverse_iwt(co, depth, filt) for co in coeffs]
    assert all(np.array_equal(a, b) for a, b in zip(frame.download(), res))
    g.check(row16)

    # the transform from a device transform frame, which must stay untouched
    tf = frames.DeviceFrame(ctx, fmt16, iw[0][1], iw[0][0])
    FrameGuard(ctx, tf, 2)
    tf.upload(frames.HostFrame(coeffs, hs, vs))
    gt = FrameGuard(ctx, tf)
    frame2 = frames.DeviceFrame(ctx, fmt16, iw[0][1], iw[0][0])
    g2 = FrameGuard(ctx, frame2, 3)
    sa.check(lib.schro_frame_inverse_iwt_transform_hip(frame2.ptr(), tf.ptr(), C.byref(params)))
    assert all(np.array_equal(a, b) for a, b in zip(frame2.download(), res))
    g2.check(row16)
    gt.check()

    # shift right in place, then convert to u8 (planar) and the u8 picture to a packed frame
    sh = [O.shift_right(r, 1) for r in res]
    FrameGuard(ctx, frame2, 4)
    frame2.upload(frames.HostFrame(res, hs, vs))         # (the guard refilled the frame: the residual again)
    g2 = FrameGuard(ctx, frame2)
    sa.check(lib.schro_hipframe_shift_right(frame2.ptr(), 1))
    assert all(np.array_equal(a, b) for a, b in zip(frame2.download(), sh))
    g2.check(row16)
    out = frames.DeviceFrame(ctx, fmt8, w, h)
    g3 = FrameGuard(ctx, out, 4)
    sa.check(lib.schro_hipframe_convert(out.ptr(), frame2.ptr()))
    pix = [O.convert_u8(s, b, a) for s, (a, b) in zip(sh, pd)]
    assert all(np.array_equal(a, b) for a, b in zip(out.download(), pix))
    g3.check(row8)
    if (hs, vs) == (1, 0) or (hs, vs) == (0, 0):
        pk_fmt = sa.FORMAT_UYVY if hs else sa.FORMAT_AYUV
        packed = frames.DeviceFrame(ctx, pk_fmt, w, h)
        g4 = FrameGuard(ctx, packed, 5)
        sa.check(lib.schro_hipframe_convert(packed.ptr(), out.ptr()))
        assert np.array_equal(packed.download(), O.pack_u8(pix, hs, vs, pk_fmt, w, h))
        g4.check([G.packed_row_bytes(pk_fmt, w)])
        packed.unref()

    # add a u8 picture to the s16 frame
    FrameGuard(ctx, frame2, 6)
    frame2.upload(frames.HostFrame(res, hs, vs))
    g2 = FrameGuard(ctx, frame2)
    sa.check(lib.schro_hipframe_add(frame2.ptr(), out.ptr()))
    got = frame2.download()
    for k, (a, b) in enumerate(pd):
        want = res[k].copy()
        want[:a, :b] = O.frame_add(res[k][:a, :b], pix[k])
        assert np.array_equal(got[k], want), k
    g2.check(row16)

    # the half-pel images of the u8 picture (single luma, chroma as one pair image where hs == 1): the two-argument form,
    # and the one-argument form that finds its source in virt_frame1
    up = frames.DeviceFrame(ctx, fmt8, w, h, upsampled=True)
    g5 = FrameGuard(ctx, up, 7)
    sa.check(lib.schro_upsampled_hipframe_upsample(up.ptr(), out.ptr()))
    check_half_pel(up, pix)
    g5.check([None] * len(g5.parts))
    up2 = frames.DeviceFrame(ctx, fmt8, w, h, upsampled=True)
    up2.c.virt_frame1 = out.p
    g5b = FrameGuard(ctx, up2, 17)
    sa.check(lib.schro_upsampled_hipframe_upsample_inplace(up2.ptr()))
    check_half_pel(up2, pix)
    g5b.check([None] * len(g5b.parts))
    up2.c.virt_frame1 = None

    # OBMC render into a u8 frame with the residual frame added (schro_motion_render_hip, add TRUE); the references and
    # the residual frame are inputs
    prec = 1
    P = synth.motion_params(w, h, 12, 8, prec, (1, 1, 1), (hs, vs))
    mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], 24, seed=4)
    op = O.MotionParams(**P)
    mp = frames.make_params(wavelet_filter_index=filt, transform_depth=depth, iwt_luma_width=iw[0][1],
                            iwt_luma_height=iw[0][0], iwt_chroma_width=iw[1][1], iwt_chroma_height=iw[1][0], num_refs=2,
                            xblen_luma=12, yblen_luma=12, xbsep_luma=8, ybsep_luma=8, mv_precision=prec, picture_weight_bits=1,
                            picture_weight_1=1, picture_weight_2=1, x_num_blocks=P["x_num_blocks"], y_num_blocks=P["y_num_blocks"])
    frame2.upload(frames.HostFrame(res, hs, vs))
    gr = FrameGuard(ctx, frame2)
    g5 = FrameGuard(ctx, up)
    rendered = frames.DeviceFrame(ctx, fmt8, w, h)
    g6 = FrameGuard(ctx, rendered, 8)
    motion = _lib.Motion(up.ptr(), up.ptr(), mv.ctypes.data, C.pointer(mp))
    sa.check(lib.schro_motion_render_hip(C.byref(motion), None, frame2.ptr(), 1, rendered.ptr()))
    got = rendered.download()
    want_pic = [O.motion_render(mv, op, k, O.UpComp(pix[k]), O.UpComp(pix[k]), res[k], b, a) for k, (a, b) in enumerate(pd)]
    for k in range(3):
        assert np.array_equal(got[k], want_pic[k]), k
    g6.check(row8)
    gr.check()
    g5.check()

    # the prediction alone (add FALSE): into a u8 frame, and into an S16 frame of the transform's size (prediction - 128
    # over the picture the references cover; the rest of the frame keeps its bytes)
    zero = [np.zeros((a, b), np.int16) for a, b in pd]
    pred = frames.DeviceFrame(ctx, fmt8, w, h)
    g7 = FrameGuard(ctx, pred, 9)
    sa.check(lib.schro_motion_render_hip(C.byref(motion), pred.ptr(), None, 0, None))
    want_pred = [O.motion_render(mv, op, k, O.UpComp(pix[k]), O.UpComp(pix[k]), zero[k], b, a) for k, (a, b) in enumerate(pd)]
    assert all(np.array_equal(a, b) for a, b in zip(pred.download(), want_pred))
    g7.check(row8)
    g5.check()
    mc_tmp = frames.DeviceFrame(ctx, fmt16, iw[0][1], iw[0][0])
    g8 = FrameGuard(ctx, mc_tmp, 10)
    sa.check(lib.schro_motion_render_hip(C.byref(motion), mc_tmp.ptr(), None, 0, None))
    got = mc_tmp.download()
    for k, (a, b) in enumerate(pd):
        acc = O.motion_render(mv, op, k, O.UpComp(pix[k]), O.UpComp(pix[k]), zero[k], b, a, return_acc=True)[1]
        assert np.array_equal(got[k][:a, :b], O.rrshift6_s16(acc)), k
    g8.check([(2 * b, a) for a, b in pd])
    g5.check()

    # the transform and x_combine's add in one call (the device transform frame and the prediction are inputs), and the
    # intra form (+ 128)
    combined = frames.DeviceFrame(ctx, fmt8, w, h)
    gp, gt = FrameGuard(ctx, pred), FrameGuard(ctx, tf)
    for n, (prediction, want) in enumerate(((pred, want_pic), (None, [O.convert_u8(r, b, a) for r, (a, b) in zip(res, pd)]))):
        g9 = FrameGuard(ctx, combined, 11 + n)
        sa.check(lib.schro_frame_inverse_iwt_transform_combine_hip(combined.ptr(), tf.ptr(), C.byref(mp),
                                                                   prediction.ptr() if prediction else None))
        got = combined.download()
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (k, n)
        g9.check(row8)
        gp.check()
        gt.check()
    for f in (frame, tf, frame2, out, up, up2, rendered, pred, mc_tmp, combined):
        f.unref()


@pytest.mark.parametrize("w,h,dtype,filt,depth", [(96, 48, np.int32, 3, 3), (1008, 40, np.int32, 3, 3), (96, 48, np.int16, 0, 2),
                                                  (100, 36, np.int32, 4, 3)])
def test_frame_layer_transform_into_v210(ctx, w, h, dtype, filt, depth):
    # schro_frame_inverse_iwt_transform_convert_hip: the fused Haar + v210 kernel (s32, depth 3, multiples of 48 x 8) and
    # the two-pass route (whose pixel frame is the library's own); only the packed rows change, the transform frame not
    lib = ctx.lib
    iw, ih = -(-w // (1 << depth)) * (1 << depth), -(-h // (1 << depth)) * (1 << depth)
    icw = -(-(-(-w // 2)) // (1 << depth)) * (1 << depth)
    iw = max(iw, icw << 1)
    icw = iw >> 1
    co = [O.forward_iwt((synth.image_s(a, b, dtype, seed=11 + k).astype(np.int64) * 5).astype(dtype), depth, filt)
          for k, (a, b) in enumerate([(ih, iw), (ih, icw), (ih, icw)])]
    params = frames.make_params(wavelet_filter_index=filt, transform_depth=depth, iwt_luma_width=iw, iwt_luma_height=ih,
                                iwt_chroma_width=icw, iwt_chroma_height=ih, num_refs=0)
    tf = frames.DeviceFrame(ctx, frames.frame_format(dtype, 1, 0), iw, ih)
    FrameGuard(ctx, tf, 1)
    tf.upload(frames.HostFrame(co, 1, 0))
    gt = FrameGuard(ctx, tf)
    px = [O.inverse_iwt(c, depth, filt) for c in co]
    want = O.pack_v210([px[0][:h, :w], px[1][:h, :-(-w // 2)], px[2][:h, :-(-w // 2)]], 1, 0, w, h)
    out = frames.DeviceFrame(ctx, sa.FORMAT_V210, w, h)
    g = FrameGuard(ctx, out, 2)
    sa.check(lib.schro_frame_inverse_iwt_transform_convert_hip(out.ptr(), tf.ptr(), C.byref(params)))
    assert np.array_equal(out.download(), want)
    g.check([G.packed_row_bytes(sa.FORMAT_V210, w)])
    gt.check()
    out.unref()
    tf.unref()


@pytest.mark.parametrize("dtype,num_refs", [(np.int16, 0), (np.int16, 1), (np.int32, 0)])
def test_frame_layer_dequantise(ctx, dtype, num_refs):
    # schro_hipframe_dequantise fills the transform frame's rows completely (zero codeblocks zero-filled) and nothing else
    import dirac_stream as D
    lib = ctx.lib
    rng = np.random.default_rng(3 + num_refs)
    intra = num_refs == 0
    for (iw, ih, depth, hs, vs) in [(96, 64, 2, 1, 1), (176, 72, 3, 1, 0), (120, 40, 3, 0, 0)]:
        dims = [(ih, iw), (ih >> vs, iw >> hs), (ih >> vs, iw >> hs)]
        tf = frames.DeviceFrame(ctx, frames.frame_format(dtype, hs, vs), iw, ih)
        g = FrameGuard(ctx, tf, iw)
        params = frames.make_params(transform_depth=depth, num_refs=num_refs, iwt_luma_width=iw, iwt_luma_height=ih,
                                    iwt_chroma_width=iw >> hs, iwt_chroma_height=ih >> vs)
        qp = _lib.QuantisedPicture()
        keep, want = [], []
        for k, (h, w) in enumerate(dims):
            quant = rng.integers(-300, 301, (h, w)).astype(np.int32)
            quant[rng.random((h, w)) < 0.6] = 0
            records = TD.synthetic_records(h, w, depth, rng)
            blob, cbs = TD.pack_codeblocks((h, w), np.dtype(dtype).itemsize, tf.c.components[k].stride, depth, quant, records)
            tab = sa.Context.codeblock_table(cbs)
            qp.codeblocks[k] = C.cast(tab, C.POINTER(_lib.Codeblock))
            qp.ncodeblocks[k] = len(cbs)
            qp.values[k] = blob.ctypes.data
            qp.values_bytes[k] = blob.size
            keep += [tab, blob]
            ref = np.zeros((h, w), dtype)
            for (index, x0, y0, x1, y1, zero, qi) in records:
                band, qb = D.subband_view(ref, depth, index), D.subband_view(quant, depth, index)
                if x1 > x0 and y1 > y0:
                    O.dequant_codeblock(band[y0:y1, x0:x1], None if zero else qb[y0:y1, x0:x1], qi, 1 if intra else 0, 0)
            if intra:
                ll = D.subband_view(ref, depth, 0)
                ll[...] = O.dc_predict(ll)
            want.append(ref)
        qp.values_on_device = 0
        sa.check(lib.schro_hipframe_dequantise(tf.ptr(), C.byref(qp), C.byref(params)))
        got = tf.download()
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (iw, ih, k)
        g.check([w * np.dtype(dtype).itemsize for h, w in dims])
        tf.unref()


@pytest.mark.parametrize("bpp", [2, 4])
def test_frame_layer_lowdelay(ctx, bpp):
    w, h = 160, 96
    for chroma in ((1, 0), (1, 1)):
        P = synth.lowdelay_params(w, h, chroma, 3, 16, 16, 400)
        fmt = frames.frame_format(np.int16 if bpp == 2 else np.int32, *chroma)
        q = synth.quantised_planes(P, seed=12 + bpp, scale=1.1)
        data = O.lowdelay_write(q, P, bpp, synth.lowdelay_base_index(P, seed=3, lo=0, hi=20))
        tf = frames.DeviceFrame(ctx, fmt, P["iwt_luma_width"], P["iwt_luma_height"])
        g = FrameGuard(ctx, tf, bpp)
        sa.check(ctx.lib.schro_hip_decode_lowdelay_transform_data(tf.ptr(), data.ctypes.data_as(C.c_void_p), data.size,
                                                                 C.byref(ctx.lowdelay_params(P))))
        want = TL.decode_cpu(data, P, bpp)
        got = tf.download()
        for k in range(3):
            assert np.array_equal(got[k], want[k]), k
        g.check([tf.c.components[k].width * bpp for k in range(3)])
        tf.unref()


# ---- a seeded random draw --------------------------------------------------------------------------------------------

DRAW_KINDS = ["iiwt", "convert", "add", "dc", "pack_u8", "pack_v210", "pack_wide", "lowdelay", "dequant", "upsample", "obmc"]


def test_random_footprints(ctx):
    """SCHRO_FUZZ_SCALE x 22 draws (default 1) of an entry point of the tests above with random geometry, leads, strides and
    gaps between the regions; SCHRO_FUZZ_SEED picks the draw (as tests/test_gpu_fuzz.py)."""
    scale = int(os.environ.get("SCHRO_FUZZ_SCALE", "1"))
    seed = int(os.environ.get("SCHRO_FUZZ_SEED", "20261015"))
    rng = np.random.default_rng(seed)
    strides, leads = ["tight", "r64", "odd"], ["a256", "a16", "a8", "unit"]
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    for n in range(22 * scale):
        kind = DRAW_KINDS[n % len(DRAW_KINDS)] if n < len(DRAW_KINDS) else pick(DRAW_KINDS)
        st, ld = pick(strides), pick(leads)
        gap = int(pick([0, 0, 1, 7, 64, 300, 4096 + 13]))
        where = "draw %d (seed %d): %s %s %s gap %d" % (n, seed, kind, st, ld, gap)
        try:
            if kind == "iiwt":
                depth = int(rng.integers(1, 5))
                dt = pick([np.int16, np.int32])
                h, w = (int(rng.integers(1, 40)) << depth, int(rng.integers(1, 60)) << depth)
                run_iiwt(ctx, [(h, w, dt, pick(strides), pick(leads), st, ld)], depth, int(rng.integers(7)), seed=n, gap=gap)
            elif kind == "convert":
                dt = pick([np.int16, np.int32])
                h, w = int(rng.integers(1, 200)), int(rng.integers(1, 300))
                c = Call(gap)
                a = synth.full_range(h, w, dt, seed=n)
                s = c.inp(a, pick(strides), pick(leads))
                oh, ow = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
                d = c.out(oh, ow, np.uint8, st, ld)
                c.build(ctx, n)
                ctx.convert_u8_batch([(c[s], c[d])])
                c.check({d: O.convert_u8(a, ow, oh)})
            elif kind == "add":
                h, w = int(rng.integers(1, 200)), int(rng.integers(1, 300))
                c = Call(gap)
                dst = rng.integers(-32768, 32768, (h, w)).astype(np.int16)
                src = rng.integers(0, 256, (h, w)).astype(np.uint8) if rng.integers(2) else rng.integers(-32768, 32768, (h, w)).astype(np.int16)
                d = c.out(h, w, np.int16, st, ld, init=dst)
                s = c.inp(src, pick(strides), pick(leads))
                c.build(ctx, n)
                ctx.add_batch([(c[d], c[s])])
                c.check({d: O.frame_add(dst, src)})
            elif kind == "dc":
                dt = pick([np.int16, np.int32])
                h, w = int(rng.integers(1, 300)), int(rng.integers(1, 400))
                c = Call(gap)
                a = synth.full_range(h, w, dt, seed=n)
                d = c.out(h, w, dt, st, ld, init=a)
                c.build(ctx, n)
                ctx.dc_predict_batch([c[d]])
                c.check({d: O.dc_predict(a)})
            elif kind.startswith("pack"):
                w, h = int(rng.integers(1, 300)), int(rng.integers(1, 20))
                if kind == "pack_u8":
                    fmt, (hs, vs), dt = pick([sa.FORMAT_YUYV, sa.FORMAT_UYVY, sa.FORMAT_AYUV]), pick([(0, 0), (1, 0), (1, 1)]), np.uint8
                elif kind == "pack_v210":
                    dt = pick([np.uint8, np.int16, np.int32])
                    fmt, (hs, vs) = sa.FORMAT_V210, (pick([(0, 0), (1, 0), (1, 1)]) if dt == np.uint8 else (1, 0))
                else:
                    dt = pick([np.uint8, np.int16, np.int32])
                    fmt = pick([sa.FORMAT_V216, sa.FORMAT_ARGB, sa.FORMAT_AY64])
                    hs, vs = (1 if fmt == sa.FORMAT_V216 else 0), 0
                pl = (TP.wide_planes(w, h, hs, dt, n) if kind == "pack_wide" else pack_planes(w, h, hs, vs, dt, n))
                W, H = (w, h) if rng.integers(2) else (w + int(rng.integers(0, 9)), h + int(rng.integers(0, 4)))
                if G.packed_row_bytes(fmt, W):
                    call, oracle, fmt_of = {
                        "pack_u8": (ctx.pack_u8_batch, lambda pl, hs, vs, W, H, f: O.pack_u8(pl, hs, vs, f, W, H), True),
                        "pack_v210": (ctx.pack_v210_batch, lambda pl, hs, vs, W, H, f: O.pack_v210(pl, hs, vs, W, H), False),
                        "pack_wide": (ctx.pack_wide_batch, lambda pl, hs, vs, W, H, f: O.pack_wide(pl, hs, vs, W, H, f), True)}[kind]
                    run_pack(ctx, call, [(pl, hs, vs, W, H, fmt)], fmt_of, oracle, n, gap=gap)
            elif kind == "lowdelay":
                run_lowdelay(ctx, pick(TL.GEOMETRIES), pick([2, 4]), gap=gap)
            elif kind == "dequant":
                depth = int(rng.integers(1, 4))
                # (sub-bands of at least 5 x 5 samples: as many as synthetic_records cuts them into at most)
                shapes = [(int(rng.integers(5, 12)) << depth, int(rng.integers(5, 24)) << depth, depth,
                           int(pick([90, 3000, 40000])), int(rng.integers(2))) for _ in range(int(rng.integers(1, 4)))]
                dt, arith = pick([(np.int16, 0), (np.int16, 1), (np.int32, 0)])
                run_dequant(ctx, dt, arith, bool(rng.integers(2)), shapes, n, gap=gap)
            elif kind == "upsample":
                run_upsample(ctx, [(int(rng.integers(1, 80)), int(rng.integers(1, 300))) for _ in range(int(rng.integers(1, 4)))],
                             n, gap=gap)
            else:
                name = pick(sorted(KINDS))
                over = {"w": int(rng.integers(66, 160)), "h": int(rng.integers(66, 90))}
                jobs, finish = obmc_case(ctx, name, 900 + n, st, ld, gap=gap, **over)
                ctx.obmc_batch(jobs)
                finish()
        except AssertionError as e:
            raise AssertionError("%s: %s" % (where, e)) from e


# ---- the SAD scan ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tables", [True, False], ids=["tables", "no_tables"])
@pytest.mark.parametrize("skew", [0, 1, 2, 3])
def test_metric_scan(ctx, skew, tables):
    """schro_hip_metric_scan_batch through the C ABI, `results` and `metrics` the test's own memory: 16 bytes per scan, and of
    a scan's table of 42 * 42 entries only the first scan_width * scan_height (include/schro_hip.h); nothing else, also
    with metrics = NULL.  Two pictures with 1 and 7 scans (no multiples of the four scans per workgroup: the last
    workgroup's idle waves), planes at every byte alignment with strides that are no multiple of 4."""
    import analysis_ref as A
    T = sa.LIMIT_METRIC_SCAN ** 2
    ext = 8
    pics = [(37, 29, [dict(x=8, y=8, block_width=8, block_height=8, ref_x=6, ref_y=5, scan_width=5, scan_height=7, gi=4, gj=0)]),
            (70, 50, [dict(x=0, y=0, block_width=16, block_height=16, ref_x=-8, ref_y=-8, scan_width=17, scan_height=17, gi=8, gj=8),
                      dict(x=20, y=10, block_width=0, block_height=4, ref_x=18, ref_y=8, scan_width=5, scan_height=5, gi=2, gj=2),
                      dict(x=6, y=2, block_width=64, block_height=48, ref_x=-6, ref_y=-8, scan_width=19, scan_height=17, gi=0, gj=16),
                      dict(x=33, y=21, block_width=5, block_height=3, ref_x=13, ref_y=20, scan_width=42, scan_height=1, gi=41, gj=0),
                      dict(x=12, y=1, block_width=1, block_height=1, ref_x=12, ref_y=1, scan_width=1, scan_height=1, gi=0, gj=0),
                      dict(x=40, y=30, block_width=13, block_height=9, ref_x=30, ref_y=8, scan_width=1, scan_height=42, gi=0, gj=21),
                      dict(x=3, y=4, block_width=7, block_height=64 - 18, ref_x=-7, ref_y=-8, scan_width=42, scan_height=20, gi=10, gj=12)])]
    L, todo = G.Layout(), []
    for n, (w, h, dicts) in enumerate(pics):
        scans = np.zeros(len(dicts), sa.SCAN_DTYPE)
        for k, (s, d) in enumerate(zip(scans, dicts)):
            for key in ("x", "y", "block_width", "block_height", "ref_x", "ref_y", "scan_width", "scan_height"):
                s[key] = d[key]
            s["gravity_x"], s["gravity_y"] = d["ref_x"] + d["gi"] - d["x"], d["ref_y"] + d["gj"] - d["y"]
            s["dx"], s["dy"] = 100 + k, -100 - k
        f = L.plane(h, w, np.uint8, stride=w + 5 + 2 * n, align=64, skew=skew, footprint=None, name="frame%d" % n)
        r = L.plane(h, w, np.uint8, stride=w + 1 + 2 * n, align=64, skew=(skew + 1 + n) & 3, footprint=None, name="ref%d" % n)
        res = L.span(16 * len(scans), align=16, footprint=("bytes", 16 * len(scans)), name="results%d" % n)
        met = L.span(4 * T * len(scans), align=4, name="metrics%d" % n,
                     footprint=[(k * T * 4, 0, 4 * int(s["scan_width"]) * int(s["scan_height"]), 1) for k, s in enumerate(scans)]) if tables else None
        todo.append((f, r, res, met, scans, A.picture(w, h, 80 + n + skew), A.picture(w, h, 90 + n + skew)))
        assert (w + 5 + 2 * n) % 4 and (w + 1 + 2 * n) % 4
    B = G.GuardedBlock(ctx, L, seed=31 + skew)
    try:
        arr = (_lib.MetricScanPicture * len(todo))()
        for a, (f, r, res, met, scans, frame, ref) in zip(arr, todo):
            B[f].upload(frame)
            B[r].upload(ref)
            a.frame, a.frame_stride, a.ref, a.ref_stride = B[f].ptr, f.stride, B[r].ptr, r.stride
            a.width, a.height, a.extension = f.width, f.height, ext
            a.scans, a.nscans = scans.ctypes.data_as(C.POINTER(_lib.MetricScan)), len(scans)
            a.results, a.metrics = B[res].ptr, B[met].ptr if met is not None else None
        sa.check(ctx.lib.schro_hip_metric_scan_batch(ctx.h, arr, len(todo)))
        ctx.synchronize()
        want = {}
        for (f, r, res, met, scans, frame, ref) in todo:
            want_r = np.zeros(len(scans), sa.SCAN_RESULT_DTYPE)
            want_m = B[met].initial().copy().view(np.uint32).reshape(len(scans), T) if met is not None else None
            for k, s in enumerate(scans):
                m = A.do_scan(frame, ref, s)
                want_r[k] = A.get_min(m, s) + (0,)
                if want_m is not None:
                    want_m[k, :m.size] = m
            want[res] = want_r.view(np.uint8).reshape(1, -1)
            if met is not None:
                want[met] = want_m.view(np.uint8).reshape(1, -1)
        B.check(want)
    finally:
        B.free()
