"""The named cases of tests/test_gpu_split2.py: inputs, and the expected motion field, superblock table and metric table
from tests/split2_ref.py (computed once per case and process).  Pictures run from 24 x 16 to 104 x 80.  The `want` tuple
of a case says what it is there for; `expected` asserts it on the CPU (tests/test_split2_ref.py walks the cases), so a
case that stops exercising its point fails there.

A "mixed" picture has four quarters: top left reference 1 predicts well and reference 2 badly, top right the other way
round, bottom left both carry independent noise (their average is the better prediction), bottom right the source is flat
and the references are unrelated texture (DC).  With one reference the top right quarter is simply predicted badly.

One want differs from the issue.  It asks for an INSIDE block with an outside neighbour in its own superblock, and another
with one in a different superblock.  No such block exists: a block is outside when x * xbsep >= width or y * ybsep >=
height, a block's neighbours are at x - 1 and y - 1, and x * xbsep < width implies (x - 1) * xbsep < width.  Only outside
blocks have outside neighbours.  What is asserted instead: `inside_with_outside_neighbour` is 0 on every case and draw,
and an OUTSIDE block has an outside neighbour in its own superblock (it sees the working form) and another has one in a
different superblock (it sees the final form) -- and the working forms do differ from the final ones (pred_mode 2)."""
import functools

import numpy as np

import rough_hint_cases as RH
import split2_ref as R

LAMBDAS = (0, 0.002, 0.1, 10)
MOTIONS = ((3, -2), (-2, 1))    # what the two references are moved by, luma samples
FORMATS = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}
INT_MAX = R.INT_MAX


def _grid(size, b):
    return -(-(-(-size // b)) // 4) * 4


def _case(w, h, xb=8, yb=8, prec=2, refs=2, fmt="420", ext=32, lam=0.1, pad=0, picture="mixed", start="near", seed=1, want=()):
    return dict(w=w, h=h, xb=xb, yb=yb, nbx=_grid(w, xb), nby=_grid(h, yb), prec=prec, refs=refs, fmt=fmt, ext=ext, lam=lam, pad=pad,
                picture=picture, start=start, seed=seed, want=tuple(want))


CASES = {
    "tiny": _case(24, 16, prec=1, ext=8, seed=20, want=("same_sb_outside_neighbour",)),
    "precision_0": _case(64, 48, prec=0, seed=21),
    "precision_1": _case(64, 48, prec=1, seed=22, want=("mode1", "mode2", "mode3", "mode0", "dc_leftover")),
    # (at precision 2 and 3 the bi-reference trial measures luma against V's prediction in a corner -- the reference's shared
    # fetch buffers, tests/split2_ref.py -- and rarely wins)
    "precision_2": _case(64, 48, prec=2, seed=23, want=("mode1", "mode2", "mode0", "dc_leftover", "shared_buffer")),
    "precision_3": _case(64, 48, prec=3, seed=24, want=("mode0", "shared_buffer")),
    # chroma rows of two samples
    "block_4x4": _case(52, 44, xb=4, yb=4, prec=3, ext=4, seed=25, want=("outside",)),
    "block_12x12": _case(96, 72, xb=12, yb=12, prec=2, fmt="422", seed=26),
    "block_16x8": _case(96, 72, xb=16, yb=8, prec=3, ext=16, seed=27),
    # two 16-sample segments per row, in all three components; the right and bottom blocks are clipped
    "block_32x32": _case(100, 75, xb=32, yb=32, prec=2, fmt="444", seed=28, want=("clipped", "shared_buffer")),
    "block_32x32_420": _case(104, 80, xb=32, yb=32, prec=3, seed=29, want=("clipped",)),
    # a width and height that are no multiples of the block, the grid padded in x, in y, in both
    "clipped_padded_both": _case(101, 75, prec=2, seed=30, want=("clipped", "outside", "same_sb_outside_neighbour", "other_sb_outside_neighbour")),
    "padded_x": _case(100, 64, prec=1, seed=31, want=("outside", "outside_mode2", "same_sb_outside_neighbour")),
    "padded_y": _case(64, 76, prec=2, seed=32, want=("outside", "outside_mode1", "same_sb_outside_neighbour")),
    "padded_stride": _case(93, 70, prec=3, refs=1, pad=37, seed=33, want=("clipped", "dc_considered_one_ref")),
    "format_444": _case(64, 48, prec=2, fmt="444", seed=34, want=("shared_buffer",)),
    "format_444_precision_1": _case(64, 48, prec=1, fmt="444", seed=34, want=("mode3",)),
    "format_422": _case(64, 48, prec=3, fmt="422", seed=35),
    # one reference: width[] and height[] stay 0, the DC trigger is 0 < best_error
    "one_reference": _case(72, 56, prec=2, refs=1, seed=36, want=("dc_considered_one_ref", "mode0", "mode1", "dc_leftover")),
    "one_reference_precision_0": _case(48, 40, prec=0, refs=1, fmt="444", seed=37, want=("dc_considered_one_ref",)),
    # the extension equal to the block, the border blocks' vectors just past the bi-reference bounds
    "extension_is_block": _case(88, 64, prec=1, ext=8, start="bounds", seed=38, want=("bi_inadmissible", "apron_columns", "rows_above")),
    "extension_is_block_precision_2": _case(80, 64, xb=16, yb=16, prec=2, ext=16, start="bounds", seed=39, want=("bi_inadmissible", "apron_columns")),
    # mv->metric == INT_MAX in sub-pel records of reference 1, of reference 2, of both
    "int_max": _case(64, 48, prec=2, start="int_max", seed=40, want=("int_max",)),
    "int_max_one_reference": _case(48, 32, prec=1, refs=1, start="int_max", seed=41, want=("int_max", "mode0")),
    # every error is 0: the entropy alone decides, ties keep the first trial
    "flat": _case(64, 48, prec=2, picture="flat", start="same", seed=42, want=("ties",)),
    "lambda_0": _case(80, 64, prec=2, lam=0, start="same", seed=43, want=("ties",)),
    "lambda_small": _case(80, 64, prec=3, lam=0.002, seed=43),
    "lambda_10": _case(80, 64, prec=1, lam=10, seed=43, want=("mode3", "mode0")),
}
# different geometry, chroma format and number of references
THREE_UNLIKE = ("block_32x32", "padded_stride", "block_12x12")


def params_of(c):
    hs, vs = FORMATS[c["fmt"]]
    return dict(x_num_blocks=c["nbx"], y_num_blocks=c["nby"], xbsep_luma=c["xb"], ybsep_luma=c["yb"], mv_precision=c["prec"], h_shift=hs, v_shift=vs)


def _sizes(c):
    hs, vs = FORMATS[c["fmt"]]
    return [(c["w"], c["h"]), ((c["w"] + hs) >> hs, (c["h"] + vs) >> vs), ((c["w"] + hs) >> hs, (c["h"] + vs) >> vs)]


def pictures(c):
    """([Y, U, V] of the source, per reference [Y, U, V])."""
    sizes, seed = _sizes(c), c["seed"]
    hs, vs = FORMATS[c["fmt"]]
    if c["picture"] == "flat":
        src = [np.full((h, w), 77, np.uint8) for (w, h) in sizes]
        return src, [[p.copy() for p in src] for _ in range(c["refs"])]
    src = [RH.texture(w, h, seed + k).copy() for k, (w, h) in enumerate(sizes)]
    for k, (w, h) in enumerate(sizes):
        src[k][h // 2:, w // 2:] = (90, 100, 140)[k]
    refs = []
    for r in range(c["refs"]):
        planes = []
        for k, (w, h) in enumerate(sizes):
            mx, my = MOTIONS[r]
            if k:
                mx, my = mx >> hs, my >> vs
            rng = np.random.default_rng(seed + 100 * r + 10 * k + 1000)
            p = RH.moved(src[k], mx, my, 0, noise=0).astype(np.int32)
            amp = np.zeros((h, w), np.int32)
            amp[:h // 2, :w // 2] = (1, 40)[r]
            amp[:h // 2, w // 2:] = (40, 1)[r]
            amp[h // 2:, :w // 2] = 14
            p = p + np.rint((rng.random((h, w)) * 2 - 1) * amp).astype(np.int32)
            p[h // 2:, w // 2:] = RH.texture(w, h, seed + 50 + 7 * r + k)[h // 2:, w // 2:]
            planes.append(np.clip(p, 0, 255).astype(np.uint8))
        refs.append(planes)
    return src, refs


def start_fields(c, src, refs):
    """The sub-pel field of each reference: the true motion plus or minus one unit of the precision, the metric the luma
    SAD there.  Flags, chroma_metric and the other reference's vector are noise; what of it must survive, survives.
    bounds: the border blocks' vectors one unit past the bi-reference trial's bounds -- the left column through reference
    1, the right column through reference 2, the top row through reference 2, the bottom row through reference 1.
    int_max: a metric of INT_MAX in every third record of field 0, every fourth of field 1.  same: both fields hold the
    same vectors in both slots, so the two single-reference trials of a block without neighbours tie."""
    nbx, nby, xb, yb, w, h, p, e = (c[k] for k in ("nbx", "nby", "xb", "yb", "w", "h", "prec", "ext"))
    fields = []
    last_i, last_j = -(-w // xb) - 1, -(-h // yb) - 1
    for r in range(c["refs"]):
        same = c["start"] == "same"
        rng = np.random.default_rng(c["seed"] + 3000 + (0 if same else r))
        f = np.zeros(nbx * nby, R.MV_DTYPE)
        f["flags"] = rng.integers(0, 1 << 32, f.size, dtype=np.uint64).astype(np.uint32)
        f["chroma_metric"] = rng.integers(0, 1 << 16, f.size)
        f["metric"] = rng.integers(0, 1 << 20, f.size)
        v = rng.integers(-9, 10, (f.size, 4)).astype(np.int16)
        spread = 1 if p else 0
        v[:, r] = (MOTIONS[0 if same else r][0] << p) + rng.integers(-spread, spread + 1, f.size)
        v[:, 2 + r] = (MOTIONS[0 if same else r][1] << p) + rng.integers(-spread, spread + 1, f.size)
        up = R.UpFrame(refs[r][0], e)
        for j in range(last_j + 1):
            for i in range(last_i + 1):
                n = j * nbx + i
                bw, bh = min(xb, w - i * xb), min(yb, h - j * yb)
                if c["start"] == "bounds":
                    if i == 0 and r == 0:
                        v[n][r] = -e - 1
                    if i == last_i and r == 1:
                        v[n][r] = (w << p) + e - bw + 1 - ((i * xb) << p)
                    if j == 0 and r == 1:
                        v[n][2 + r] = -e - 1
                    if j == last_j and r == 0:
                        v[n][2 + r] = (h << p) + e - bh + 1 - ((j * yb) << p)
                got = up.block(((i * xb) << p) + int(v[n][r]), ((j * yb) << p) + int(v[n][2 + r]), p, bw, bh)
                f["metric"][n] = int(np.abs(src[0][j * yb:j * yb + bh, i * xb:i * xb + bw].astype(np.int32) - got).sum())
                if c["start"] == "int_max" and n % (3 + r) == 0:
                    f["metric"][n] = INT_MAX
        f["v"] = v
        fields.append(f)
    return fields


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(src planes, reference planes, fields) of a case; read-only."""
    return make_inputs(tuple(sorted(CASES[name].items())))


@functools.lru_cache(maxsize=None)
def make_inputs(items):
    c = dict(items)
    src, refs = pictures(c)
    fields = start_fields(c, src, refs)
    for a in src + [p for r in refs for p in r] + fields:
        a.setflags(write=False)
    return src, refs, fields


def reference(c, src, refs, fields, **kw):
    return R.split2(src, refs, params_of(c), c["lam"], fields, c["ext"], **kw)


def derived(c, st):
    """The stats the wants name that the restatement does not count itself."""
    st = dict(st)
    for m in range(4):
        st["mode%d" % m] = st["modes"][m]
    st["outside"] = sum(st["outside_mode"])
    st["outside_mode1"], st["outside_mode2"] = st["outside_mode"][1], st["outside_mode"][2]
    st["clipped"] = int(c["w"] % c["xb"] != 0 or c["h"] % c["yb"] != 0)
    return st


@functools.lru_cache(maxsize=None)
def expected(name):
    """(motion, superblocks, table, stats) of a case by tests/split2_ref.py, raster order; read-only."""
    c = CASES[name]
    src, refs, fields = inputs(name)
    stats = {}
    motion, sb, table = reference(c, src, refs, fields, stats=stats)
    stats = derived(c, stats)
    for key in c["want"]:
        assert stats[key] > 0, (name, key, stats)
    assert stats["inside_with_outside_neighbour"] == 0, name
    for a in (motion, sb, table):
        a.setflags(write=False)
    return motion, sb, table, stats


# ---- the rounding case: a choice from crafted tables ------------------------------------------------------------------

ROUNDING = dict(w=64, h=48, xb=8, yb=8, nbx=8, nby=8, prec=1, refs=2, fmt="420", ext=32, lam=0.1, pad=0)


@functools.lru_cache(maxsize=None)
def rounding():
    """(fields, table, motion, superblocks, fused motion): lambda 0.1 and, per block, a bi-reference error that puts its
    score ON the better single reference's in exact arithmetic (ten of error per bit of entropy), so that the two roundings
    of `entropy + error * lambda` decide.  The entropies are taken with every neighbour predicting from both references
    (near enough).  DC is kept out of it: the area entry is huge.  Searched: the first seed whose unfused and fused
    results differ."""
    c = ROUNDING
    P = params_of(c)
    nbx = c["nbx"]
    for seed in range(64):
        rng = np.random.default_rng(7000 + seed)
        fields = [RH.random_field(nbx, c["nby"], 0, 7100 + 2 * seed + r, reach=6).copy() for r in (0, 1)]
        for f in fields:
            f["metric"] = rng.integers(1500, 4000, f.size)
        table = np.zeros((fields[0].size, R.T_INTS), np.int32)
        table[:, R.T_CHROMA] = rng.integers(200, 900, fields[0].size)
        table[:, R.T_CHROMA + 1] = rng.integers(200, 900, fields[0].size)
        table[:, R.T_BI_OK] = 1
        table[:, R.T_AREA] = 1 << 20
        table[:, R.T_DC_ERROR] = R.T_NONE
        both = [bytearray(R.BEST_MV) for _ in range(fields[0].size)]
        for n, rec in enumerate(both):
            rec[0] = 0x13
            for k in range(4):
                R.set_vec(rec, k, int(fields[k & 1]["v"][n][k]))
        for n in range(fields[0].size):
            i, j = n % nbx, n // nbx
            entropy = [R.block_entropy(lambda x, y: both[y * nbx + x], i, j, bytearray([r + 1]) + bytes(both[n][1:])) for r in (0, 1)]
            error = [int(table[n][R.T_CHROMA + r]) + int(fields[r]["metric"][n]) for r in (0, 1)]
            best = min((0, 1), key=lambda r: entropy[r] + 0.1 * error[r])
            total = max(error[best] - 10 * entropy[1 - best], 2)
            table[n][R.T_BI_LUMA], table[n][R.T_BI_CHROMA] = total - total // 3, total // 3
        plain, sb = R.choose(table, P, c["w"], c["h"], c["lam"], fields)
        fused, _ = R.choose(table, P, c["w"], c["h"], c["lam"], fields, fused=True)
        if plain.tobytes() != fused.tobytes():
            for a in fields + [table, plain, sb, fused]:
                a.setflags(write=False)
            return fields, table, plain, sb, fused
    raise AssertionError("no seed separates the unfused from the fused score")


# ---- seeded draws -------------------------------------------------------------------------------------------------------

N_DRAWS = 12
SEPARATIONS = (4, 8, 12, 16, 20, 24, 28, 32)


def draw_case(n):
    """Geometry n: sizes 17 .. 104, every separation 4 .. 32 in steps of 4, every chroma format, precision and lambda, an
    extension between the block and 32."""
    rng = np.random.default_rng(9000 + n)
    xb, yb = SEPARATIONS[n % 8], SEPARATIONS[(3 * n + n // 8) % 8]
    w, h = int(rng.integers(17, 105)), int(rng.integers(17, 81))
    return _case(w, h, xb=xb, yb=yb, prec=n % 4, refs=1 + (n % 3 != 0), fmt=("420", "422", "444")[n % 3], ext=int(rng.integers(max(xb, yb, 4), 33)),
                 lam=LAMBDAS[n % len(LAMBDAS)], pad=int(rng.integers(0, 3)) * 13, seed=9100 + n)


@functools.lru_cache(maxsize=None)
def draw(n):
    """(case, src, refs, fields, motion, superblocks, table) of draw n."""
    c = draw_case(n)
    src, refs, fields = make_inputs(tuple(sorted(c.items())))
    motion, sb, table = reference(c, src, refs, fields)
    return c, src, refs, fields, motion, sb, table


# ---- refusals -------------------------------------------------------------------------------------------------------------

# What is spoilt in the second of two pictures, one member at a time: (member, value, what the message says).
REFUSED_CASE = "precision_1"
REFUSED_MEMBERS = (
    ("prec", 4, "mv_precision"), ("prec", -1, "mv_precision"), ("xb", 36, "block of"), ("yb", 0, "block of"), ("nbx", 0, "blocks"),
    ("nbx", 6, "whole superblocks"), ("nby", 9, "whole superblocks"), ("xb", 7, "chroma subsampling"), ("ext", 7, "extension"), ("ext", 33, "extension"),
    ("lam", -1.0, "lambda"), ("lam", float("nan"), "lambda"), ("lam", float("inf"), "lambda"), ("stride", -1, "stride"),
    ("refs", 0, "references"), ("refs", 3, "references"), ("shifts", (0, 1), "chroma shifts"), ("shifts", (2, 1), "chroma shifts"),
    ("shifts", (1, -1), "chroma shifts"), ("no_component", 1, "component U"), ("no_component", 2, "component V"), ("no_image", (1, 0), "upsampled Y image"),
    ("no_image", (0, 2), "upsampled V image"), ("no_field", 1, "field of reference 1"), ("no_motion", 0, "NULL"), ("no_superblocks", 0, "NULL"),
)
