"""The named single-level cases and the seeded draws of tests/test_gpu_hier_bm.py: inputs, and the expected field from
tests/hier_bm_ref.py (computed once per case and process).  Every plane is about 100 x 75 or less: the planes are those
of the level itself, the block grid is the full picture's (level blocks << shift).  The assertions at the bottom of
`expected` say what a case is there for; they run on the CPU (tests/test_hier_bm_ref.py walks them)."""
import functools

import numpy as np

import analysis_ref as A
import hier_bm_ref as R
import oracle_lib as O
from rough_hint_cases import moved, random_field, texture

ROUGH_WAVES = 16                # SCHRO_HIP_ROUGH_WAVES
FORMATS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}


def _level_blocks(size, b, multiple=1):
    n = -(-size // b)
    return -(-n // multiple) * multiple


def _case(w, h, shift, xb=8, yb=8, fmt="420", ref_index=0, ext=32, h_range=5, pad=0, picture="texture", hint="random", seed=1,
          grid_multiple=1, motion=(3, -2), want=()):
    """A level plane of w x h with the block grid of the full picture: as many level blocks as cover the plane, rounded up
    to `grid_multiple` of them (the encoder rounds x_num_blocks up to whole superblocks), << shift."""
    return dict(w=w, h=h, shift=shift, xb=xb, yb=yb, fmt=fmt, ref_index=ref_index, ext=ext, h_range=h_range, pad=pad, picture=picture,
                hint=hint, seed=seed, nbx=_level_blocks(w, xb, grid_multiple) << shift, nby=_level_blocks(h, yb, grid_multiple) << shift,
                motion=motion, want=tuple(want))


CASES = {
    # x_num_blocks, y_num_blocks rounded up to multiples of 4: blocks off the plane are skipped, partial right and bottom blocks
    "padded_grid_shift0": _case(101, 75, 0, grid_multiple=4, h_range=3, seed=11, want=("skipped", "dropped")),
    "padded_grid_shift1": _case(101, 75, 1, grid_multiple=4, h_range=3, seed=12, want=("skipped", "dropped")),
    "padded_grid_shift2": _case(101, 75, 2, grid_multiple=4, h_range=5, seed=13, want=("skipped",)),
    "padded_grid_shift3": _case(101, 75, 3, grid_multiple=4, h_range=10, seed=14, want=("skipped",)),
    # 19 block rows and 26 columns: diagonals of up to 19 blocks for 16 waves
    "tall_4x4": _case(101, 75, 0, xb=4, yb=4, h_range=3, seed=15, want=("turns",)),
    "sep_12x12": _case(101, 75, 1, xb=12, yb=12, seed=16),
    "sep_16x8": _case(101, 75, 1, xb=16, yb=8, seed=17),
    "sep_16x16_shift0": _case(101, 75, 0, xb=16, yb=16, h_range=3, seed=18),
    # odd luma sizes: rounded-up chroma planes in every format
    "chroma_422": _case(101, 75, 1, fmt="422", seed=19),
    "chroma_444": _case(101, 75, 1, fmt="444", seed=20),
    "chroma_422_shift0": _case(61, 45, 0, fmt="422", h_range=3, seed=21),
    "ref_1": _case(101, 75, 1, ref_index=1, seed=22),
    "ref_1_shift0": _case(61, 45, 0, ref_index=1, h_range=3, pad=37, seed=23),
    # constant planes, parents [0, A, 0, B, ..] per star: every metric is 0, the order of LAST occurrence decides
    "flat_ties": _case(64, 48, 1, picture="flat", hint="star", seed=24, want=("order_ties", "dropped")),
    # frame == reference and a hint field of zeros: every candidate is a duplicate of the zero vector
    "still": _case(64, 48, 1, picture="still", hint="zero", seed=25, want=("all_duplicates",)),
    # a 64 x 48 picture moved by (-19, 14), its level 2 (16 x 12), hints of that size and far beyond: the clamps fire,
    # negative vectors go through >>, the window of 41 is larger than the plane
    "moved_far": _case(16, 12, 2, h_range=20, picture="pyramid", hint="far", motion=(-19, 14), seed=26, want=("clamped",)),
    # the top level of a chain: neighbours only
    "nohint_top": _case(51, 38, 2, h_range=20, hint=None, seed=27, want=("dropped",)),
    "nohint_shift0": _case(40, 30, 0, h_range=3, hint=None, seed=28),
    "range_1": _case(64, 48, 1, h_range=1, seed=29),
    "extension_is_the_block": _case(64, 48, 1, xb=16, yb=16, ext=16, h_range=20, hint="far", seed=30, want=("clamped",)),
}

THREE_UNLIKE = ("padded_grid_shift2", "chroma_444", "ref_1_shift0")


def params_of(c):
    return dict(x_num_blocks=c["nbx"], y_num_blocks=c["nby"], xbsep_luma=c["xb"], ybsep_luma=c["yb"])


def chroma_size(w, h, fmt):
    hs, vs = FORMATS[fmt]
    return R.round_up_shift(w, hs), R.round_up_shift(h, vs)


def star_field(nbx, nby, shift):
    """Parents of a star in the order the list takes them -- centre, left, right, above, below -- hold 0, A, 0, B, A:
    by column parity and row parity of the parent grid."""
    f = R.field_set(nbx * nby, 0, 1)
    step = 2 << shift
    a, b = 4 << shift, -(6 << shift)
    for kk in range(0, nby, step):
        for ll in range(0, nbx, step):
            px, py = (ll // step) & 1, (kk // step) & 1
            v = (0, 0) if (px, py) == (0, 0) else ((a, a) if py == 0 else (b, a))
            f[kk * nbx + ll]["v"] = (v[0], v[0], v[1], v[1])
    return f


def pictures(w, h, fmt, kind, seed, motion):
    """((Y, U, V) of the frame, (Y, U, V) of the reference)."""
    cw, chh = chroma_size(w, h, fmt)
    sizes = ((w, h), (cw, chh), (cw, chh))
    if kind == "flat":
        frame = tuple(np.full((hh, ww), 77 + 20 * k, np.uint8) for k, (ww, hh) in enumerate(sizes))
        return frame, tuple(p.copy() for p in frame)
    frame = tuple(texture(ww, hh, seed + 10 * k) for k, (ww, hh) in enumerate(sizes))
    if kind == "still":
        return frame, tuple(p.copy() for p in frame)
    hs, vs = FORMATS[fmt]
    ref = tuple(moved(p, motion[0] >> (hs if k else 0), motion[1] >> (vs if k else 0), seed + 1000 + k) for k, p in enumerate(frame))
    return frame, ref


def make_inputs(c):
    w, h, seed, shift = c["w"], c["h"], c["seed"], c["shift"]
    if c["picture"] == "pyramid":
        # the level planes of a full picture and of its moved copy
        full = pictures(w << shift, h << shift, c["fmt"], "texture", seed, c["motion"])
        frame, ref = (R.pyramid3(p, shift)[shift] for p in full)
        assert frame[0].shape == (h, w)
    else:
        frame, ref = pictures(w, h, c["fmt"], c["picture"], seed, c["motion"])
    nbx, nby = c["nbx"], c["nby"]
    if c["hint"] is None:
        hint = None
    elif c["hint"] == "zero":
        hint = random_field(nbx, nby, shift, seed + 2000, reach=0)
    elif c["hint"] == "star":
        hint = star_field(nbx, nby, shift)
    elif c["hint"] == "far":
        hint = random_field(nbx, nby, shift, seed + 2000, reach=3, wild=0.4)
        hint["v"] += np.array([c["motion"][0], c["motion"][0], c["motion"][1], c["motion"][1]], np.int16) << shift
        hint["v"] += 1          # (odd negative values: >> rounds down)
    else:
        hint = random_field(nbx, nby, shift, seed + 2000, reach=6)
    for a in frame + ref + ((hint,) if hint is not None else ()):
        a.setflags(write=False)
    return frame, ref, hint


@functools.lru_cache(maxsize=None)
def inputs(name):
    """((Y, U, V) frame, (Y, U, V) ref, hint field or None) of a case; read-only."""
    return make_inputs(CASES[name])


def max_diagonal(nbx, nby, shift):
    skip = 1 << shift
    return min(-(-nbx // skip), -(-nby // skip))


def reference(c, frame, ref, hint, order="raster"):
    stats = {}
    hs, vs = FORMATS[c["fmt"]]
    field = R.hbm_scan_hint(frame, ref, params_of(c), c["shift"], c["h_range"], c["ref_index"], hint, hs, vs, c["ext"], order=order, stats=stats)
    stats["turns"] = int(max_diagonal(c["nbx"], c["nby"], c["shift"]) > ROUGH_WAVES)
    return field, stats


@functools.lru_cache(maxsize=None)
def expected(name):
    """(field, stats) of a case by tests/hier_bm_ref.py; the field is read-only."""
    c = CASES[name]
    field, stats = reference(c, *inputs(name))
    for key in c["want"]:
        assert stats[key] > 0, (name, key, stats)
    if c["ref_index"] == 1:
        assert not field["v"][:, 0].any() and not field["v"][:, 2].any(), name      # dx[0], dy[0] stay 0
        assert ((field["flags"] & 3) == 2).all()
    field.setflags(write=False)
    return field, stats


# ---- seeded draws: geometry, format, level, reference and hint at random -------------------------------------------------

N_DRAWS = 4


def draw_case(n):
    rng = np.random.default_rng(9100 + n)
    xb, yb = (int(rng.choice([4, 8, 12, 16])) for _ in range(2))
    shift = int(rng.integers(0, 4))
    return _case(int(rng.integers(20, 91)), int(rng.integers(16, 71)), shift, xb=xb, yb=yb, fmt=str(rng.choice(sorted(FORMATS))),
                 ref_index=int(rng.integers(0, 2)), ext=int(rng.choice([16, 32, 40])), h_range=int(rng.choice([1, 3, 5, 10, 20])),
                 pad=int(rng.integers(0, 40)), hint=[None, "random", "far"][int(rng.integers(0, 3))], seed=9200 + n,
                 grid_multiple=int(rng.choice([1, 4])), motion=(int(rng.integers(-6, 7)), int(rng.integers(-6, 7))))


@functools.lru_cache(maxsize=None)
def draw(n):
    """(case, frame, ref, hint, expected field) of draw n."""
    c = draw_case(n)
    frame, ref, hint = make_inputs(c)
    field, _ = reference(c, frame, ref, hint)
    field.setflags(write=False)
    return c, frame, ref, hint, field


# ---- the chain ------------------------------------------------------------------------------------------------------------

CHAIN_SIZES = [(128, 96), (101, 75)]
CHAIN_EXT = 32


def chain_params(w, h, xb=8, yb=8):
    """The blocks of the full picture (level 0), whole superblocks as the encoder lays them out."""
    return dict(x_num_blocks=4 * -(-w // (4 * xb)), y_num_blocks=4 * -(-h // (4 * yb)), xbsep_luma=xb, ybsep_luma=yb)


@functools.lru_cache(maxsize=None)
def chain_pictures(w, h):
    frame, ref = pictures(w, h, "420", "texture", 7000 + w, (5, -3))
    for a in frame + ref:
        a.setflags(write=False)
    return frame, ref


@functools.lru_cache(maxsize=None)
def chain_reference(w, h, n_levels, ref_index):
    """The fields 0 .. n_levels of tests/hier_bm_ref.hbm_scan on the numpy pyramid (level 0 included: levels 1 .. n_levels
    are the same with and without it), and the stats."""
    frame, ref = chain_pictures(w, h)
    stats = {}
    fields = R.hbm_scan(R.pyramid3(frame, n_levels), R.pyramid3(ref, n_levels), chain_params(w, h), n_levels, ref_index, 1, 1, CHAIN_EXT,
                        with_level0=True, stats=stats)
    for f in fields:
        f.setflags(write=False)
    return fields, stats


# What tests/test_gpu_hier_bm.py::test_a_refused_call_writes_nothing spoils in the second of two entries, one at a time
REFUSED_CASE = "range_1"
REFUSED_MEMBERS = (("h_range", 0), ("h_range", 21), ("shift", -1), ("shift", 9), ("ref_index", 2), ("nbx", 0), ("yb", 65), ("ext", 7),
                   ("h_shift", 2), ("stride", -1))
