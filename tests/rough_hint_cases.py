"""The named single-level cases of tests/test_gpu_rough_hint.py: inputs, and the expected field from tests/rough_hint_ref.py
(computed once per case and process).  Every plane is about 100 x 80 or less but the one whose diagonals must be longer
than the workgroup has waves.  The assertions at the bottom of `expected` say what a case is there for; they run on the
CPU (tests/test_rough_hint_draws.py walks them)."""
import functools

import numpy as np

import analysis_ref as A
import oracle_lib as O
import rough_hint_ref as R

ROUGH_WAVES = 16                # SCHRO_HIP_ROUGH_WAVES


def texture(w, h, seed):
    """A picture with structure at the scale of a block: box-filtered noise."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (h + 8, w + 8)).astype(np.float64)
    k = np.ones(5) / 5
    p = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, p)
    p = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, p)
    p = (p - p.min()) / max(p.max() - p.min(), 1) * 255
    return p[4:4 + h, 4:4 + w].astype(np.uint8)


def moved(frame, dx, dy, seed, noise=3):
    """The reference picture of `frame`: its content moved by (dx, dy), edge samples repeated, plus a little noise."""
    h, w = frame.shape
    ys, xs = np.clip(np.arange(h) - dy, 0, h - 1), np.clip(np.arange(w) - dx, 0, w - 1)
    n = np.random.default_rng(seed).integers(-noise, noise + 1, (h, w)) if noise else 0
    return np.clip(frame[np.ix_(ys, xs)].astype(np.int32) + n, 0, 255).astype(np.uint8)


def random_field(nbx, nby, shift, seed, reach=24, wild=0.0):
    """A field of level shift + 1 with random records: vectors of up to `reach` level samples in BOTH references, a share
    `wild` of them far outside any picture; metrics and flags are noise the hint level must not read."""
    rng = np.random.default_rng(seed)
    f = np.zeros(nbx * nby, O.MV_DTYPE)
    f["flags"] = rng.integers(0, 4, f.size)
    f["metric"] = rng.integers(0, 1 << 20, f.size)
    v = rng.integers(-reach, reach + 1, (f.size, 4)) << shift
    far = rng.random((f.size, 4)) < wild
    v = np.where(far, rng.choice([-30000, -900, 900, 30000], (f.size, 4)), v)
    f["v"] = v.astype(np.int16)
    return f


def constant_field(nbx, nby, dx, dy):
    f = np.zeros(nbx * nby, O.MV_DTYPE)
    f["flags"] = 1
    f["v"] = np.array([dx, dx, dy, dy], np.int16)
    return f


def _case(w, h, nbx, nby, shift, xb=8, yb=8, ref_index=0, ext=0, dist=4, pad=0, picture="texture", hint="random", seed=1, want=()):
    return dict(w=w, h=h, nbx=nbx, nby=nby, shift=shift, xb=xb, yb=yb, ref_index=ref_index, ext=ext, dist=dist, pad=pad,
                picture=picture, hint=hint, seed=seed, want=tuple(want))


def _grid(size, b, shift):
    """Block count of the full picture for a level plane of `size` samples: the level's blocks just cover the plane."""
    return -(-size // b) << shift


CASES = {
    # level sizes that are no multiples of the block: partial right and bottom blocks
    "partial_blocks": _case(100, 76, _grid(100, 8, 1), _grid(76, 8, 1), 1, seed=11),
    # x_num_blocks * xbsep well beyond the picture: blocks of size <= 0 -- SAD 0 and invalid windows
    "beyond_the_picture": _case(52, 44, 24, 16, 1, seed=12, want=("empty_block_scan", "invalid_window", "gravity_outside", "skip_empty")),
    # block counts that are no multiples of skip or 2 * skip: parents out of range at the right and at the bottom
    "odd_counts_shift2": _case(48, 40, 23, 17, 2, seed=13),
    "odd_counts_shift1": _case(60, 52, 15, 13, 1, seed=14),
    "one_block": _case(8, 8, 1, 1, 1, seed=15),
    "one_row": _case(96, 8, 24, 1, 1, seed=16),
    "one_column": _case(8, 80, 2, 20, 1, seed=17),
    # 20 x 20 blocks of the level: diagonals of up to 20 blocks for 16 waves
    "long_diagonal": _case(160, 160, 40, 40, 1, seed=18, want=("turns",)),
    # hint vectors that point off the top and left, and off the bottom and right
    "hints_off_top_left": _case(64, 48, 16, 12, 1, hint=(-300, -300), seed=19, want=("skip_negative",)),
    "hints_off_bottom_right": _case(64, 48, 16, 12, 1, hint=(300, 300), seed=20, want=("skip_beyond",)),
    "hints_wild": _case(72, 56, 18, 14, 1, hint="wild", seed=21, want=("skip_negative", "skip_beyond")),
    "extension_32": _case(100, 76, _grid(100, 8, 1), _grid(76, 8, 1), 1, ext=32, seed=22),
    "extension_32_beyond": _case(52, 44, 24, 16, 1, ext=32, seed=23, want=("empty_block_scan", "invalid_window")),
    "shift3": _case(40, 32, 40, 32, 3, seed=24),
    "shift3_odd": _case(45, 35, 43, 37, 3, ext=32, seed=25),
    "block_12x12": _case(100, 80, _grid(100, 12, 1), _grid(80, 12, 1), 1, xb=12, yb=12, seed=26),
    "block_16x16": _case(100, 80, _grid(100, 16, 1), _grid(80, 16, 1), 1, xb=16, yb=16, seed=27),
    "block_16x8": _case(100, 80, _grid(100, 16, 1), _grid(80, 8, 1), 1, xb=16, yb=8, seed=28),
    "block_4x4": _case(50, 42, _grid(50, 4, 1), _grid(42, 4, 1), 1, xb=4, yb=4, seed=29),
    # 9568 bytes of LDS per wave at distance 4, 15328 at distance 20: 6 and 4 waves in the workgroup's 64 KB, not 16
    "block_64x64": _case(100, 80, 4, 4, 1, xb=64, yb=64, seed=30),
    "block_64x64_distance_20": _case(100, 80, 4, 4, 1, xb=64, yb=64, dist=20, ext=32, seed=31),
    "ref_1": _case(100, 76, _grid(100, 8, 1), _grid(76, 8, 1), 1, ref_index=1, seed=32),
    "ref_1_shift2": _case(48, 40, 23, 17, 2, ref_index=1, ext=32, seed=33),
    # tie order: the first candidate wins, the gravity position is kept
    "flat": _case(64, 48, 16, 12, 1, picture="flat", seed=34),
    "checkerboard": _case(64, 48, 16, 12, 1, picture="checkerboard", seed=35),
    "checkerboard_ext": _case(61, 47, 16, 12, 1, picture="checkerboard", ext=32, seed=36),
    "padded_strides": _case(100, 76, _grid(100, 8, 1), _grid(76, 8, 1), 1, pad=37, seed=37),
    "distance_1": _case(64, 48, 16, 12, 1, dist=1, seed=38),
}


# What tests/test_gpu_rough_hint.py::test_a_refused_call_writes_nothing spoils in the second of two "one_row" pictures, one
# at a time: (member of the case, value) -- "stride": the frame's stride relative to a row -- and the two aliasings: the
# picture's hint field is its own output field; its output field is the first picture's.  tests/encoder_walk_cases.py
# sends the same calls through the host code under the sanitizers.
REFUSED_CASE = "one_row"
REFUSED_MEMBERS = (("dist", 0), ("dist", -4), ("dist", 21), ("shift", 0), ("shift", 8), ("ref_index", 2), ("ref_index", -1),
                   ("nbx", 0), ("nby", 0), ("xb", 65), ("yb", 0), ("stride", -1))
REFUSED_ALIASES = ("hint_is_own_field", "field_is_first_field")


def params_of(c):
    return dict(x_num_blocks=c["nbx"], y_num_blocks=c["nby"], xbsep_luma=c["xb"], ybsep_luma=c["yb"])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(frame, ref, hint field) of a case; read-only."""
    c = CASES[name]
    w, h, seed = c["w"], c["h"], c["seed"]
    if c["picture"] == "flat":
        frame, ref = np.full((h, w), 77, np.uint8), np.full((h, w), 77, np.uint8)
    elif c["picture"] == "checkerboard":
        frame, ref = A.checkerboard(w, h), A.checkerboard(w, h)
    else:
        frame = texture(w, h, seed)
        ref = moved(frame, 3, -2, seed + 1000)
    if isinstance(c["hint"], tuple):
        hint = constant_field(c["nbx"], c["nby"], *c["hint"])
    else:
        hint = random_field(c["nbx"], c["nby"], c["shift"], seed + 2000, wild=0.3 if c["hint"] == "wild" else 0.0)
    for a in (frame, ref, hint):
        a.setflags(write=False)
    return frame, ref, hint


def max_diagonal(nbx, nby, shift):
    skip = 1 << shift
    return min(-(-nbx // skip), -(-nby // skip))


@functools.lru_cache(maxsize=None)
def expected(name):
    """(field, stats) of a case by tests/rough_hint_ref.py; the field is read-only."""
    c = CASES[name]
    frame, ref, hint = inputs(name)
    stats = {}
    field = R.rough_scan_hint(frame, ref, params_of(c), c["shift"], c["dist"], c["ref_index"], hint, c["ext"], stats=stats)
    stats["turns"] = int(max_diagonal(c["nbx"], c["nby"], c["shift"]) > ROUGH_WAVES)
    for key in c["want"]:
        assert stats[key] > 0, (name, key, stats)
    if c["ref_index"] == 1:
        assert not field["v"][:, 0].any() and not field["v"][:, 2].any(), name      # dx[0], dy[0] stay 0
    field.setflags(write=False)
    return field, stats
