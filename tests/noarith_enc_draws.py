"""Seeded random geometries of the noarith transform-data encoder, shared by the CPU walk and the GPU test.

The draws keep |q| <= 2047 and rows of at most 32 samples, so that no 16-bit row sum reaches 65536: the reference's zero
test is then the true one, false_zero is 0 on every draw and the round trip through the restated decoder gives back every
value.  tests/test_noarith_enc_ref.py asserts both on all draws.
"""
import numpy as np

import noarith_enc_cases as NC

SEED = 20260117
NDRAWS = 24
MAX_ABS = 2047
MAX_ROW = 32


def _fill(case, rng, densities=(0.0, 0.1, 0.5, 0.9)):
    density = rng.choice(densities)
    for p in case.planes:
        v = rng.integers(-MAX_ABS, MAX_ABS + 1, p.shape)
        p[...] = np.where(rng.random(p.shape) < density, v, 0)
    # some whole sub-bands and codeblocks are zero
    for k in range(3):
        for i in range(case.nsub):
            if rng.random() < 0.2:
                case.band(k, i)[...] = 0


def draws():
    rng = np.random.default_rng(SEED)
    out = []
    for n in range(NDRAWS):
        depth = (n >> 2) % 4       # every (sample size, codeblock mode, depth) occurs
        fmt = int(rng.choice([420, 422, 444]))
        lw = int(rng.integers(1, MAX_ROW + 1)) >> depth << depth or 1 << depth
        lh = int(rng.integers(1, 25))
        counts = [(int(rng.integers(1, 5)), int(rng.integers(1, 4))) for _ in range(depth + 1)]
        dtype = np.int16 if n % 2 == 0 else np.int32
        out.append(NC.Case("draw-%d" % n, dtype, lw, lh, fmt, depth, counts, (n >> 1) & 1, _fill,
                           seed=int(rng.integers(1 << 30)), qbase=int(rng.integers(0, 61))))
        assert max(w for w, h in out[-1].sizes) <= MAX_ROW
    return out


DEEP_SEED = 20261020
DEEP_DEPTHS = (4, 5, 6)


def deep_draws():
    """Depths 4, 5 and 6 for both sample sizes and both codeblock modes, from a generator of their own (DRAWS stay what
    they were).  The transform's width is a multiple of 1 << depth, so the limit on rows is held where it matters: the
    widest sub-band row -- half the plane -- has at most MAX_ROW samples.  At depth 6 the LL band of a 64 x 64 component is
    one sample and most levels have more codeblocks than samples."""
    rng = np.random.default_rng(DEEP_SEED)
    out = []
    for depth in DEEP_DEPTHS:
        for dtype in (np.int16, np.int32):
            for mode in (0, 1):
                fmt = int(rng.choice([420, 422, 444]))
                lw = int(rng.integers(1, 2 * MAX_ROW + 1))
                lh = int(rng.integers(1, 2 * MAX_ROW + 1))
                counts = [(int(rng.integers(1, 5)), int(rng.integers(1, 4))) for _ in range(depth + 1)]
                name = "deep-d%d-%s-m%d" % (depth, "s16" if dtype == np.int16 else "s32", mode)
                out.append(NC.Case(name, dtype, lw, lh, fmt, depth, counts, mode, lambda c, r: _fill(c, r, (0.1, 0.5, 0.9)),
                                   seed=int(rng.integers(1 << 30)), qbase=int(rng.integers(0, 61))))
                assert max(w for w, h in out[-1].sizes) // 2 <= MAX_ROW
    return out


DRAWS = draws()
DEEP_DRAWS = deep_draws()
