"""30 seeded random draws for tests/test_gpu_rough_hint.py: 1 .. 3 unlike pictures per draw -- plane size, block size,
block counts (just covering the level's plane, short of it, or padded beyond it), shift, extension, reference index and a
field of the level above whose vectors are random, not plausible.  tests/test_rough_hint_draws.py walks them on the CPU
and asserts what they cover."""
import functools

import numpy as np

import rough_hint_cases as K
import rough_hint_ref as R

N_DRAWS = 30
BLOCKS = [(8, 8), (8, 8), (4, 4), (12, 12), (16, 16), (16, 8), (8, 16), (5, 7), (32, 32)]


@functools.lru_cache(maxsize=None)
def draw(n):
    """[picture] of draw n: dicts with the members of a case plus frame, ref, hint."""
    rng = np.random.default_rng(9000 + n)
    pics = []
    for k in range(int(rng.integers(1, 4))):
        xb, yb = BLOCKS[int(rng.integers(0, len(BLOCKS)))]
        if n % 10 == 3 and k == 0:
            xb, yb = 4, 4       # (small blocks on a large plane: diagonals longer than the workgroup has waves)
        shift = int(rng.integers(1, 4))
        w, h = (int(v) for v in rng.integers(72 if (xb, yb) == (4, 4) and k == 0 and n % 10 == 3 else 9, 101, 2))
        # the level's grid: from two blocks short of the plane to three beyond it
        gx = max(1, -(-w // xb) + int(rng.integers(-2, 4)))
        gy = max(1, -(-h // yb) + int(rng.integers(-2, 4)))
        nbx = max(1, (gx << shift) - int(rng.integers(0, 1 << shift)))
        nby = max(1, (gy << shift) - int(rng.integers(0, 1 << shift)))
        c = K._case(w, h, nbx, nby, shift, xb=xb, yb=yb, ref_index=int(rng.integers(0, 2)), ext=int(rng.choice([0, 0, 8, 32])),
                    dist=int(rng.choice([4, 4, 4, 2, 7])), pad=int(rng.choice([0, 0, 3, 64])), seed=9000 + 10 * n + k)
        frame = K.texture(w, h, c["seed"])
        c["frame"] = frame
        c["ref"] = K.moved(frame, int(rng.integers(-6, 7)), int(rng.integers(-6, 7)), c["seed"] + 1)
        c["hint"] = K.random_field(nbx, nby, shift, c["seed"] + 2, reach=int(rng.choice([4, 16, 60])), wild=float(rng.choice([0, 0.05, 0.3])))
        pics.append(c)
    return pics


@functools.lru_cache(maxsize=None)
def expected(n):
    """[(field, stats)] of draw n's pictures by tests/rough_hint_ref.py."""
    out = []
    for c in draw(n):
        stats = {}
        field = R.rough_scan_hint(c["frame"], c["ref"], K.params_of(c), c["shift"], c["dist"], c["ref_index"], c["hint"], c["ext"], stats=stats)
        stats["turns"] = int(K.max_diagonal(c["nbx"], c["nby"], c["shift"]) > K.ROUGH_WAVES)
        out.append((field, stats))
    return out
