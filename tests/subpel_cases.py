"""The named cases of tests/test_gpu_subpel.py: inputs, and the expected field and error tables from tests/subpel_ref.py
(computed once per case and process).  Every plane is about 100 x 75 or less.  The `want` tuple of a case says what it is
there for; `expected` asserts it on the CPU (tests/test_subpel_ref.py walks the cases), so a case that stops exercising
its point fails there."""
import functools

import numpy as np

import rough_hint_cases as RH
import subpel_ref as R

LAMBDAS = (0, 0.002, 0.1, 1, 10)
MOTION = (3, -2)                # what `moved` moves the reference by


def _grid(size, b, multiple=1):
    n = -(-size // b)
    return -(-n // multiple) * multiple


def _case(w, h, xb=8, yb=8, prec=2, ref_index=0, ext=32, lam=0.1, pad=0, picture="texture", start="near", seed=1, superblocks=False,
          want=()):
    m = 4 if superblocks else 1
    return dict(w=w, h=h, xb=xb, yb=yb, nbx=_grid(w, xb, m), nby=_grid(h, yb, m), prec=prec, ref_index=ref_index, ext=ext, lam=lam, pad=pad,
                picture=picture, start=start, seed=seed, want=tuple(want))


CASES = {
    "precision_0": _case(64, 48, prec=0, seed=40),
    "precision_1": _case(96, 72, prec=1, seed=41),
    "precision_2": _case(96, 72, prec=2, seed=42, want=("positions2",)),
    "precision_3": _case(96, 72, prec=3, seed=43, want=("positions3",)),
    "block_4x4": _case(52, 44, xb=4, yb=4, prec=3, ext=4, seed=44, want=("positions3",)),
    "block_12x12": _case(96, 72, xb=12, yb=12, prec=2, seed=45),
    "block_16x8": _case(96, 72, xb=16, yb=8, prec=3, ext=16, seed=46),
    "block_16x16": _case(96, 80, xb=16, yb=16, prec=2, ext=16, seed=47),
    "block_32x32": _case(100, 75, xb=32, yb=32, prec=3, ext=32, seed=48, want=("clipped",)),
    "block_20x28": _case(100, 75, xb=20, yb=28, prec=2, ext=28, seed=49, want=("clipped",)),
    # the extension equal to the block: the smallest the calls take
    "extension_is_block": _case(88, 64, xb=8, yb=8, prec=3, ext=8, start="bounds", seed=50, want=("inadmissible", "apron_columns", "rows_beyond")),
    # the right and bottom blocks are partial
    "partial_blocks": _case(101, 75, prec=2, seed=51, want=("clipped",)),
    "partial_blocks_12": _case(101, 75, xb=12, yb=12, prec=3, seed=52, want=("clipped",)),
    # a grid rounded up to whole superblocks: blocks off the picture are skipped, their records not even shifted
    "padded_grid": _case(100, 76, prec=2, superblocks=True, seed=53, want=("skipped", "unshifted")),
    "ref_1": _case(96, 72, prec=2, ref_index=1, seed=54),
    "padded_stride": _case(93, 70, prec=3, ref_index=1, pad=37, seed=55, want=("clipped",)),
    # start vectors on the admissibility bounds in all four directions
    "bounds": _case(96, 72, prec=1, start="bounds", seed=56, want=("inadmissible", "apron_columns", "rows_beyond", "rows_above")),
    "bounds_precision_3": _case(90, 66, xb=12, yb=8, prec=3, ext=12, start="bounds", seed=57, want=("inadmissible", "apron_columns", "rows_beyond")),
    "bounds_32": _case(100, 75, xb=32, yb=32, prec=2, start="bounds", seed=58, want=("inadmissible", "apron_columns", "rows_beyond")),
    # every error is 0: the entropy alone decides, ties keep the centre
    "flat": _case(64, 48, prec=2, picture="flat", start="random", seed=59, want=("ties",)),
    # lambda 0: the entropy alone decides.  A doubled vector is even and so is every prediction (a copy or a median of
    # doubled vectors; two neighbours never occur), and estimate_sint is constant over 1 .. 2, 3 .. 6, 7 .. 14: no odd
    # difference costs less than the even one beside it, nothing ever moves -- on the device as little as here.  At lambda
    # 10 on the same pictures the error outweighs every entropy.  Between the two, at lambda 1 and at a small lambda, is
    # where the chain decides: the result differs from the one predicted from the neighbours as the pass found them.
    "lambda_0": _case(80, 64, prec=2, lam=0, start="random", seed=60, want=("none_only", "ties")),
    "lambda_10": _case(80, 64, prec=2, lam=10, start="random", seed=60),
    "lambda_1": _case(80, 64, prec=2, lam=1, start="random", seed=60, want=("chain",)),
    "lambda_small": _case(80, 64, prec=3, lam=0.002, start="random", seed=61, want=("chain",)),
    # vectors that wrap when they are doubled
    "wild_vectors": _case(72, 56, prec=2, start="wild", seed=62, want=("inadmissible",)),
}
THREE_UNLIKE = ("precision_0", "block_16x16", "padded_stride")
# over these every one of the eight directions wins somewhere, and so does "none"
DIRECTION_CASES = ("precision_1", "precision_2", "precision_3")


# The sub-pel positions (x & 1, y & 1) of pass 2 and (x & 3, y & 3) of pass 3 a candidate can have.  The centre is a
# doubled vector on a block origin that is a multiple of 2 ^ mvprec: both coordinates even; the eight candidates move at
# least one coordinate by one.  So a candidate never has two even coordinates: 3 of the 4 positions of pass 2 and 12 of the
# 16 of pass 3 occur, never the half-pel block itself, and pass 3 never takes the two-tap average (pass 2 does, as (1, 0)
# and (0, 1)).
POSITIONS = {2: {(a, b) for a in range(2) for b in range(2) if a & 1 or b & 1}, 3: {(a, b) for a in range(4) for b in range(4) if a & 1 or b & 1}}


def params_of(c):
    return dict(x_num_blocks=c["nbx"], y_num_blocks=c["nby"], xbsep_luma=c["xb"], ybsep_luma=c["yb"])


def full_pel_sad(src, ref, c, i, j, dx, dy):
    """The SAD of block (i, j) at a full-pel vector, coordinates clamped to the picture: a plausible level-0 metric."""
    h, w = src.shape
    x0, y0 = i * c["xb"], j * c["yb"]
    bw, bh = min(c["xb"], w - x0), min(c["yb"], h - y0)
    ys, xs = np.clip(np.arange(y0, y0 + bh) + dy, 0, h - 1), np.clip(np.arange(x0, x0 + bw) + dx, 0, w - 1)
    return int(np.abs(src[y0:y0 + bh, x0:x0 + bw].astype(np.int32) - ref[np.ix_(ys, xs)]).sum())


def start_field(c, src, ref):
    """The level-0 field a case starts from.  near: the true motion plus or minus 1, the metric the SAD there; random:
    RH.random_field's small vectors with that metric; bounds: the border blocks' vectors put ON the admissibility bounds of
    pass 1; wild: a share of vectors far outside.  Flags, chroma_metric and the other reference's vector are noise that
    must survive."""
    nbx, nby, r = c["nbx"], c["nby"], c["ref_index"]
    rng = np.random.default_rng(c["seed"] + 3000)
    f = RH.random_field(nbx, nby, 0, c["seed"] + 2000, reach=3, wild=0.3 if c["start"] == "wild" else 0.0).copy()
    f["chroma_metric"] = rng.integers(0, 1 << 16, f.size)
    v = f["v"]
    if c["start"] in ("near", "bounds"):
        v[:, r] = MOTION[0] + rng.integers(-1, 2, f.size)
        v[:, 2 + r] = MOTION[1] + rng.integers(-1, 2, f.size)
    if c["start"] == "bounds":
        e, w, h, xb, yb = c["ext"], c["w"], c["h"], c["xb"], c["yb"]
        last_i, last_j = min(nbx, -(-w // xb)) - 1, min(nby, -(-h // yb)) - 1
        for j in range(nby):
            for i in range(nbx):
                n = j * nbx + i
                # pass 1 has x = 2 * (i * xb + dx): -e is the first inadmissible position on the left, 2 w + e - xb the
                # last admissible one on the right
                if i == 0:
                    v[n][r] = -(e // 2)
                elif i == last_i:
                    v[n][r] = w + (e - xb) // 2 - i * xb
                if j == 0:
                    v[n][2 + r] = -(e // 2)
                elif j == last_j:
                    v[n][2 + r] = h + (e - yb) // 2 - j * yb
    for j in range(nby):
        for i in range(nbx):
            if i * c["xb"] < c["w"] and j * c["yb"] < c["h"]:
                n = j * nbx + i
                f["metric"][n] = full_pel_sad(src, ref, c, i, j, int(v[n][r]), int(v[n][2 + r]))
    return f


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(src, ref, start field) of a case; read-only."""
    c = CASES[name]
    return make_inputs(tuple(sorted(c.items())))


@functools.lru_cache(maxsize=None)
def make_inputs(items):
    c = dict(items)
    w, h, seed = c["w"], c["h"], c["seed"]
    if c["picture"] == "flat":
        src, ref = np.full((h, w), 77, np.uint8), np.full((h, w), 77, np.uint8)
    else:
        src = RH.texture(w, h, seed)
        ref = RH.moved(src, MOTION[0], MOTION[1], seed + 1000)
    field = start_field(c, src.astype(np.int32), ref.astype(np.int32))
    for a in (src, ref, field):
        a.setflags(write=False)
    return src, ref, field


def reference(c, src, ref, field, **kw):
    return R.subpel_deep(src, ref, params_of(c), c["prec"], c["ref_index"], c["lam"], field, c["ext"], **kw)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(field, tables, stats) of a case by tests/subpel_ref.py; read-only."""
    c = CASES[name]
    src, ref, start = inputs(name)
    stats = {}
    field, tables = reference(c, src, ref, start, stats=stats)
    r = c["ref_index"]
    off = np.array([i * c["xb"] >= c["w"] or j * c["yb"] >= c["h"] for j in range(c["nby"]) for i in range(c["nbx"])])
    stats["unshifted"] = int(off.sum()) if c["prec"] and np.array_equal(field[off], start[off]) and start["v"][off][:, [r, 2 + r]].any() else 0
    if "chain" in c["want"]:
        stale, _ = reference(c, src, ref, start, stale_neighbours=True)
        stats["chain"] = int((stale["v"] != field["v"]).any(axis=1).sum())
    stats["none_only"] = int(stats["wins"][0] > 0 and not any(stats["wins"][1:]))
    for key in c["want"]:
        if key == "positions2":
            assert stats[key] == POSITIONS[2], (name, stats[key])
        elif key == "positions3":
            assert stats[key] == POSITIONS[3], (name, stats[key])
        else:
            assert stats[key] > 0, (name, key, stats)
    # what the pass must not touch: flags, chroma_metric, the other reference's vector
    for key in ("flags", "chroma_metric"):
        assert np.array_equal(field[key], start[key]), name
    assert np.array_equal(field["v"][:, [1 - r, 3 - r]], start["v"][:, [1 - r, 3 - r]]), name
    assert len(tables) == c["prec"]
    field.setflags(write=False)
    for t in tables:
        t.setflags(write=False)
    return field, tables, stats


@functools.lru_cache(maxsize=None)
def fields_by_pass(name):
    """[the start field, the field behind pass 1, behind pass 2, ..] of a case; read-only."""
    c = CASES[name]
    src, ref, start = inputs(name)
    out = [R.subpel_deep(src, ref, params_of(c), p, c["ref_index"], c["lam"], start, c["ext"])[0] for p in range(c["prec"] + 1)]
    assert out[0].tobytes() == start.tobytes() and out[-1].tobytes() == expected(name)[0].tobytes()
    for f in out:
        f.setflags(write=False)
    return out


# ---- the rounding case: a choice from crafted tables ------------------------------------------------------------------

ROUNDING = dict(w=64, h=48, xb=8, yb=8, nbx=8, nby=6, prec=1, ref_index=0, ext=32, lam=0.1, pad=0)


@functools.lru_cache(maxsize=None)
def rounding():
    """(src, start field, tables, field, fused field): lambda 0.1 -- the reference's own (schroencoder.c:80,109) -- and, per
    candidate, an error that puts its score ON the centre's in exact arithmetic (ten of error per bit of entropy), so
    that the two roundings of `entropy + lambda * error` decide, as they do for entropy 27, metric 2557 against entropy
    25, error 2577.  Searched: the first seed whose unfused and fused results differ."""
    c = ROUNDING
    P = params_of(c)
    src = np.zeros((c["h"], c["w"]), np.uint8)         # (the choice reads no picture: only its size)
    for seed in range(64):
        rng = np.random.default_rng(7000 + seed)
        f = RH.random_field(c["nbx"], c["nby"], 0, 7100 + seed, reach=6).copy()
        f["metric"] = rng.integers(1500, 4000, f.size)
        table = np.zeros((f.size, 8), np.int32)
        v = f["v"].astype(np.int64) * 2
        for n in range(f.size):
            i, j = n % c["nbx"], n // c["nbx"]
            px, py = R.vector_prediction(v, c["nbx"], i, j, 0)         # (from the unrefined neighbours: near enough)
            e0 = R.estimate_sint(v[n][0] - px) + R.estimate_sint(v[n][2] - py)
            for k, (mx, my) in enumerate(R.MATCHES):
                ek = R.estimate_sint(v[n][0] + mx - px) + R.estimate_sint(v[n][2] + my - py)
                table[n][k] = max(int(f["metric"][n]) + 10 * (e0 - ek), 0)
        table[rng.random(table.shape) < 0.1] = -1
        plain, _ = R.subpel_deep(src, None, P, 1, 0, c["lam"], f, c["ext"], tables=[table])
        fused, _ = R.subpel_deep(src, None, P, 1, 0, c["lam"], f, c["ext"], tables=[table], fused=True)
        if (plain["v"] != fused["v"]).any() or (plain["metric"] != fused["metric"]).any():
            for a in (src, f, table, plain, fused):
                a.setflags(write=False)
            return src, f, table, plain, fused
    raise AssertionError("no seed separates the unfused from the fused score")


# ---- seeded draws -------------------------------------------------------------------------------------------------------

N_DRAWS = 20
SEPARATIONS = tuple(range(4, 33, 4))


def draw_case(n):
    """Geometry n: sizes 17 .. 120, every separation 4 .. 32 in steps of 4 (draw n takes separation n mod 8 in x and a
    permutation of it in y), an extension between the block and 32, every lambda of LAMBDAS."""
    rng = np.random.default_rng(9000 + n)
    xb, yb = SEPARATIONS[n % 8], SEPARATIONS[(3 * n + n // 8) % 8]
    w, h = int(rng.integers(17, 121)), int(rng.integers(17, 121))
    ext = int(rng.integers(max(xb, yb), 33))
    c = _case(w, h, xb=xb, yb=yb, prec=int(rng.integers(1, 4)), ref_index=int(rng.integers(0, 2)), ext=ext, lam=LAMBDAS[n % len(LAMBDAS)],
              pad=int(rng.integers(0, 3)) * 13, start=("near", "random", "bounds")[n % 3], seed=9100 + n, superblocks=bool(n % 2))
    return c


@functools.lru_cache(maxsize=None)
def draw(n):
    """(case, src, ref, start field, field, tables) of draw n."""
    c = draw_case(n)
    src, ref, start = make_inputs(tuple(sorted(c.items())))
    field, tables = reference(c, src, ref, start)
    return c, src, ref, start, field, tables


# ---- refusals -------------------------------------------------------------------------------------------------------------

# What tests/test_gpu_subpel.py::test_a_refused_call_writes_nothing spoils in the second of two chains, one at a time.
REFUSED_CASE = "precision_1"
REFUSED_MEMBERS = (("prec", 4), ("prec", -1), ("xb", 33), ("yb", 0), ("nbx", 0), ("ref_index", 2), ("ext", 7), ("ext", 33), ("lam", -1.0),
                   ("lam", float("nan")), ("lam", float("inf")), ("stride", -1))
