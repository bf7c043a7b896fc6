"""The named cases of the whole mode decision: inputs, and what tests/mode_ref.py makes of them (computed once per case
and process).  Pictures and sub-pel fields are tests/split2_cases.py's, at sizes that give 3 x 3 superblocks -- a
superblock then has all three neighbours -- up to 160 x 128; `block_32x32` is the one-superblock clipped and padded grid.
The `want` tuple of a case says what it is there for; `expected` asserts it on the CPU.

The level-1 and level-2 fields are synthetic full grids: noise everywhere, and at the records that are read (every 2 and
every 4 blocks) the true motion in whole pixels plus or minus one, with, by the record's number,
    % 7 == 3    metric INT_MAX (the hint is skipped),
    % 7 == 5    the vector that, shifted by the precision, equals the quadrant's first sub-pel vector (dropped: the shift is right),
    % 11 == 6   the first sub-pel vector itself, unshifted (kept at precision > 0 although it names another place),
    % 13 == 9   a vector far outside the picture (fails the bound test).
`start`:
    near        split2_cases' fields: the true motion plus or minus one unit of the precision
    doubles     in every quadrant the first sub-pel vector is the true motion m << precision, the second is m UNSHIFTED --
                another place, yet rule 2's shift makes it the first one's equal and drops it -- and the third is a true
                copy of the first, which the same shift keeps
    no_hints    every sub-pel and level record of reference 1 has metric INT_MAX in the quadrants chosen by `holes`
    all_int_max every level-1 and level-2 record has metric INT_MAX (the agreement with the split-2 stage is run on this)"""
import functools

import numpy as np

import mode_ref as M
import split2_cases as K
import split2_ref as R

INT_MAX = R.INT_MAX
LAMBDAS = K.LAMBDAS


def _case(w, h, levels="near", holes=(), **kw):
    c = K._case(w, h, **kw)
    c["levels"], c["holes"] = levels, tuple(holes)
    return c


CASES = {
    "precision_0": _case(96, 96, prec=0, seed=51, want=("split1", "split2")),
    "precision_1": _case(96, 96, prec=1, seed=52, want=("split1", "rule6_absent")),
    "precision_2": _case(96, 96, prec=2, seed=53, want=("rule6",)),
    "precision_3": _case(96, 96, prec=3, seed=54, want=("rule6",)),
    "block_4x4": _case(48, 48, xb=4, yb=4, prec=3, ext=4, seed=55),
    "block_16x8": _case(160, 96, xb=16, yb=8, prec=2, ext=16, fmt="422", seed=56),
    "block_32x32": _case(100, 75, xb=32, yb=32, prec=2, fmt="444", seed=57, want=("rule6",)),
    "clipped_padded": _case(101, 75, prec=2, seed=58, want=("outside_quadrant",)),
    "padded_x": _case(100, 96, prec=1, seed=59, want=("outside_quadrant",)),
    "format_444": _case(96, 96, prec=1, fmt="444", seed=60),
    "one_reference": _case(96, 96, prec=2, refs=1, seed=61, want=("single_4",)),
    "one_reference_padded": _case(104, 88, prec=1, refs=1, pad=37, seed=62, want=("outside_quadrant",)),
    "doubles": _case(96, 96, prec=1, start="doubles", seed=63, want=("dropped_by_the_shift", "kept_by_the_shift")),
    "doubles_precision_3": _case(96, 96, prec=3, start="doubles", seed=64, want=("dropped_by_the_shift", "kept_by_the_shift")),
    "invalid_first_quadrant": _case(96, 96, prec=2, levels="no_hints", holes=(0,), refs=1, seed=65, want=("invalid_q0",)),
    "invalid_later_quadrant": _case(96, 96, prec=1, levels="no_hints", holes=(2, 3), refs=1, seed=66, want=("invalid_later",)),
    "flat": _case(96, 96, prec=2, picture="flat", start="same", seed=67),
    "lambda_0": _case(96, 96, prec=2, lam=0, seed=68),
    "lambda_small": _case(96, 96, prec=3, lam=0.002, seed=69),
    "lambda_10": _case(96, 96, prec=1, lam=10, seed=70),
    "all_int_max": _case(96, 96, prec=2, refs=1, levels="all_int_max", start="int_max", seed=71),
}
THREE_UNLIKE = ("block_32x32", "one_reference_padded", "block_16x8")


def params_of(c):
    return K.params_of(c)


def level_fields(c, fields):
    """(level-1 fields, level-2 fields), one of each per reference."""
    nbx, nby, p = c["nbx"], c["nby"], c["prec"]
    out = ([], [])
    for level, step in ((0, 2), (1, 4)):
        for r in range(c["refs"]):
            rng = np.random.default_rng(c["seed"] + 5000 + 10 * level + r)
            f = np.zeros(nbx * nby, R.MV_DTYPE)
            f["flags"] = rng.integers(0, 1 << 32, f.size, dtype=np.uint64).astype(np.uint32) & ~np.uint32(4)
            f["metric"] = rng.integers(0, 1 << 20, f.size)
            f["chroma_metric"] = rng.integers(0, 1 << 16, f.size)
            v = rng.integers(-9, 10, (f.size, 4)).astype(np.int16)
            for y in range(0, nby, step):
                for x in range(0, nbx, step):
                    n = y * nbx + x
                    v[n][r] = K.MOTIONS[r][0] + rng.integers(-1, 2)
                    v[n][2 + r] = K.MOTIONS[r][1] + rng.integers(-1, 2)
                    first = fields[r]["v"][n]
                    if n % 7 == 5:
                        v[n][r], v[n][2 + r] = int(first[r]) >> p, int(first[2 + r]) >> p
                    if n % 11 == 6:
                        v[n][r], v[n][2 + r] = first[r], first[2 + r]
                    if n % 13 == 9:
                        v[n][r] = -(c["w"] + 3 * c["ext"])
                    if n % 7 == 3 or c["levels"] == "all_int_max":
                        f["metric"][n] = INT_MAX
                    if c["levels"] == "no_hints" and r == 0 and (((x >> 1) & 1) + 2 * ((y >> 1) & 1) in c["holes"]):
                        f["metric"][n] = INT_MAX
            f["v"] = v
            out[level].append(f)
    return out


def sub_pel_fields(c, src, refs):
    fields = [f.copy() for f in K.start_fields(c, src, refs)]
    nbx, nby = c["nbx"], c["nby"]
    for r, f in enumerate(fields):
        f["flags"] &= ~np.uint32(4)                     # (using_global set in a hint is rule 11's own test)
        for y in range(0, nby, 2):
            for x in range(0, nbx, 2):
                n = y * nbx + x
                if c["start"] == "doubles":
                    v = f["v"]
                    mx, my = K.MOTIONS[r]
                    v[n][r], v[n][2 + r] = mx << c["prec"], my << c["prec"]
                    v[n + 1][r], v[n + 1][2 + r] = mx, my
                    v[n + nbx][r], v[n + nbx][2 + r] = v[n][r], v[n][2 + r]
                if c["levels"] == "no_hints" and r == 0 and (((x >> 1) & 1) + 2 * ((y >> 1) & 1) in c["holes"]):
                    for k in (n, n + 1, n + nbx, n + nbx + 1):
                        f["metric"][k] = INT_MAX
    return fields


@functools.lru_cache(maxsize=None)
def make_inputs(items):
    c = dict(items)
    src, refs = K.pictures(c)
    fields = sub_pel_fields(c, src, refs)
    level1, level2 = level_fields(c, fields)
    for a in src + [p for r in refs for p in r] + fields + level1 + level2:
        a.setflags(write=False)
    return src, refs, fields, level1, level2


def inputs(name):
    """(src planes, reference planes, sub-pel fields, level-1 fields, level-2 fields) of a case; read-only."""
    return make_inputs(tuple(sorted(CASES[name].items())))


def reference(c, src, refs, fields, level1, level2, **kw):
    return M.mode_decision(src, refs, params_of(c), c["lam"], fields, level1, level2, c["ext"], **kw)


def derived(c, st, trials, table):
    st = dict(st)
    for s in range(3):
        st["split%d" % s] = st["final_split"][s]
    for s in range(5):
        st["single_%d" % s] = st["singles"][s]
    st["outside_quadrant"] = sum(st["outside_quadrant_mode"])
    st["outside_quadrant_mode2"] = st["outside_quadrant_mode"][2]
    st["invalid_q0"] = st["invalid_quadrant"][0]
    st["invalid_later"] = sum(st["invalid_quadrant"][1:])
    st["split0_not_tried"] = int((trials["state"][:, 2] == -1).sum())
    st["split0_invalid"] = int((trials["state"][:, 2] == 0).sum())
    st["split0_lost"] = int(((trials["state"][:, 2] == 1) & (trials["score"][:, 2] >= trials["score"][:, 1])).sum())
    shared = st.get("shared_buffer", 0)                 # the bi-reference trials of split 1, split 0 and the zero vectors
    st["rule6"] = int(c["prec"] > 1 and shared > 0)
    st["rule6_absent"] = int(c["prec"] < 2 and shared == 0)
    return st


@functools.lru_cache(maxsize=None)
def expected(name):
    """(motion, superblocks, trials, statistics, split-2 table, mode table, stats) of a case, raster order; read-only."""
    c = CASES[name]
    stats = {}
    out = reference(c, *inputs(name), stats=stats)
    stats = derived(c, stats, out[2], out[5])
    for key in c["want"]:
        assert stats[key] > 0, (name, key, {k: v for k, v in stats.items() if k != "dropped"})
    for a in out:
        a.setflags(write=False)
    return out + (stats,)


# ---- seeded draws -------------------------------------------------------------------------------------------------------

N_DRAWS = 8


def draw_case(n):
    """Geometry n: 3 x 3 superblocks or a little less, every chroma format, precision and lambda."""
    rng = np.random.default_rng(9500 + n)
    xb, yb = ((4, 4), (8, 8), (8, 4), (12, 8), (4, 8), (8, 12), (16, 8), (8, 8))[n % 8]
    w, h = int(rng.integers(8 * xb + 1, 12 * xb + 1)), int(rng.integers(8 * yb + 1, 12 * yb + 1))
    return _case(w, h, xb=xb, yb=yb, prec=n % 4, refs=1 + (n % 3 != 0), fmt=("420", "422", "444")[n % 3], ext=int(rng.integers(max(xb, yb, 4), 33)),
                 lam=LAMBDAS[n % len(LAMBDAS)], pad=int(rng.integers(0, 3)) * 13, seed=9600 + n)


@functools.lru_cache(maxsize=None)
def draw(n):
    """(case, inputs, outputs) of draw n."""
    c = draw_case(n)
    ins = make_inputs(tuple(sorted(c.items())))
    return c, ins, reference(c, *ins)


# ---- crafted tables: the walk alone ------------------------------------------------------------------------------------

CRAFTED = dict(K._case(96, 96, prec=1, lam=0.1, seed=80), levels="all_int_max", holes=())


def _no_reads(split, x, y, v0, v1):
    raise AssertionError("a crafted case measures no pair of vectors")


def _crafted_inputs(seed, split0_fails):
    """(fields, level1, level2, split-2 table, mode table) of the crafted cases: reference 1 alone has hints."""
    c = CRAFTED
    P = params_of(c)
    nbx, nby = c["nbx"], c["nby"]
    rng = np.random.default_rng(seed)
    fields = []
    for r in (0, 1):
        f = np.zeros(nbx * nby, R.MV_DTYPE)
        f["flags"] = rng.integers(0, 1 << 32, f.size, dtype=np.uint64).astype(np.uint32) & ~np.uint32(4)
        f["metric"] = 400 if r == 0 else INT_MAX
        f["chroma_metric"] = rng.integers(0, 1 << 16, f.size)
        f["v"] = rng.integers(-6, 7, (f.size, 4)).astype(np.int16)
        fields.append(f)
    level1, level2 = level_fields(c, fields)
    table2 = np.zeros((nbx * nby, R.T_INTS), np.int32)
    table2[:, R.T_CHROMA], table2[:, R.T_CHROMA + 1] = 0, 0
    table2[:, R.T_AREA] = 1 << 20
    table2[:, R.T_DC_ERROR] = R.T_NONE
    nsb = nbx * nby // 16
    table = np.full((nsb, M.M_INTS), M.M_NONE, np.int32)
    for s in range(nsb):
        for ref in (0, 1):
            for cand in range(M.M_CANDS):
                e = table[s][ref * M.M_REF_INTS + cand * M.M_CAND_INTS:][:M.M_CAND_INTS]
                e[M.M_OK1] = 1 if cand < 20 else M.M_NONE
                e[M.M_OK0] = int(not split0_fails or s % 3 != 2)
                e[M.M_QUAD:M.M_QUAD + 8] = (200, 100) * 4
                e[10:] = 0
        table[s][M.M_ZERO_BI:] = (1, 1 << 20, 0, 0)

    return fields, level1, level2, table2, table


@functools.lru_cache(maxsize=None)
def crafted():
    """(fields, level1, level2, split-2 table, mode table, outputs of the walk, stats): tables made by hand, so that rule 7
    and an invalid split-0 trial are certain.  Reference 2 has no hint anywhere (every metric INT_MAX), so every quadrant
    is won by reference 1 alone (s = 4: the trial's error is the honest sum minus 4) and no pair is measured -- the walk
    reads no picture.  Every candidate SAD is 300 per quadrant against 400 of luma per block at split 2, lambda 0.1:
    split 1 beats split 2, and split 0 -- the same SADs, a quarter of the entropy -- beats split 1.  In every third
    superblock the split-0 bound tests fail instead: tried and invalid.  The zero-vector trial's error is then set,
    superblock by superblock in raster order, to put its score strictly between split 0's and split 1's: it wins because
    min_score is still split 1's."""
    c = CRAFTED
    P = params_of(c)
    nsb = c["nbx"] * c["nby"] // 16
    fields, level1, level2, table2, table = _crafted_inputs(8000, True)

    def walk(**kw):
        return M.choose(table2, table, P, c["w"], c["h"], c["lam"], fields, level1, level2, _no_reads, **kw)
    for s in range(nsb):
        trials = walk()[2]
        if trials["state"][s][2] != 1:
            continue
        low, high, entropy = float(trials["score"][s][2]), float(trials["score"][s][1]), int(trials["entropy"][s][3])
        assert low < high
        error = int(((low + high) / 2 - entropy) / c["lam"])
        table[s][M.M_ZERO_BI + 1], table[s][M.M_ZERO_BI + 2] = error - error // 3, error // 3
    stats = {}
    out = walk(stats=stats)
    assert stats["rule7"] > 0 and (out[2]["state"][:, 2] == 0).sum() > 0 and stats["singles"][4] == nsb, stats
    for a in fields + level1 + level2 + [table2, table] + list(out):
        a.setflags(write=False)
    return fields, level1, level2, table2, table, out, stats


# ---- refusals -------------------------------------------------------------------------------------------------------------

# the members of a picture as schroedinger_amd.mode_pictures takes it
SRC, REFS, SHIFTS, EXT, PARAMS, LAM, FIELDS, LEVEL1, LEVEL2, MOTION, SBS, TRIALS, STATS = range(13)


def _params(good, **kw):
    return dict(good[1][PARAMS], **kw)


# What is spoilt in the second of two pictures: (member, the value from the two good pictures, what the message says).
REFUSED = (
    (LEVEL1, lambda g: [None] + list(g[1][LEVEL1][1:]), "level-1 field of reference 0"),
    (LEVEL2, lambda g: list(g[1][LEVEL2][:-1]) + [None], "level-2 field of reference"),
    (TRIALS, lambda g: None, "trial table"),
    (STATS, lambda g: None, "statistics"),
    (PARAMS, lambda g: _params(g, x_num_blocks=g[1][PARAMS]["x_num_blocks"] + 4), "superblock outside"),
    (PARAMS, lambda g: _params(g, y_num_blocks=g[1][PARAMS]["y_num_blocks"] + 8), "superblock outside"),
    (PARAMS, lambda g: _params(g, mv_precision=4), "mv_precision"),
    (PARAMS, lambda g: _params(g, x_num_blocks=6), "whole superblocks"),
    (EXT, lambda g: 33, "extension"),
    (LAM, lambda g: -1.0, "lambda"),
    (FIELDS, lambda g: [None] + list(g[1][FIELDS][1:]), "field of reference 0"),
    (MOTION, lambda g: None, "NULL"),
    (TRIALS, lambda g: g[0][TRIALS], "overlaps"),
    (STATS, lambda g: g[0][MOTION], "overlaps"),
    (MOTION, lambda g: g[1][LEVEL1][0], "overlaps"),
    (TRIALS, lambda g: g[1][LEVEL2][0], "overlaps"),
)


def _rounding_search(split):
    """(E, seed) to try.  Split 0: every E on one seed.  Split 1: the hints of quadrant 0 are known beforehand, so only the
    E at which the two roundings of their scores pick different hints, over seeds whose hints differ in entropy."""
    if split == 0:
        for E in range(130, 1000):
            yield E, 8100
        return
    from fractions import Fraction
    nbx = CRAFTED["nbx"]
    for seed in range(8101, 8141):
        v = _crafted_inputs(seed, False)[0][0]["v"]
        ents = [M.S.estimate_sint(int(v[(m >> 1) * nbx + (m & 1)][0])) + M.S.estimate_sint(int(v[(m >> 1) * nbx + (m & 1)][2])) for m in range(4)]
        for E in range(200, 1000):
            plain = [e + float(E - 10 * e) * 0.1 for e in ents]
            fused = [float(Fraction(0.1) * (E - 10 * e) + e) for e in ents]
            if min(range(4), key=lambda k: (plain[k], k)) != min(range(4), key=lambda k: (fused[k], k)):
                yield E, seed


@functools.lru_cache(maxsize=None)
def rounding(split):
    """(fields, level1, level2, split-2 table, mode table, the walk's outputs, the FUSED walk's outputs): crafted tables at
    lambda 0.1 whose candidates of one trial TIE in exact arithmetic, so that the two roundings of `entropy + error *
    lambda` decide -- fused, every candidate rounds to the same score and the first hint keeps the trial; unfused, the
    rounded products differ.  The trial is in the first superblock, whose blocks at (0, 0) have no neighbour: a hint's
    entropy is the estimate of its vector.  split 1: the four sub-pel hints of quadrant 0 get the error E - 10 entropy.
    split 0: every candidate's SADs outside its own quadrant are set so that its sum over the superblock is E - 10 entropy.
    Searched: the first E at which the unfused and the fused walk differ in that trial."""
    c = CRAFTED
    P = params_of(c)
    nbx = c["nbx"]
    for E, seed in _rounding_search(split):
        fields, level1, level2, table2, table = _crafted_inputs(seed, False)
        for cand in range(20):
            q, m = divmod(cand, 5)
            if m == M.M_LEVEL1:
                continue
            v = fields[0]["v"][(2 * (q >> 1) + (m >> 1)) * nbx + 2 * (q & 1) + (m & 1)]
            entropy = M.S.estimate_sint(int(v[0])) + M.S.estimate_sint(int(v[2]))
            e = table[0][cand * M.M_CAND_INTS:][:M.M_CAND_INTS]
            if split == 1 and q == 0:
                total = E - 10 * entropy
                e[M.M_QUAD], e[M.M_QUAD + 1] = total - total // 3, total // 3
            if split == 0:
                rest = E - 10 * entropy - 300      # (its own quadrant keeps 200 + 100)
                for k, other in enumerate(x for x in range(4) if x != q):
                    part = rest // 3 + (rest % 3 if k == 0 else 0)
                    e[M.M_QUAD + 2 * other], e[M.M_QUAD + 2 * other + 1] = part - part // 4, part // 4
        table[:, M.M_ZERO_BI] = 0                       # (the zero vectors stay out of it)
        plain = M.choose(table2, table, P, c["w"], c["h"], c["lam"], fields, level1, level2, _no_reads)
        fused = M.choose(table2, table, P, c["w"], c["h"], c["lam"], fields, level1, level2, _no_reads, fused=True)
        level = 1 if split == 1 else 2
        if plain[2][0][level]["state"] == 1 and plain[2][0][level]["entropy"] != fused[2][0][level]["entropy"]:
            assert plain[0].tobytes() != fused[0].tobytes()
            for a in fields + level1 + level2 + [table2, table] + list(plain) + list(fused):
                a.setflags(write=False)
            return fields, level1, level2, table2, table, plain, fused
    raise AssertionError("no E separates the unfused from the fused score at split %d" % split)
