"""The cases of tests/test_gpu_long_diagonals.py: grids whose anti-diagonals outgrow a wave, then the workgroup, of the
three serial choice kernels that walk them -- subpel_choose_kernel and split2_choose_kernel (256 threads, a block per
thread, walk_diagonals of motion_common.h) and mode_choose_kernel (8 waves, a superblock per wave, rounds of 8) -- with what
tests/subpel_ref.py, tests/split2_ref.py and tests/mode_ref.py make of them (computed once per case and process).  Every
grid has 4 x 4 blocks, so that the pictures stay small; a diagonal is min (cols, rws) long.

The geometry helpers restate the walks: which thread, wave and turn (or wave and round) handles a block, and from that the
BOUNDARY blocks -- those with a left, upper or upper-left neighbour handled by another wave ("wave"), or in another turn
("turn") or round ("round"), than the block itself.  There the hand-over between the waves of the workgroup, with only a
barrier between two diagonals, is what the result rests on.

The witness of a sub-pel or split-2 case, asserted on the CPU (tests/test_long_diagonal_cases.py): the restatement run
again with a "stale" model -- a neighbour across the boundary of that kind yields the record as it was before the call --
gives another record at 8 or more boundary blocks of that kind.  A grid that only just crosses an edge has fewer boundary
blocks than that -- 68 x 66 has 6 at the wave, 260 x 258 has 6 at the turn, the padded grid has 3: rows 64 and 65 (or 256
and 257) reach thread 64 (or the turn) on four diagonals only -- so 8 cannot be had there, and half of them (rounded up)
must differ instead (`needed`).  The wave has its full eight on the wide, tall and 256 grids; for the turn `turn_tall`
(260 x 272) is added to the issue's grids.  The seeds in the table below are the first that give the witness (`find_seed`
is how they were found; the test asserts the recorded one, so nothing searches at run time).  The witness of a mode case
is its geometry: rounds, a partial last round, diagonals that start below the top row.

Every case is also walked in anti-diagonal order and gives the same bytes."""
import functools

import numpy as np

import mode_cases as MC
import mode_ref as M
import rough_hint_cases as RH
import split2_cases as K2
import split2_ref as R2
import subpel_cases as KS
import subpel_ref as RS

WAVE = 64
CHOOSE_THREADS = 256            # kSubpelChooseThreads, kSplit2ChooseThreads
MODE_WAVES = 8                  # kModeChooseWaves
BLOCK = 4
NEEDED = 8


# ---- geometry -------------------------------------------------------------------------------------------------------------

def walk_slot(cols, rws, threads, i, j):
    """(thread, wave, turn) of block (i, j) in walk_diagonals (cols, rws, threadIdx.x, threads, ..)."""
    assert 0 <= i < cols and 0 <= j < rws
    k = j - max(0, i + j - (cols - 1))
    return k % threads, (k % threads) >> 6, k // threads


def mode_slot(sbx, sby, sx, sy):
    """(wave, round) of superblock (sx, sy) in mode_choose_kernel's walk; also the diagonal's first row `lo`."""
    assert 0 <= sx < sbx and 0 <= sy < sby
    lo = max(0, sx + sy - (sbx - 1))
    return (sy - lo) % MODE_WAVES, (sy - lo) // MODE_WAVES, lo


def neighbours(i, j):
    return [(ni, nj) for ni, nj in ((i - 1, j), (i, j - 1), (i - 1, j - 1)) if ni >= 0 and nj >= 0]


def crosses(cols, rws, threads, kind, i, j, ni, nj):
    """Whether neighbour (ni, nj) of block (i, j) is handled by another wave, or in another turn; False off the walk."""
    if not (i < cols and j < rws and ni < cols and nj < rws):
        return False
    a, b = walk_slot(cols, rws, threads, i, j), walk_slot(cols, rws, threads, ni, nj)
    return a[1] != b[1] if kind == "wave" else a[2] != b[2]


@functools.lru_cache(maxsize=None)
def boundary_blocks(cols, rws, threads=CHOOSE_THREADS):
    """{"wave": [(i, j), ..], "turn": [..]} in raster order."""
    out = {"wave": [], "turn": []}
    for j in range(rws):
        for i in range(cols):
            for kind in out:
                if any(crosses(cols, rws, threads, kind, i, j, ni, nj) for ni, nj in neighbours(i, j)):
                    out[kind].append((i, j))
    return out


@functools.lru_cache(maxsize=None)
def mode_boundary(sbx, sby):
    """The superblocks with a neighbour of another round."""
    return [(sx, sy) for sy in range(sby) for sx in range(sbx)
            if any(mode_slot(sbx, sby, nx, ny)[1] != mode_slot(sbx, sby, sx, sy)[1] for nx, ny in neighbours(sx, sy))]


def mode_geometry(sbx, sby):
    """What the mode walk does on a grid: rounds of the longest diagonal, whether some diagonal's last round leaves waves
    idle, whether some diagonal starts below the top row."""
    lengths = [min(d, sby - 1) - max(0, d - (sbx - 1)) + 1 for d in range(sbx + sby - 1)]
    return dict(rounds=-(-max(lengths) // MODE_WAVES), partial_last=int(any(n > MODE_WAVES and n % MODE_WAVES for n in lengths)),
                partial=int(any(n % MODE_WAVES for n in lengths)), lo_positive=int(sby > 1), longest=max(lengths))


def describe_block(cols, rws, i, j, threads=CHOOSE_THREADS):
    """For a failure message: where the walk handles block (i, j)."""
    if not (i < cols and j < rws):
        return "block (%d, %d), outside the walk" % (i, j)
    t, w, turn = walk_slot(cols, rws, threads, i, j)
    kinds = [k for k, blocks in boundary_blocks(cols, rws, threads).items() if (i, j) in blocks]
    return "block (%d, %d): diagonal %d, thread %d, wave %d, turn %d, %s" % (i, j, i + j, t, w, turn,
                                                                          "a boundary block (%s)" % ", ".join(kinds) if kinds else "no boundary block")


def describe_superblock(sbx, sby, sx, sy):
    w, r, lo = mode_slot(sbx, sby, sx, sy)
    return "superblock (%d, %d): diagonal %d from row %d, wave %d, round %d, %s" % (
        sx, sy, sx + sy, lo, w, r, "a boundary superblock" if (sx, sy) in mode_boundary(sbx, sby) else "no boundary superblock")


# ---- the grids of the sub-pel and the split-2 choice ---------------------------------------------------------------------

def _grid(cols, rws, prec, kinds, nbx=None, nby=None, clip=0, subpel_seed=0, split2_seed=0):
    return dict(cols=cols, rws=rws, prec=prec, kinds=tuple(kinds), nbx=nbx or cols, nby=nby or rws, clip=clip, subpel_seed=subpel_seed,
                split2_seed=split2_seed)


# cols x rws: the blocks inside the picture, which the kernels walk; kinds: the boundaries a case is named for.  Each edge
# has its neighbour on the near side: 64 x 64 has no wave boundary, 256 x 256 no turn.
GRIDS = {
    "wave_inside": _grid(64, 64, 3, ()),
    "wave_crossed": _grid(68, 66, 3, ("wave",), subpel_seed=3),
    "turn_inside": _grid(256, 256, 1, ("wave",)),
    "turn_crossed": _grid(260, 258, 1, ("turn",), subpel_seed=2, split2_seed=9),
    # (not the issue's: 260 x 258 has 6 boundary blocks at the turn, this one has the eight and more the witness asks for)
    "turn_tall": _grid(260, 272, 1, ("turn",), split2_seed=1),
    # 66 diagonals of 66 blocks: wide, they start in the top row and thread 64 reads what thread 63 stored; tall, they start
    # below it (jlo > 0) and thread 63 reads what thread 64 stored
    "wide": _grid(132, 66, 2, ("wave",)),
    "tall": _grid(66, 132, 2, ("wave",)),
    # a 68 x 68 grid over a picture of 66 x 65 blocks whose last block lacks a pixel each way: the skipped (sub-pel) or
    # outside (split-2) blocks lie beside blocks of wave 1
    "padded": _grid(66, 65, 3, ("wave",), nbx=68, nby=68, clip=1, split2_seed=12),
}
EMPTY = {"wave_inside": ("wave", "turn"), "wave_crossed": ("turn",), "turn_inside": ("turn",), "wide": ("turn",), "tall": ("turn",), "padded": ("turn",),
         "turn_crossed": (), "turn_tall": ()}


def needed(name, kind):
    """The boundary blocks of a kind at which the stale model must give another record: the issue's 8 -- or, on a grid that
    has fewer than 8 such blocks, half of them (rounded up)."""
    g = GRIDS[name]
    n = len(boundary_blocks(g["cols"], g["rws"])[kind])
    return NEEDED if n >= NEEDED else -(-n // 2)


def _stale(g, kind):
    cols, rws = g["cols"], g["rws"]
    return lambda i, j, ni, nj: crosses(cols, rws, CHOOSE_THREADS, kind, i, j, ni, nj)


def _records_differ(a, b, nbx, blocks):
    a, b = a.view(np.uint8).reshape(-1, 20), b.view(np.uint8).reshape(-1, 20)
    return sum(int((a[j * nbx + i] != b[j * nbx + i]).any()) for i, j in blocks)


# ---- sub-pel ------------------------------------------------------------------------------------------------------------

def subpel_case(name):
    g = GRIDS[name]
    return dict(w=g["cols"] * BLOCK - g["clip"], h=g["rws"] * BLOCK - g["clip"], xb=BLOCK, yb=BLOCK, nbx=g["nbx"], nby=g["nby"], prec=g["prec"],
                ref_index=g["prec"] & 1, ext=16, lam=0.1, pad=0)


def subpel_tables(name, seed):
    """(start field, [table of pass 1, ..]): RH.random_field with a random metric, and per candidate an error some tens
    off the metric -- at lambda 0.1 ten of error weigh a bit of entropy, so the prediction from the neighbours decides --
    with -1 (inadmissible) mixed in."""
    c = subpel_case(name)
    rng = np.random.default_rng(seed)
    f = RH.random_field(c["nbx"], c["nby"], 0, seed + 100, reach=6).copy()
    f["metric"] = rng.integers(1500, 4000, f.size)
    f["chroma_metric"] = rng.integers(0, 1 << 16, f.size)
    tables = []
    for _ in range(c["prec"]):
        t = (f["metric"].astype(np.int64)[:, None] + 10 * rng.integers(-4, 5, (f.size, 8))).astype(np.int32)
        t[rng.random(t.shape) < 0.1] = -1
        tables.append(t)
    return f, tables


def _subpel(c, src, field, tables, **kw):
    return RS.subpel_deep(src, None, KS.params_of(c), len(tables), c["ref_index"], c["lam"], field, c["ext"], tables=tables, **kw)[0]


@functools.lru_cache(maxsize=None)
def subpel_expected(name):
    """(case, src, tables, [the start field, the field behind pass 1, ..]); read-only.  The choice reads no picture: src is
    only its size."""
    c = subpel_case(name)
    src = np.zeros((c["h"], c["w"]), np.uint8)
    start, tables = subpel_tables(name, GRIDS[name]["subpel_seed"])
    fields = [start]
    for t in tables:
        fields.append(_subpel(c, src, fields[-1], [t]))
    for a in [src] + tables + fields:
        a.setflags(write=False)
    return c, src, tables, fields


def subpel_witness(name, seed=None):
    """{kind: boundary blocks of that kind where the stale model's final records differ from the true ones}."""
    g, c = GRIDS[name], subpel_case(name)
    src = np.zeros((c["h"], c["w"]), np.uint8)
    if seed is None:
        _, _, tables, fields = subpel_expected(name)
        start, true = fields[0], fields[-1]
    else:
        start, tables = subpel_tables(name, seed)
        true = _subpel(c, src, start, tables)
    blocks = boundary_blocks(g["cols"], g["rws"])
    return {kind: _records_differ(true, _subpel(c, src, start, tables, stale_neighbours=_stale(g, kind)), c["nbx"], blocks[kind]) for kind in g["kinds"]}


def subpel_diagonal_order(name):
    c, src, tables, fields = subpel_expected(name)
    return _subpel(c, src, fields[0], tables, order="diagonal"), fields[-1]


# the whole stage from pictures, at the 68 x 66 grid only (the restatement reads 8 blocks per block and pass)
SUBPEL_STAGE = KS._case(68 * BLOCK, 66 * BLOCK, xb=BLOCK, yb=BLOCK, prec=2, ext=8, lam=0.1, start="random", seed=70)


@functools.lru_cache(maxsize=None)
def subpel_stage():
    """(case, src, ref, start field, field)"""
    c = SUBPEL_STAGE
    src, ref, start = KS.make_inputs(tuple(sorted(c.items())))
    field, _ = KS.reference(c, src, ref, start)
    field.setflags(write=False)
    return c, src, ref, start, field


# ---- split 2 ------------------------------------------------------------------------------------------------------------

def _up4(n):
    return -(-n // 4) * 4


def split2_case(name):
    g = GRIDS[name]
    return dict(w=g["cols"] * BLOCK - g["clip"], h=g["rws"] * BLOCK - g["clip"], xb=BLOCK, yb=BLOCK, nbx=_up4(g["nbx"]), nby=_up4(g["nby"]), prec=1,
                refs=2, fmt="420", ext=16, lam=0.1, pad=0)


def split2_tables(name, seed):
    """(fields, table), built as split2_cases.rounding builds its own: random fields, and errors of the two single
    references and of the bi-reference trial that lie within a few bits of entropy of one another (ten of error per bit at
    lambda 0.1), so that the entropies -- the predictions from the neighbours -- decide.  One block in ten also has a small
    area and a DC error, so that DC records (which predict nothing) lie among the neighbours."""
    c = split2_case(name)
    g = GRIDS[name]
    n = c["nbx"] * c["nby"]
    rng = np.random.default_rng(seed)
    fields = [RH.random_field(c["nbx"], c["nby"], 0, seed + 100 + r, reach=6).copy() for r in (0, 1)]
    table = np.zeros((n, R2.T_INTS), np.int32)
    base = rng.integers(2000, 4500, n)
    for r, f in enumerate(fields):                      # the two single-reference errors: a few bits of entropy apart
        table[:, R2.T_CHROMA + r] = rng.integers(200, 900, n)
        f["metric"] = base + 10 * rng.integers(-2, 3, n) - table[:, R2.T_CHROMA + r]
    table[:, R2.T_BI_OK] = 1
    total = base - 10 * rng.integers(3, 11, n)
    table[:, R2.T_BI_LUMA], table[:, R2.T_BI_CHROMA] = total - total // 3, total // 3
    dc = rng.random(n) < 0.1
    table[:, R2.T_AREA] = np.where(dc, BLOCK * BLOCK + 2 * (BLOCK // 2) ** 2, 1 << 20)
    table[:, R2.T_DC_ERROR] = np.where(dc, rng.integers(1000, 4000, n), R2.T_NONE)
    table[:, R2.T_DC:R2.T_DC + 3] = np.where(dc[:, None], rng.integers(-128, 128, (n, 3)), 0)
    j, i = np.divmod(np.arange(n), c["nbx"])
    outside = (i >= g["cols"]) | (j >= g["rws"])
    table[outside] = 0                                  # as split2_ref.metric_tables leaves a block outside the picture
    for k in (R2.T_CHROMA, R2.T_CHROMA + 1, R2.T_DC_ERROR):
        table[outside, k] = R2.T_NONE
    return fields, table


def _split2(c, fields, table, **kw):
    return R2.choose(table, K2.params_of(c), c["w"], c["h"], c["lam"], fields, **kw)


@functools.lru_cache(maxsize=None)
def split2_expected(name):
    """(case, fields, table, motion, superblocks); read-only."""
    c = split2_case(name)
    fields, table = split2_tables(name, GRIDS[name]["split2_seed"])
    motion, sb = _split2(c, fields, table)
    for a in fields + [table, motion, sb]:
        a.setflags(write=False)
    return c, fields, table, motion, sb


def split2_witness(name, seed=None):
    g, c = GRIDS[name], split2_case(name)
    if seed is None:
        _, fields, table, true, _ = split2_expected(name)
    else:
        fields, table = split2_tables(name, seed)
        true = _split2(c, fields, table)[0]
    blocks = boundary_blocks(g["cols"], g["rws"])
    return {kind: _records_differ(true, _split2(c, fields, table, stale=_stale(g, kind))[0], c["nbx"], blocks[kind]) for kind in g["kinds"]}


def split2_diagonal_order(name):
    c, fields, table, motion, sb = split2_expected(name)
    return _split2(c, fields, table, order="diagonal"), (motion, sb)


def find_seed(stage, name, first=0, tries=64):
    """The first seed whose witness reaches `needed` for every kind the grid is named for."""
    witness = subpel_witness if stage == "subpel" else split2_witness
    for seed in range(first, first + tries):
        got = witness(name, seed)
        if all(got[kind] >= needed(name, kind) for kind in GRIDS[name]["kinds"]):
            return seed
    raise AssertionError("no seed gives the witness of %s %s" % (stage, name))


# the whole stage from pictures at 68 x 66 blocks (the grid is padded to 68 x 68)
SPLIT2_STAGE = K2._case(68 * BLOCK, 66 * BLOCK, xb=BLOCK, yb=BLOCK, prec=1, ext=16, seed=71)


@functools.lru_cache(maxsize=None)
def split2_stage():
    """(case, src, refs, fields, motion, superblocks)"""
    c = SPLIT2_STAGE
    src, refs, fields = K2.make_inputs(tuple(sorted(c.items())))
    motion, sb, _ = K2.reference(c, src, refs, fields)
    for a in (motion, sb):
        a.setflags(write=False)
    return c, src, refs, fields, motion, sb


# ---- the mode decision ----------------------------------------------------------------------------------------------------

def _mode(sbx, sby, clip=0, want=(), **kw):
    c = MC._case(4 * BLOCK * sbx - clip, 4 * BLOCK * sby - clip, xb=BLOCK, yb=BLOCK, ext=16, **kw)
    assert (c["nbx"], c["nby"]) == (4 * sbx, 4 * sby)
    c["want"] = tuple(want)
    return c


# in superblocks: 8 x 8 stays inside one round, 10 x 9 takes a second; 12 x 3 and 3 x 12 leave waves idle on diagonals that
# start below the top row; 18 x 17 over a picture clipped by 5 px takes three rounds, its last column and row partly outside
MODE_CASES = {
    "round_inside": _mode(8, 8, prec=1, seed=81, want=("one_round",)),
    "round_crossed": _mode(10, 9, prec=2, seed=82, want=("rounds2", "partial_last", "lo_positive")),
    "wide": _mode(12, 3, prec=3, seed=83, want=("one_round", "partial", "lo_positive")),
    "tall": _mode(3, 12, prec=1, refs=1, seed=84, want=("one_round", "partial", "lo_positive")),
    "three_rounds_padded": _mode(18, 17, clip=5, prec=2, seed=85, want=("rounds3", "partial_last", "lo_positive")),
}


def mode_grid(name):
    c = MODE_CASES[name]
    return c["nbx"] // 4, c["nby"] // 4


def mode_inputs(name):
    return MC.make_inputs(tuple(sorted(MODE_CASES[name].items())))


@functools.lru_cache(maxsize=None)
def mode_expected(name):
    """(motion, superblocks, trials, statistics, split-2 table, mode table, stats) of a case, raster order; read-only."""
    c = MODE_CASES[name]
    stats = {}
    out = MC.reference(c, *mode_inputs(name), stats=stats)
    stats = MC.derived(c, stats, out[2], out[5])
    geo = mode_geometry(*mode_grid(name))
    stats.update(geo, one_round=int(geo["rounds"] == 1), rounds2=int(geo["rounds"] >= 2), rounds3=int(geo["rounds"] >= 3))
    for key in c["want"]:
        assert stats[key] > 0, (name, key, geo)
    for a in out:
        a.setflags(write=False)
    return out + (stats,)


def mode_diagonal_order(name):
    c = MODE_CASES[name]
    src, refs, fields, level1, level2 = mode_inputs(name)
    out = mode_expected(name)
    P = MC.params_of(c)
    return M.choose(out[4], out[5], P, c["w"], c["h"], c["lam"], fields, level1, level2, M.picture_reader(src, refs, P, c["ext"]), order="diagonal"), out[:4]
