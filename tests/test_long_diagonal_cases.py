"""CPU: the cases of tests/long_diagonal_cases.py.  The geometry helpers equal a brute-force run of the kernels' loops; the
boundary lists are empty on the near side of every edge and not beyond it; every sub-pel and split-2 case has its witness
(a stale neighbour across the boundary changes boundary blocks), every mode case its rounds; and the anti-diagonal order
gives the bytes of the raster order on every case."""
import pathlib
import re

import numpy as np
import pytest

import long_diagonal_cases as L

CSRC = pathlib.Path(__file__).resolve().parent.parent / "schroedinger_amd" / "csrc"
CROSSING = sorted(n for n, g in L.GRIDS.items() if g["kinds"])


def brute_walk(cols, rws, threads):
    """walk_diagonals (motion_common.h) as every thread runs it: {(i, j): (thread, wave, turn)}."""
    out = {}
    for d in range(cols + rws - 1):
        jlo, jhi = max(0, d - (cols - 1)), min(d, rws - 1)
        for first in range(threads):
            for turn, j in enumerate(range(jlo + first, jhi + 1, threads)):
                assert (d - j, j) not in out
                out[d - j, j] = (first, first >> 6, turn)
    return out


def brute_mode_walk(sbx, sby):
    """mode_choose_kernel's loops: {(sx, sy): (wave, round, lo)}."""
    out = {}
    for d in range(sbx + sby - 1):
        lo, hi = max(0, d - (sbx - 1)), min(d, sby - 1)
        for rnd, base in enumerate(range(lo, hi + 1, L.MODE_WAVES)):
            for wave in range(L.MODE_WAVES):
                if base + wave <= hi:
                    assert (d - base - wave, base + wave) not in out
                    out[d - base - wave, base + wave] = (wave, rnd, lo)
    return out


def test_the_constants_are_the_kernels():
    for file, name, value in (("subpel.hip", "kSubpelChooseThreads", L.CHOOSE_THREADS), ("mode_split2.hip", "kSplit2ChooseThreads", L.CHOOSE_THREADS),
                              ("mode_decision.hip", "kModeChooseWaves", L.MODE_WAVES)):
        found = re.search(r"constexpr int %s = (\d+);" % name, (CSRC / file).read_text())
        assert found and int(found.group(1)) == value, name


@pytest.mark.parametrize("threads", [4, 64, 256])
@pytest.mark.parametrize("grid", [(1, 1), (5, 3), (3, 5), (7, 7), (9, 70), (70, 9), (68, 66), (131, 140), (270, 261)])
def test_walk_slot_is_the_walk(grid, threads):
    cols, rws = grid
    want = brute_walk(cols, rws, threads)
    assert len(want) == cols * rws
    for (i, j), slot in want.items():
        assert L.walk_slot(cols, rws, threads, i, j) == slot, (i, j)
    if threads == 4 and max(grid) <= 9:                 # the boundary lists against the brute-force slots
        got = L.boundary_blocks(cols, rws, threads)
        for kind, k in (("wave", 1), ("turn", 2)):
            assert got[kind] == [(i, j) for j in range(rws) for i in range(cols) if any(want[n][k] != want[i, j][k] for n in L.neighbours(i, j))]


@pytest.mark.parametrize("grid", [(1, 1), (3, 3), (8, 8), (9, 8), (10, 9), (12, 3), (3, 12), (18, 17), (30, 26)])
def test_mode_slot_is_the_walk(grid):
    sbx, sby = grid
    want = brute_mode_walk(sbx, sby)
    assert len(want) == sbx * sby
    for (sx, sy), slot in want.items():
        assert L.mode_slot(sbx, sby, sx, sy) == slot, (sx, sy)
    assert L.mode_boundary(sbx, sby) == [(sx, sy) for sy in range(sby) for sx in range(sbx)
                                         if any(want[n][1] != want[sx, sy][1] for n in L.neighbours(sx, sy))]
    geo = L.mode_geometry(sbx, sby)
    assert geo["rounds"] == 1 + max(s[1] for s in want.values()) and geo["lo_positive"] == int(any(s[2] > 0 for s in want.values()))


@pytest.mark.parametrize("name", sorted(L.GRIDS))
def test_boundary_lists_are_empty_on_the_near_side_only(name):
    g = L.GRIDS[name]
    blocks = L.boundary_blocks(g["cols"], g["rws"])
    for kind in ("wave", "turn"):
        assert (not blocks[kind]) == (kind in L.EMPTY[name]), (name, kind, len(blocks[kind]))
        assert kind not in g["kinds"] or blocks[kind]
    longest = min(g["cols"], g["rws"])
    assert (longest > L.WAVE) == bool(blocks["wave"]) and (longest > L.CHOOSE_THREADS) == bool(blocks["turn"])
    for kind in g["kinds"]:                             # a boundary block says so in a failure message
        i, j = blocks[kind][0]
        assert "a boundary block" in L.describe_block(g["cols"], g["rws"], i, j) and kind in L.describe_block(g["cols"], g["rws"], i, j)
    assert "no boundary block" in L.describe_block(g["cols"], g["rws"], 0, 0)


def test_wide_and_tall_cross_the_wave_both_ways():
    """While a diagonal starts in the top row a block's UPPER neighbours have the thread before its own: the boundary block
    is thread 64 (wide).  Below the top row (jlo > 0) its LEFT neighbour has the thread after its own: the boundary block is
    thread 63, in wave 0, and reads what wave 1 stored (tall)."""
    for name, below_top, thread in (("wide", False, 64), ("tall", True, 63)):
        g = L.GRIDS[name]
        cols, rws = g["cols"], g["rws"]
        blocks = [(i, j) for i, j in L.boundary_blocks(cols, rws)["wave"] if (i + j - (cols - 1) > 0) == below_top]
        assert len(blocks) >= 60 and all(L.walk_slot(cols, rws, L.CHOOSE_THREADS, i, j)[0] == thread for i, j in blocks)


def test_the_padded_grid():
    """cols < nbx and rws < nby, the last block lacks a pixel each way, and blocks the walk leaves out lie beside wave 1."""
    g = L.GRIDS["padded"]
    for c in (L.subpel_case("padded"), L.split2_case("padded")):
        cols, rws = -(-c["w"] // c["xb"]), -(-c["h"] // c["yb"])
        assert (cols, rws) == (g["cols"], g["rws"]) and cols < c["nbx"] and rws < c["nby"]
        assert c["w"] % c["xb"] == c["xb"] - 1 and c["h"] % c["yb"] == c["yb"] - 1
    wave1 = [(i, j) for j in range(g["rws"]) for i in range(g["cols"]) if L.walk_slot(g["cols"], g["rws"], L.CHOOSE_THREADS, i, j)[1] == 1]
    assert wave1 and any(j + 1 == g["rws"] for i, j in wave1)
    # sub-pel: the skipped records are not even shifted; split 2: the outside records are the constant best_mv
    c, _, _, fields = L.subpel_expected("padded")
    j, i = np.divmod(np.arange(c["nbx"] * c["nby"]), c["nbx"])
    off = (i >= g["cols"]) | (j >= g["rws"])
    assert off.any() and fields[-1][off].tobytes() == fields[0][off].tobytes() and fields[0]["v"][off].any()
    c, _, _, motion, _ = L.split2_expected("padded")
    assert all(motion[n].tobytes() == L.R2.BEST_MV for n in np.flatnonzero(off))


@pytest.mark.parametrize("name", CROSSING)
def test_subpel_witness(name):
    got = L.subpel_witness(name)
    for kind in L.GRIDS[name]["kinds"]:
        assert got[kind] >= L.needed(name, kind), (name, kind, got)


@pytest.mark.parametrize("name", CROSSING)
def test_split2_witness(name):
    got = L.split2_witness(name)
    for kind in L.GRIDS[name]["kinds"]:
        assert got[kind] >= L.needed(name, kind), (name, kind, got)


def test_needed_is_the_issue_s_eight_wherever_a_grid_has_them():
    for name, g in L.GRIDS.items():
        for kind in g["kinds"]:
            n = len(L.boundary_blocks(g["cols"], g["rws"])[kind])
            assert L.needed(name, kind) == (L.NEEDED if n >= L.NEEDED else -(-n // 2)) and L.needed(name, kind) >= 1
    # each kind has a grid that gives the full eight
    assert all(any(kind in g["kinds"] and L.needed(n, kind) == L.NEEDED for n, g in L.GRIDS.items()) for kind in ("wave", "turn"))


@pytest.mark.parametrize("name", sorted(L.GRIDS))
def test_subpel_orders_agree(name):
    c, src, tables, fields = L.subpel_expected(name)
    assert len(fields) == c["prec"] + 1 == L.GRIDS[name]["prec"] + 1
    again, want = L.subpel_diagonal_order(name)         # (all passes in one call, against the passes chained)
    assert again.tobytes() == want.tobytes()
    r = c["ref_index"]
    assert (fields[-1]["v"][:, [r, 2 + r]] != 2 ** c["prec"] * fields[0]["v"][:, [r, 2 + r]]).any(axis=1).mean() > 0.25       # (the passes do move vectors)


@pytest.mark.parametrize("name", sorted(L.GRIDS))
def test_split2_orders_agree(name):
    (motion, sb), want = L.split2_diagonal_order(name)
    assert motion.tobytes() == want[0].tobytes() and sb.tobytes() == want[1].tobytes()
    modes = np.bincount(want[0]["flags"] & 3, minlength=4)
    assert (modes > 0).all(), modes                     # DC, either reference and both all win somewhere


def test_the_stages_from_pictures():
    c, src, ref, start, field = L.subpel_stage()
    assert (c["nbx"], c["nby"]) == (68, 66) and src.shape == (264, 272)
    again, _ = L.KS.reference(c, src, ref, start, order="diagonal")
    assert again.tobytes() == field.tobytes() and field.tobytes() != start.tobytes()
    c, src, refs, fields, motion, sb = L.split2_stage()
    assert (c["nbx"], c["nby"]) == (68, 68) and src[0].shape == (264, 272)
    m2, sb2, _ = L.K2.reference(c, src, refs, fields, order="diagonal")
    assert m2.tobytes() == motion.tobytes() and sb2.tobytes() == sb.tobytes()


@pytest.mark.parametrize("name", sorted(L.MODE_CASES))
def test_mode_case(name):
    """The wants (asserted by mode_expected): rounds, a partial last round, a diagonal that starts below the top row."""
    out = L.mode_expected(name)
    sbx, sby = L.mode_grid(name)
    stats = out[-1]
    assert stats["longest"] == min(sbx, sby)
    assert bool(L.mode_boundary(sbx, sby)) == (stats["rounds"] > 1) == (name in ("round_crossed", "three_rounds_padded"))
    again, want = L.mode_diagonal_order(name)
    for a, b in zip(again, want):
        assert a.tobytes() == b.tobytes()
    assert all(stats["final_split"][s] > 0 for s in range(3)), stats["final_split"]
    if L.mode_boundary(sbx, sby):
        sx, sy = L.mode_boundary(sbx, sby)[0]
        assert "a boundary superblock" in L.describe_superblock(sbx, sby, sx, sy)


def test_the_mode_grids_are_the_issue_s():
    assert {n: L.mode_grid(n) for n in L.MODE_CASES} == {"round_inside": (8, 8), "round_crossed": (10, 9), "wide": (12, 3), "tall": (3, 12),
                                                         "three_rounds_padded": (18, 17)}
    c = L.MODE_CASES["three_rounds_padded"]
    assert (16 * 18 - c["w"], 16 * 17 - c["h"]) == (5, 5)   # the last block column and row outside, the ones before them partial
    assert c["w"] <= (c["nbx"] - 1) * c["xb"] and c["w"] % c["xb"] and c["h"] <= (c["nby"] - 1) * c["yb"] and c["h"] % c["yb"]
    assert {n: (g["cols"], g["rws"]) for n, g in L.GRIDS.items() if n != "turn_tall"} == {
        "wave_inside": (64, 64), "wave_crossed": (68, 66), "turn_inside": (256, 256), "turn_crossed": (260, 258), "wide": (132, 66), "tall": (66, 132),
        "padded": (66, 65)}
