"""GPU: the three serial choice kernels that walk anti-diagonals inside one workgroup -- subpel_choose_kernel,
split2_choose_kernel, mode_choose_kernel -- on grids whose diagonals outgrow a wave, the workgroup's 256 threads, or the
mode walk's 8 waves (tests/long_diagonal_cases.py), byte for byte against tests/subpel_ref.py, tests/split2_ref.py and
tests/mode_ref.py; scores are compared as bits.  A block there reads records that ANOTHER wave stored one diagonal earlier,
with a barrier between them; tests/test_long_diagonal_cases.py shows on the CPU that a stale read across that boundary
changes the result.

A mismatch is reported with the first differing block in the order of the walk and with the thread, wave and turn (or wave
and round) that handles it, so a hand-over bug shows itself as "a boundary block".  Everything lies in guarded blocks
(tests/guard_lib.py), through the rigs of the stages' own tests: a stray write fails the test that did it."""
import zlib

import numpy as np
import pytest

import long_diagonal_cases as L
import mode_cases as MC
import schroedinger_amd as sa
import split2_cases as K2
import subpel_cases as KS
import test_gpu_mode_decision as TM
import test_gpu_split2 as T2
import test_gpu_subpel as TS

pytestmark = pytest.mark.gpu

MV = sa.MV_DTYPE.itemsize


def seed_of(name, k=0):
    return k + (zlib.crc32(name.encode()) & 0xfff0)


def differing(got, want, size):
    """The indices of the `size`-byte entries that differ."""
    a = np.ascontiguousarray(got).view(np.uint8).reshape(-1, size)
    b = np.ascontiguousarray(want).view(np.uint8).reshape(-1, size)
    assert a.shape == b.shape
    return np.flatnonzero((a != b).any(axis=1))


def report_blocks(what, got, want, nbx, cols, rws):
    """Fails with the first differing record in the order of walk_diagonals."""
    bad = differing(got, want, MV)
    if bad.size:
        i, j = min(((int(n % nbx), int(n // nbx)) for n in bad), key=lambda b: (b[0] + b[1], b[1]))
        raise AssertionError("%s: %d of %d records differ, first in the walk's order %s" % (what, bad.size, want.size, L.describe_block(cols, rws, i, j)))


def report_superblocks(what, got, want, size, sbx, sby):
    bad = differing(got, want, size)
    if bad.size:
        sx, sy = min(((int(n % sbx), int(n // sbx)) for n in bad), key=lambda b: (b[0] + b[1], b[1]))
        raise AssertionError("%s: %d of %d entries differ, first in the walk's order %s" % (what, bad.size, sbx * sby, L.describe_superblock(sbx, sby, sx, sy)))


# ---- sub-pel ------------------------------------------------------------------------------------------------------------

def subpel_choice(ctx, entries, seed):
    """entries: (case, src, [(field before, table, field behind) per pass], cols, rws); every pass is one call over all the
    entries that have it."""
    spans = []
    for c, _, passes, _, _ in entries:
        n = c["nbx"] * c["nby"]
        spans.append(dict([("field%d" % p, (n * MV, True)) for p in range(len(passes))] + [("table%d" % p, (n * 32, False)) for p in range(len(passes))]))
    rig = TS.Rig(ctx, [(c, src, src) for c, src, _, _, _ in entries], spans, seed=seed)
    try:
        for p in range(max(len(e[2]) for e in entries)):
            ks = [k for k, e in enumerate(entries) if p < len(e[2])]
            for k in ks:
                rig.put(k, "field%d" % p, entries[k][2][p][0])
                rig.put(k, "table%d" % p, entries[k][2][p][1])
            ctx.subpel_choose_batch([rig.chain(k, None, "field%d" % p) for k in ks], p + 1, [rig.span(k, "table%d" % p) for k in ks])
        ctx.synchronize()
        expected = {}
        for k, (c, _, passes, cols, rws) in enumerate(entries):
            for p, (_, _, behind) in enumerate(passes):
                report_blocks("chain %d, pass %d" % (k, p + 1), rig.span(k, "field%d" % p).download(), behind, c["nbx"], cols, rws)
                expected[k, "field%d" % p] = behind
        rig.check(expected)
    finally:
        rig.free()


def subpel_entry(name):
    c, src, tables, fields = L.subpel_expected(name)
    g = L.GRIDS[name]
    return c, src, [(fields[p], tables[p], fields[p + 1]) for p in range(c["prec"])], g["cols"], g["rws"]


@pytest.mark.parametrize("name", sorted(L.GRIDS))
def test_subpel_choice(ctx, name):
    """subpel_choose_batch per pass from the crafted tables: all 20 bytes of every record; the tables and the skipped
    records stay as they were."""
    subpel_choice(ctx, [subpel_entry(name)], seed_of(name))


def test_subpel_choice_mixed(ctx):
    """A crossing grid and a small named case of tests/subpel_cases.py in one call, in both orders: two chains with unlike
    numbers of diagonals."""
    small = "precision_1"
    c = KS.CASES[small]
    fields, tables = KS.fields_by_pass(small), KS.expected(small)[1]
    entry = (c, KS.inputs(small)[0], [(fields[0], tables[0], fields[1])], c["nbx"], c["nby"])
    big = subpel_entry("wave_crossed")
    subpel_choice(ctx, [(big[0], big[1], big[2][:1]) + big[3:], entry], 11)
    subpel_choice(ctx, [entry, (big[0], big[1], big[2][:1]) + big[3:]], 12)


def test_subpel_stage_from_pictures(ctx):
    """subpel_batch at 68 x 66 blocks of 4 x 4: the error launches and the choices of both passes chained on the device."""
    c, src, ref, start, field = L.subpel_stage()
    n = c["nbx"] * c["nby"] * MV
    rig = TS.Rig(ctx, [(c, src, ref)], [{"start": (n, False), "field": (n, True)}], seed=13)
    try:
        rig.put(0, "start", start)
        ctx.subpel_batch([rig.chain(0, "start", "field")])
        ctx.synchronize()
        report_blocks("the stage", rig.span(0, "field").download(), field, c["nbx"], c["nbx"], c["nby"])
        rig.check({(0, "field"): field})
    finally:
        rig.free()


# ---- split 2 ------------------------------------------------------------------------------------------------------------

def flat_pictures(c):
    flat = [np.zeros((h, w), np.uint8) for (w, h) in K2._sizes(c)]      # (the choice reads no picture: only its size)
    return flat, [flat] * c["refs"]


def split2_choice(ctx, entries, seed):
    """entries: (case, src, refs, fields, table, motion, superblocks, cols, rws), all in one call."""
    rig = T2.Rig(ctx, [e[:3] for e in entries], ("motion", "superblocks"), seed=seed)
    try:
        for n, e in enumerate(entries):
            rig.put_fields(n, e[3])
            rig.put(n, "table", e[4])
        ctx.split2_choose_batch([rig.picture(n) for n in range(len(entries))], [rig.span(n, "table") for n in range(len(entries))])
        ctx.synchronize()
        expected = {}
        for n, (c, _, _, _, _, motion, sb, cols, rws) in enumerate(entries):
            report_blocks("picture %d" % n, rig.span(n, "motion").download(), motion, c["nbx"], cols, rws)
            report_superblocks("picture %d, the sums" % n, rig.span(n, "superblocks").download(), sb, T2.SB, c["nbx"] // 4, c["nby"] // 4)
            expected[n, "motion"], expected[n, "superblocks"] = motion, sb
        rig.check(expected)
    finally:
        rig.free()


def split2_entry(name):
    c, fields, table, motion, sb = L.split2_expected(name)
    g = L.GRIDS[name]
    return (c,) + flat_pictures(c) + (fields, table, motion, sb, g["cols"], g["rws"])


@pytest.mark.parametrize("name", sorted(L.GRIDS))
def test_split2_choice(ctx, name):
    """split2_choose_batch from the crafted tables: the motion records and the superblock table -- sums that every block of
    every wave adds to atomically, and the score as bits."""
    split2_choice(ctx, [split2_entry(name)], seed_of(name, 2))


def test_split2_choice_mixed(ctx):
    small = "tiny"
    c = K2.CASES[small]
    src, refs, fields = K2.inputs(small)
    motion, sb, table, _ = K2.expected(small)
    entry = (c, src, refs, fields, table, motion, sb, c["nbx"], c["nby"])
    big = split2_entry("wave_crossed")
    split2_choice(ctx, [big, entry], 14)
    split2_choice(ctx, [entry, big], 15)


def test_split2_stage_from_pictures(ctx):
    c, src, refs, fields, motion, sb = L.split2_stage()
    rig = T2.Rig(ctx, [(c, src, refs)], ("motion", "superblocks"), seed=16)
    try:
        rig.put_fields(0, fields)
        ctx.split2_batch([rig.picture(0)])
        ctx.synchronize()
        report_blocks("the stage", rig.span(0, "motion").download(), motion, c["nbx"], -(-c["w"] // c["xb"]), -(-c["h"] // c["yb"]))
        rig.check({(0, "motion"): motion, (0, "superblocks"): sb})
    finally:
        rig.free()


# ---- the mode decision ----------------------------------------------------------------------------------------------------

def mode_entry(name):
    src, refs = L.mode_inputs(name)[:2]
    return L.MODE_CASES[name], src, refs


def mode_report(rig, n, c, out):
    sbx, sby = c["nbx"] // 4, c["nby"] // 4
    bad = differing(rig.span(n, "motion").download(), out[0], MV)
    if bad.size:
        sx, sy = min(((int(k % c["nbx"]) >> 2, int(k // c["nbx"]) >> 2) for k in bad), key=lambda b: (b[0] + b[1], b[1]))
        raise AssertionError("picture %d: %d of %d records differ, first in the walk's order %s" % (n, bad.size, out[0].size,
                                                                                                    L.describe_superblock(sbx, sby, sx, sy)))
    report_superblocks("picture %d, superblocks" % n, rig.span(n, "superblocks").download(), out[1], TM.SB, sbx, sby)
    report_superblocks("picture %d, trials" % n, rig.span(n, "trials").download(), out[2], TM.TRIALS, sbx, sby)


@pytest.mark.parametrize("name", sorted(L.MODE_CASES))
def test_mode_metric_launch(ctx, name):
    out = L.mode_expected(name)
    rig = TM.Rig(ctx, [mode_entry(name)], ("table2", "table"), seed=seed_of(name, 3))
    try:
        rig.put_fields(0, *L.mode_inputs(name)[2:])
        ctx.mode_metric_batch([rig.picture(0)], rig.tables([0]))
        ctx.synchronize()
        rig.check({(0, "table2"): out[4], (0, "table"): out[5]})
    finally:
        rig.free()


@pytest.mark.parametrize("name", sorted(L.MODE_CASES))
def test_mode_choice_launch(ctx, name):
    """From the restatement's tables: a wave's work slot serves a superblock per round, waves without one keep the barriers."""
    out = L.mode_expected(name)
    rig = TM.Rig(ctx, [mode_entry(name)], TM.OUTPUTS, seed=seed_of(name, 4))
    try:
        rig.put_fields(0, *L.mode_inputs(name)[2:])
        rig.put(0, "table2", out[4])
        rig.put(0, "table", out[5])
        ctx.mode_choose_batch([rig.picture(0)], rig.tables([0]))
        ctx.synchronize()
        mode_report(rig, 0, L.MODE_CASES[name], out)
        rig.check(TM.outputs(0, out))
    finally:
        rig.free()


def mode_stage(ctx, entries, inputs, want, seed):
    rig = TM.Rig(ctx, entries, TM.OUTPUTS, seed=seed)
    try:
        for n, ins in enumerate(inputs):
            rig.put_fields(n, *ins)
        ctx.mode_decision_batch([rig.picture(n) for n in range(len(entries))])
        ctx.synchronize()
        expected = {}
        for n, out in enumerate(want):
            mode_report(rig, n, entries[n][0], out)
            expected.update(TM.outputs(n, out))
        rig.check(expected)
    finally:
        rig.free()


@pytest.mark.parametrize("name", sorted(L.MODE_CASES))
def test_mode_stage(ctx, name):
    """mode_decision_batch: motion, superblocks, trials and the statistics."""
    mode_stage(ctx, [mode_entry(name)], [L.mode_inputs(name)[2:]], [L.mode_expected(name)], seed_of(name, 5))


def test_mode_stage_mixed(ctx):
    """A grid of two rounds and a small named case of tests/mode_cases.py in one call, in both orders."""
    small, big = "block_4x4", "round_crossed"
    a = (mode_entry(big), L.mode_inputs(big)[2:], L.mode_expected(big))
    b = (TM.case_entry(small), MC.inputs(small)[2:], MC.expected(small))
    for order, seed in (((a, b), 17), ((b, a), 18)):
        mode_stage(ctx, [e[0] for e in order], [e[1] for e in order], [e[2] for e in order], seed)
