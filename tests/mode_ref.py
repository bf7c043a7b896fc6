"""The restatement of schro_mode_decision entire (schromotionest.c:2587-2688): per superblock schro_do_split2, then
schro_do_split1 (:2008-2206, with schro_get_best_mv_split1 :1840-2005), schro_do_split0 if split 1 won (:2510-2582, with
schro_get_best_split0_mv :2208-2363 and schro_do_split0_biref :2365-2486), schro_do_split0_biref_zero with two references
(:2488-2507), schro_block_fixup (:1473-1494), schro_motion_copy_to and the three statistics (:2655-2681).  Everything
tests/split2_ref.py restates is taken from there: records as 20-byte bytearrays, UpFrame, the prediction functions, the
split-2 trial of one block and the shared fetch buffers of the bi-reference trials.

The work is cut where the device cuts it.
    metric_tables   everything that reads a picture and depends on no decision: M_INTS int32 per SUPERBLOCK, the layout of
                    include/schro_hip.h (SCHRO_HIP_MODE_TABLE_INTS).  Per reference 22 candidate vectors: slot 5 q + m of
                    quadrant q is sub-pel record m of the quadrant (m = 2 jj + ii) or, m = 4, the level-1 record with its
                    vector shifted; 20 is the level-2 record, shifted; 21 is the zero vector (what split 0 inherits from a
                    quadrant outside the picture).  A candidate carries the bound test of split 1 on its own quadrant, the
                    bound test of split 0 on the superblock, and its luma and chroma SAD over EACH of the four quadrants:
                    clipping and the bilinear form are per sample, so a split-0 SAD is the sum over the quadrants (asserted
                    in tests/test_mode_ref.py).  Then the bi-reference trial at zero vectors.
    Reads           the bi-reference metrics of split 1 and split 0 depend on the chosen pair; the walk asks `biref` for
                    them.
    choose          the walk.  order "raster" is the C text: one array of records, superblock by superblock, with every
                    write schro_do_split1 and the candidate trials make into `motion` on the way and one tryblock reused
                    over the three later trials.  order "diagonal" is the device's: anti-diagonals of superblocks, a
                    superblock working on records of its own and reading only the FINAL records of its left, upper and
                    upper-left neighbours; a read of a record of its own that it has not written is an error.

Rules beyond the issue's ten that the C text shows:
 11. A split-1 or split-0 candidate is `*mv_motion = *hint_mv[m]` with split and pred_mode set and using_global NOT
     cleared.  A hint record whose using_global bit is set therefore has entropy 0 (schro_motion_block_estimate_entropy
     :1266), is skipped by its neighbours' predictions, and carries the bit into the final field.  (The split-2 trial and
     both bi-reference trials of split 0 clear it; the bi-reference trial of split 1 keeps mv_ref[0]'s.)
 12. A superblock whose origin lies outside the picture would win at split 1 (entropy 8 against 32) and then run into
     SCHRO_ASSERT (0) of schro_get_best_split0_mv (:2260).  The reference's grids have none; a grid that has one is
     refused.
 13. schro_get_best_mv_split1 leaves *error and *entropy alone when no hint is admissible; nothing reads them then, and
     the record it leaves in split1_mf is stack junk but for metric = INT_MAX, which is all split 0 looks at."""
import struct

import numpy as np

import split2_ref as R
import subpel_ref as S

MV_DTYPE = R.MV_DTYPE
SB_DTYPE = R.SB_DTYPE
TRIAL_DTYPE = np.dtype([("state", "<i4"), ("error", "<i4"), ("entropy", "<i4"), ("pad", "<i4"), ("score", "<f8")])
INT_MAX = R.INT_MAX
_i32, _i16 = R._i32, R._i16

# the table entry of a superblock (include/schro_hip.h)
M_CANDS = 22
M_LEVEL1, M_LEVEL2, M_ZERO = 4, 20, 21
M_CAND_INTS = 12
M_OK1, M_OK0, M_QUAD = 0, 1, 2          # M_QUAD + 2 q: luma, chroma of quadrant q
M_REF_INTS = M_CANDS * M_CAND_INTS
M_ZERO_BI = 2 * M_REF_INTS              # ok, luma, chroma, 0
M_INTS = M_ZERO_BI + 4
M_NONE = -1

SPLIT1_BEST = bytes([0x09]) + bytes(19)  # best_mv = { 0 }; split = 1; pred_mode = 1


def split_of(rec):
    return (rec[0] >> 3) & 3


def set_split(rec, split):
    rec[0] = (rec[0] & ~0x18 & 0xff) | (split << 3)


def set_pred(rec, mode):
    rec[0] = (rec[0] & ~3 & 0xff) | mode


def set_metric(rec, metric, chroma=None):
    struct.pack_into("<I", rec, 4, metric & 0xffffffff)
    if chroma is not None:
        struct.pack_into("<I", rec, 8, chroma & 0xffffffff)


def block_entropy(get, x, y, mv):
    """schro_motion_block_estimate_entropy for a record that predicts from a reference and sits at its block's origin"""
    assert R.pred_mode(mv) != 0
    if (mv[0] >> 2) & 1:                                # using_global (rule 11)
        return 0
    return R.block_entropy(get, x, y, mv)


def block_size(params):
    return 16 * params["xbsep_luma"] * params["ybsep_luma"] * 2 // 3


# ---- what reads the pictures ------------------------------------------------------------------------------------------

def _bound_ok(dx, dy, w, h, sizes, prec, ext):
    xmax, ymax = (sizes[0][0] << prec) + ext, (sizes[0][1] << prec) + ext
    return not (-ext > dx or -ext > dy or not xmax > dx + w - 1 or not ymax > dy + h - 1)


def candidates(fields, level1, level2, nbx, i, j, ref, prec):
    """The 22 candidate vectors (dx[ref], dy[ref]) of reference `ref` at the superblock whose first block is (i, j)."""
    out = []
    for q in range(4):
        x, y = i + 2 * (q & 1), j + 2 * (q >> 1)
        for m in range(4):
            v = fields[ref]["v"][(y + (m >> 1)) * nbx + x + (m & 1)]
            out.append((int(v[ref]), int(v[2 + ref])))
        v = level1[ref]["v"][y * nbx + x]
        out.append((_i16(int(v[ref]) << prec), _i16(int(v[2 + ref]) << prec)))
    v = level2[ref]["v"][j * nbx + i]
    out.append((_i16(int(v[ref]) << prec), _i16(int(v[2 + ref]) << prec)))
    out.append((0, 0))
    return out


def _sad(src, ups, ref, k, x0, y0, w, h, dx, dy, prec):
    got = ups[ref][k].block(dx, dy, prec, w, h)
    return int(np.abs(src[k][y0:y0 + h, x0:x0 + w].astype(np.int32) - got).sum())


def metric_tables(src, refs, params, fields, level1, level2, extension, stats=None):
    """The (superblocks, M_INTS) int32 table."""
    height, width = src[0].shape
    nbx, nby, blocks, sizes = R.geometry(params, width, height)
    prec, num_refs = params["mv_precision"], len(refs)
    dims = (params["h_shift"], params["v_shift"])
    st = stats if stats is not None else {}
    ups = [[R.UpFrame(r[k], extension, st) for k in range(3)] for r in refs]
    sbx = nbx // 4
    table = np.full((sbx * (nby // 4), M_INTS), M_NONE, np.int32)
    for j in range(0, nby, 4):
        for i in range(0, nbx, 4):
            t = table[(j // 4) * sbx + i // 4]
            assert i * blocks[0][0] < width and j * blocks[0][1] < height          # rule 12
            w4, h4 = min(4 * blocks[0][0], width - i * blocks[0][0]), min(4 * blocks[0][1], height - j * blocks[0][1])
            for ref in range(num_refs):
                for c, (vx, vy) in enumerate(candidates(fields, level1, level2, nbx, i, j, ref, prec)):
                    e = t[ref * M_REF_INTS + c * M_CAND_INTS:][:M_CAND_INTS]
                    e[10], e[11] = 0, 0
                    ok0 = _bound_ok(vx + ((i * blocks[0][0]) << prec), vy + ((j * blocks[0][1]) << prec), w4, h4, sizes, prec, extension)
                    e[M_OK0] = int(ok0)
                    for q in range(4):
                        x, y = i + 2 * (q & 1), j + 2 * (q >> 1)
                        x0, y0 = x * blocks[0][0], y * blocks[0][1]
                        if x0 >= width or y0 >= height:
                            continue                    # a quadrant outside the picture: M_NONE
                        own = c < 20 and c // 5 == q
                        ok1 = False
                        if own:
                            w2, h2 = min(2 * blocks[0][0], width - x0), min(2 * blocks[0][1], height - y0)
                            ok1 = _bound_ok(vx + (x0 << prec), vy + (y0 << prec), w2, h2, sizes, prec, extension)
                            e[M_OK1] = int(ok1)
                        if not (ok0 or ok1):
                            continue                    # nothing the walk may read: M_NONE
                        total = [0, 0]
                        for k in range(3):
                            cx0, cy0 = x * blocks[k][0], y * blocks[k][1]
                            assert cx0 < sizes[k][0] and cy0 < sizes[k][1]
                            w, h = min(2 * blocks[k][0], sizes[k][0] - cx0), min(2 * blocks[k][1], sizes[k][1] - cy0)
                            dx = (vx >> (dims[0] if k else 0)) + (cx0 << prec)
                            dy = (vy >> (dims[1] if k else 0)) + (cy0 << prec)
                            total[k > 0] += _sad(src, ups, ref, k, cx0, cy0, w, h, dx, dy, prec)
                        e[M_QUAD + 2 * q], e[M_QUAD + 2 * q + 1] = total
            if num_refs > 1:
                ok, luma, chroma = biref_metric(src, ups, params, extension, 0, i, j, (0, 0), (0, 0), st)
                t[M_ZERO_BI:] = (int(ok), luma, chroma, 0)
    return table


def biref_metric(src, ups, params, extension, split, x, y, v0, v1, st=None):
    """The bi-reference trial of split `split` (2, 1, 0) whose block begins at block (x, y): (admissible, luma, chroma),
    with the shared fetch buffers of precision 2 and 3 (tests/split2_ref.py)."""
    height, width = src[0].shape
    _, _, blocks, sizes = R.geometry(params, width, height)
    scale = 4 >> split
    assert x % scale == 0 and y % scale == 0
    big = tuple((bw * scale, bh * scale) for bw, bh in blocks)
    ok, luma, chroma, _, _ = R._biref(src, ups, (params["h_shift"], params["v_shift"]), big, sizes, params["mv_precision"], extension, x // scale,
                                      y // scale, v0, v1, st if st is not None else {})
    return ok, luma, chroma


def picture_reader(src, refs, params, extension, stats=None):
    """The `biref` a walk over real pictures asks: (split, x, y, v0, v1) -> (admissible, luma, chroma)."""
    st = stats if stats is not None else {}
    ups = [[R.UpFrame(r[k], extension, st) for k in range(3)] for r in refs]
    return lambda split, x, y, v0, v1: biref_metric(src, ups, params, extension, split, x, y, v0, v1, st)


# ---- the walk -----------------------------------------------------------------------------------------------------------

def _score(entropy, lam, error, fused=False):
    return R._score(entropy, lam, error, fused)


class _Block:
    """SchroBlock: valid, error, entropy, score, mv[4][4]"""

    def __init__(self):
        self.valid, self.error, self.entropy, self.score = False, 0, 0, 0.0
        self.mv = [[bytearray(20) for _ in range(4)] for _ in range(4)]

    def copy(self):
        b = _Block()
        b.valid, b.error, b.entropy, b.score = self.valid, self.error, self.entropy, self.score
        b.mv = [[bytearray(r) for r in row] for row in self.mv]
        return b

    def fixup(self):
        """schro_block_fixup"""
        m = self.mv
        if split_of(m[0][0]) == 0:
            for jj in range(4):
                for ii in range(4):
                    m[jj][ii] = bytearray(m[0][0])
        elif split_of(m[0][0]) == 1:
            for jj in (0, 2):
                for ii in (0, 2):
                    m[jj][ii + 1] = bytearray(m[jj][ii])
                    m[jj + 1][ii] = bytearray(m[jj][ii])
                    m[jj + 1][ii + 1] = bytearray(m[jj][ii])


class _Walk:
    def __init__(self, table2, table, params, width, height, lam, fields, level1, level2, biref, fused, stop_at_invalid, st):
        self.t2, self.t, self.P, self.w, self.h, self.lam = table2, table, params, width, height, lam
        self.fields, self.l1, self.l2, self.biref, self.fused, self.stop, self.st = fields, level1, level2, biref, fused, stop_at_invalid, st
        self.nbx, self.nby, self.blocks, self.sizes = R.geometry(params, width, height)
        self.prec, self.num_refs = params["mv_precision"], len(fields)
        self.ext = None

    def inside(self, x, y):
        return x * self.blocks[0][0] < self.w and y * self.blocks[0][1] < self.h

    def entry(self, i, j, ref, c):
        return self.t[(j // 4) * (self.nbx // 4) + i // 4][ref * M_REF_INTS + c * M_CAND_INTS:][:M_CAND_INTS]

    # -- schro_do_split2
    def split2(self, get, put, i, j):
        block = _Block()
        error = entropy = 0
        for jj in range(4):
            for ii in range(4):
                x, y = i + ii, j + jj
                n = y * self.nbx + x
                work, final, e, h = R.choose_block(get, x, y, self.inside(x, y), self.num_refs, self.lam, self.fields, self.t2[n], n, self.fused,
                                                   self.st["split2_level"])
                put(x, y, work)
                block.mv[jj][ii] = final
                error, entropy = _i32(error + e), _i32(entropy + h)
        block.valid, block.error, block.entropy = True, error, entropy
        block.score = _score(entropy, self.lam, error, self.fused)
        return block

    def _hints(self, ref, records, shift, extra, extra_slot):
        """The hint list: (slot, record) of `records` whose metric is not INT_MAX and whose SHIFTED vector is not in the
        list (mv_already_in_list, :1821-1835), then the block matching's record `extra` with its vector shifted by the precision."""
        hints = []

        def listed(mv, by):
            return any((R.vec(mv, ref) << by) == R.vec(h, ref) and (R.vec(mv, 2 + ref) << by) == R.vec(h, 2 + ref) for _, h in hints)
        for slot, mv in records:
            if R.metric(mv) != INT_MAX:
                # (these records are in sub-pel units already: the right shift would be 0, rule 2)
                self.st["dropped_by_the_shift"] += int(bool(hints) and listed(mv, shift) and not listed(mv, 0))
                self.st["kept_by_the_shift"] += int(bool(hints) and not listed(mv, shift) and listed(mv, 0))
                if not hints or not listed(mv, shift):
                    hints.append((slot, mv))
                else:
                    self.st["dropped"].append((ref, slot, shift))
            else:
                self.st["hint_int_max"] += 1
        if R.metric(extra) != INT_MAX:
            if not hints or not listed(extra, self.prec):
                temp = bytearray(extra)
                R.set_vec(temp, ref, R.vec(extra, ref) << self.prec)
                R.set_vec(temp, 2 + ref, R.vec(extra, 2 + ref) << self.prec)
                hints.append((extra_slot, temp))
            else:
                self.st["dropped"].append((ref, extra_slot, self.prec))
        else:
            self.st["hint_int_max"] += 1
        return hints

    # -- schro_get_best_mv_split1: (mv_ref or None, error, entropy)
    def best_split1(self, get, put, i, j, q, ref):
        x, y = i + 2 * (q & 1), j + 2 * (q >> 1)
        records = [(5 * q + m, bytearray(self.fields[ref][(y + (m >> 1)) * self.nbx + x + (m & 1)].tobytes())) for m in range(4)]
        hints = self._hints(ref, records, self.prec, bytearray(self.l1[ref][y * self.nbx + x].tobytes()), 5 * q + M_LEVEL1)
        min_score, best = float("inf"), None
        for slot, hint in hints:
            e = self.entry(i, j, ref, slot)
            cand = candidates(self.fields, self.l1, self.l2, self.nbx, i, j, ref, self.prec)[slot]
            assert cand == (R.vec(hint, ref), R.vec(hint, 2 + ref))
            assert e[M_OK1] in (0, 1)
            if not e[M_OK1]:
                self.st["out_of_bounds"] += 1
                continue
            luma, chroma = int(e[M_QUAD + 2 * q]), int(e[M_QUAD + 2 * q + 1])
            assert luma >= 0 and chroma >= 0
            mv = bytearray(hint)
            set_split(mv, 1)
            set_pred(mv, ref + 1)
            put(x, y, mv)
            ent = block_entropy(get, x, y, mv)
            self.st["global_hint"] += (mv[0] >> 2) & 1
            score = _score(ent, self.lam, luma + chroma, self.fused)
            if min_score > score:
                min_score, best = score, (hint, ent, luma, chroma, slot)
        if best is None:
            return None, None, None, None
        hint, ent, luma, chroma, slot = best
        mv = bytearray(hint)
        set_metric(mv, luma >> 2, chroma >> 2)
        set_split(mv, 1)
        set_pred(mv, ref + 1)
        return mv, luma + chroma, ent, slot

    # -- schro_do_split1: (tryblock, split1_mf of the superblock: per reference and quadrant (record or None, slot))
    def split1(self, get, put, i, j, tryblock):
        block, lam = tryblock, self.lam
        block.valid = True
        total_entropy = total_error = 0
        mf = [[None] * 4 for _ in range(2)]
        singles = 0
        for q in range(4):
            ii, jj = 2 * (q & 1), 2 * (q >> 1)
            x, y = i + ii, j + jj

            def spread():                               # set_split1_motion
                for dx, dy in ((1, 0), (0, 1), (1, 1)):
                    put(x + dx, y + dy, bytearray(get(x, y)))
            if not self.inside(x, y):
                mv = bytearray(SPLIT1_BEST)
                mode = R.mode_prediction(get, x, y)
                if mode != 1 and mode != 2:
                    mode = 1
                set_pred(mv, mode)
                px, py = R.vector_prediction(get, x, y, 1)
                R.set_vec(mv, mode - 1, px)
                R.set_vec(mv, 2 + mode - 1, py)
                put(x, y, mv)
                block.mv[jj][ii] = bytearray(mv)
                spread()
                total_entropy = _i32(total_entropy + 2)
                mf[0][q] = (bytearray(SPLIT1_BEST), M_ZERO)
                second = bytearray(SPLIT1_BEST)
                set_pred(second, 2)
                mf[1][q] = (second, M_ZERO)
                self.st["outside_quadrant_mode"][mode] += 1
                continue
            mv = bytearray(get(x, y))
            set_metric(mv, INT_MAX, INT_MAX)
            put(x, y, mv)
            min_score = float("inf")
            best_entropy = best_chroma_error = best_error = INT_MAX
            best_mv = None                              # metric INT_MAX
            mv_ref, entropy, error = [None, None], [None, None], None
            for ref in range(self.num_refs):
                got, err, ent, slot = self.best_split1(get, put, i, j, q, ref)
                mv_ref[ref] = got
                mf[ref][q] = (bytearray(got) if got is not None else None, slot)        # *mv_split1 = mv_ref[ref], a copy
                if got is not None:
                    error, entropy[ref] = err, ent
                    score = _score(ent, lam, error, self.fused)
                    if min_score > score:
                        min_score, best_mv, best_entropy, best_error = score, bytearray(got), ent, error
            won_by_bi = False
            if self.num_refs > 1 and mv_ref[0] is not None and mv_ref[1] is not None:
                both = mv_ref[0]                        # (the C text changes mv_ref[0] in place; split1_mf holds its copy)
                R.set_vec(both, 1, R.vec(mv_ref[1], 1))
                R.set_vec(both, 3, R.vec(mv_ref[1], 3))
                set_pred(both, 3)
                ok, luma, chroma = self.biref(1, x, y, (R.vec(both, 0), R.vec(both, 2)), (R.vec(both, 1), R.vec(both, 3)))
                self.st["split1_bi"][int(ok)] += 1
                if ok:
                    score = _score(entropy[0] + entropy[1], lam, luma + chroma, self.fused)
                    set_metric(both, luma >> 2, chroma >> 2)
                    if min_score > score:
                        best_error, best_chroma_error, best_entropy, best_mv, min_score = luma, chroma, entropy[0] + entropy[1], bytearray(both), score
                        won_by_bi = True
            if best_mv is None:
                block.valid = False
                self.st["invalid_quadrant"][q] += 1
                if self.stop:
                    break
            else:
                singles += int(not won_by_bi)
                put(x, y, bytearray(best_mv))
                total_error = _i32(total_error + _i32(best_error + best_chroma_error))      # rule 1: INT_MAX unless the pair won
                total_entropy = _i32(total_entropy + best_entropy)
                block.mv[jj][ii] = bytearray(best_mv)
                spread()
        block.error, block.entropy = total_error, total_entropy
        block.score = _score(total_entropy, lam, total_error, self.fused)
        if block.valid:
            self.st["singles"][singles] += 1
        return mf, singles

    # -- schro_get_best_split0_mv
    def best_split0(self, get, put, i, j, ref, mf):
        records = [(slot, rec) for rec, slot in mf[ref] if rec is not None]     # (a junk record has metric INT_MAX: skipped)
        hints = self._hints(ref, records, 0, bytearray(self.l2[ref][j * self.nbx + i].tobytes()), M_LEVEL2)
        min_score, best = float("inf"), None
        for slot, hint in hints:
            e = self.entry(i, j, ref, slot)
            cand = candidates(self.fields, self.l1, self.l2, self.nbx, i, j, ref, self.prec)[slot]
            assert cand == (R.vec(hint, ref), R.vec(hint, 2 + ref)), (slot, cand)
            if not e[M_OK0]:
                self.st["out_of_bounds0"] += 1
                continue
            quads = [(int(e[M_QUAD + 2 * q]), int(e[M_QUAD + 2 * q + 1])) for q in range(4) if e[M_QUAD + 2 * q] != M_NONE]
            luma, chroma = sum(a for a, _ in quads), sum(b for _, b in quads)
            mv = bytearray(hint)
            set_split(mv, 0)
            set_pred(mv, ref + 1)
            put(i, j, mv)
            ent = block_entropy(get, i, j, mv)
            score = _score(ent, self.lam, luma + chroma, self.fused)
            if min_score > score:
                min_score, best = score, (hint, ent, luma, chroma)
        if best is None:
            return None, None, None
        hint, ent, luma, chroma = best
        mv = bytearray(hint)
        set_metric(mv, luma >> 4, chroma >> 4)
        set_split(mv, 0)
        set_pred(mv, ref + 1)
        return mv, luma + chroma, ent

    # -- schro_do_split0_biref on block->mv[0][0] with its flags already set
    def split0_biref(self, get, put, i, j, block):
        block.valid = False
        mv = block.mv[0][0]
        put(i, j, bytearray(mv))
        entropy = block_entropy(get, i, j, mv)
        v0, v1 = (R.vec(mv, 0), R.vec(mv, 2)), (R.vec(mv, 1), R.vec(mv, 3))
        if v0 == (0, 0) == v1:
            t = self.t[(j // 4) * (self.nbx // 4) + i // 4]
            ok, luma, chroma = int(t[M_ZERO_BI]), int(t[M_ZERO_BI + 1]), int(t[M_ZERO_BI + 2])
            assert ok in (0, 1)
        else:
            ok, luma, chroma = self.biref(0, i, j, v0, v1)
        if ok:
            set_metric(mv, luma >> 4, chroma >> 4)
            block.entropy, block.error = entropy, luma + chroma
            block.score = _score(block.entropy, self.lam, block.error, self.fused)
            block.valid = True

    # -- schro_do_split0
    def split0(self, get, put, i, j, tryblock, mf):
        block, lam = tryblock, self.lam
        block.valid = False
        min_score, best_mv, best_error, best_entropy = float("inf"), None, INT_MAX, INT_MAX
        mv_ref, entropy = [None, None], [None, None]
        for ref in range(self.num_refs):
            got, err, ent = self.best_split0(get, put, i, j, ref, mf)
            mv_ref[ref] = got
            if got is not None:
                entropy[ref] = ent
                score = _score(ent, lam, err, self.fused)
                if min_score > score:
                    min_score, best_mv, best_entropy, best_error = score, bytearray(got), ent, err
        if self.num_refs > 1 and mv_ref[0] is not None and mv_ref[1] is not None:
            bi = _Block()
            mv = bi.mv[0][0]
            mv[0] = 3                                   # split 0, pred_mode 3, using_global 0
            for k, v in enumerate((R.vec(mv_ref[0], 0), R.vec(mv_ref[1], 1), R.vec(mv_ref[0], 2), R.vec(mv_ref[1], 3))):
                R.set_vec(mv, k, v)
            set_metric(mv, INT_MAX)
            self.split0_biref(get, put, i, j, bi)
            self.st["split0_bi"][int(bi.valid)] += 1
            if bi.valid and min_score > bi.score:
                min_score, best_mv, best_error, best_entropy = bi.score, bytearray(bi.mv[0][0]), bi.error, bi.entropy
        if best_mv is not None:
            block.valid, block.error, block.entropy = True, best_error, best_entropy
            block.score = _score(best_entropy, lam, best_error, self.fused)
            block.mv[0][0] = best_mv

    # -- the body of schro_mode_decision's loops: (block, trials)
    def superblock(self, get, put, i, j):
        st = self.st
        trials = np.zeros(4, TRIAL_DTYPE)
        trials["state"] = -1

        def note(k, b):
            trials[k] = (1, b.error, b.entropy, 0, b.score) if b.valid else (0, 0, 0, 0, 0.0)
        block = self.split2(get, put, i, j)
        note(0, block)
        min_score = block.score
        tryblock = _Block()
        mf, singles = self.split1(get, put, i, j, tryblock)
        note(1, tryblock)
        if tryblock.valid and min_score > tryblock.score:
            block = tryblock.copy()
            block.fixup()
            for jj in range(4):                         # schro_motion_copy_to
                for ii in range(4):
                    put(i + ii, j + jj, bytearray(block.mv[jj][ii]))
            min_score = block.score
            self.split0(get, put, i, j, tryblock, mf)
            note(2, tryblock)
            if tryblock.valid and min_score > tryblock.score:
                st["split0_beats_split1"] += 1
                block = tryblock.copy()
                block.fixup()                           # (min_score stays split 1's: rule 7)
        elif tryblock.valid:
            st["honest_loss"][singles] += 1
        if self.num_refs > 1:
            was_split0 = split_of(block.mv[0][0]) == 0
            before = block.score
            tryblock.mv[0][0][0] = (tryblock.mv[0][0][0] & 0xe0) | 3        # split 0, pred_mode 3, using_global 0
            for k in range(4):
                R.set_vec(tryblock.mv[0][0], k, 0)
            self.split0_biref(get, put, i, j, tryblock)
            note(3, tryblock)
            if tryblock.valid and min_score > tryblock.score:
                st["rule7"] += int(was_split0 and before < tryblock.score)
                st["zero_wins"] += 1
                block = tryblock.copy()
                block.fixup()
        st["final_split"][split_of(block.mv[0][0])] += 1
        return block, trials


def new_stats(stats=None):
    st = stats if stats is not None else {}
    st.setdefault("split2_level", R.new_stats())
    for key in ("out_of_bounds", "out_of_bounds0", "hint_int_max", "global_hint", "split0_beats_split1", "rule7", "zero_wins", "dropped_by_the_shift",
                "kept_by_the_shift"):
        st.setdefault(key, 0)
    st.setdefault("dropped", [])
    st.setdefault("singles", [0] * 5)           # valid split-1 trials by their number of single-reference quadrants (rule 1)
    st.setdefault("honest_loss", [0] * 5)       # ... that lost to split 2
    st.setdefault("invalid_quadrant", [0] * 4)
    st.setdefault("outside_quadrant_mode", [0] * 3)
    st.setdefault("split1_bi", [0, 0])
    st.setdefault("split0_bi", [0, 0])
    st.setdefault("final_split", [0] * 3)
    return st


def statistics(sb, dc_blocks, params):
    """(mc_error, badblock_ratio, dcblock_ratio), :2655-2681, from the winners' errors in raster order."""
    size = block_size(params)
    nbx, nby = params["x_num_blocks"], params["y_num_blocks"]
    total, bad = 0.0, 0
    for e in sb["error"]:
        e = int(e)
        bad += int(e > 10 * size)
        total += float(e) * e / float(size * size)
    return np.array([total / (240.0 * 240.0) / nbx * nby / 16, float(bad) / (nbx * nby // 16), float(dc_blocks) / (nbx * nby)], np.float64)


def choose(table2, table, params, width, height, lam, fields, level1, level2, biref, order="raster", fused=False, stop_at_invalid=False, stats=None):
    """(motion as MV_DTYPE, superblocks as SB_DTYPE, trials as (superblocks, 4) TRIAL_DTYPE, the three statistics)."""
    st = new_stats(stats)
    w = _Walk(table2, table, params, width, height, lam, fields, level1, level2, biref, fused, stop_at_invalid, st)
    nbx, nby = w.nbx, w.nby
    assert nbx % 4 == 0 and nby % 4 == 0
    sbx, sby = nbx // 4, nby // 4
    motion = [None] * (nbx * nby)
    sb = np.zeros(sbx * sby, SB_DTYPE)
    trials = np.zeros((sbx * sby, 4), TRIAL_DTYPE)
    dc_blocks = 0

    def finish(i, j, block, tr):
        nonlocal dc_blocks
        for jj in range(4):
            for ii in range(4):
                motion[(j + jj) * nbx + i + ii] = bytearray(block.mv[jj][ii])
                dc_blocks += int(R.pred_mode(block.mv[jj][ii]) == 0)
        n = (j // 4) * sbx + i // 4
        sb[n] = (block.error, block.entropy, block.score)
        trials[n] = tr
    if order == "raster":
        def get(x, y):
            assert motion[y * nbx + x] is not None
            return motion[y * nbx + x]

        def put(x, y, rec):
            motion[y * nbx + x] = rec
        for j in range(0, nby, 4):
            for i in range(0, nbx, 4):
                finish(i, j, *w.superblock(get, put, i, j))
    else:
        assert order == "diagonal"
        for d in range(sbx + sby - 1):
            done = []
            for sy in range(max(0, d - (sbx - 1)), min(d, sby - 1) + 1):
                sx = d - sy
                own = {}

                def get(x, y, sx=sx, sy=sy, own=own):
                    if (x >> 2, y >> 2) == (sx, sy):
                        return own[x, y]                # (a KeyError: a record of its own read before it was written)
                    assert (x >> 2, y >> 2) in ((sx - 1, sy), (sx, sy - 1), (sx - 1, sy - 1)) and motion[y * nbx + x] is not None
                    return motion[y * nbx + x]

                def put(x, y, rec, sx=sx, sy=sy, own=own):
                    assert (x >> 2, y >> 2) == (sx, sy)
                    own[x, y] = rec
                done.append((4 * sx, 4 * sy) + w.superblock(get, put, 4 * sx, 4 * sy))
            for item in done:                           # (a diagonal's superblocks do not see one another)
                finish(*item)
    out = np.frombuffer(b"".join(bytes(r) for r in motion), MV_DTYPE).copy()
    return out, sb, trials, statistics(sb, dc_blocks, params)


def mode_decision(src, refs, params, lam, fields, level1, level2, extension, order="raster", fused=False, stop_at_invalid=False, stats=None):
    """(motion, superblocks, trials, statistics, the split-2 table, the mode table)"""
    st = new_stats(stats)
    table2 = R.metric_tables(src, refs, params, fields, extension, st["split2_level"])
    table = metric_tables(src, refs, params, fields, level1, level2, extension, st)
    reader = picture_reader(src, refs, params, extension, st)
    out = choose(table2, table, params, src[0].shape[1], src[0].shape[0], lam, fields, level1, level2, reader, order, fused, stop_at_invalid, st)
    return out + (table2, table)
