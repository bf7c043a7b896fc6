"""The restatement of the split-2 level of schro_mode_decision (schromotionest.c:2587-2688): for every superblock in
raster order schro_do_split2 (:1600-1807) and then schro_motion_copy_to (:1511-1522), nothing else -- with
schro_get_split2_metric (:1527-1594), schro_block_average (:481-516), schro_metric_get_biref (schrometric.c:273-304),
schro_motion_block_estimate_entropy (:1243-1281), schro_motion_vector_prediction and schro_motion_get_mode_prediction
(schromotion.c:315-430), over numpy planes.

A record is the 20 bytes of a SchroMotionVector (schromotion.h:20-37), kept as a bytearray: a DC record is built IN
PLACE over a motion record, and what it leaves of it is compared.  Byte 0 holds pred_mode (bits 0-1), using_global (bit
2), split (bits 3-4) and three unused bits; bytes 1-3 (scan, padding) travel with every struct copy.

The reads are RAW reads of the upsampled references with real `extension`-wide aprons (subpel_ref.UpFrame, one per
component); every read asserts that it stays inside them.

The work is cut where the device cuts it.  `metric_tables` is everything that reads a picture: T_INTS int32 per block,
the layout of include/schro_hip.h.  `choose` is the walk over the blocks, from the tables and the sub-pel fields alone:
    order "raster"     superblock by superblock over ONE array of records, as the C text has it;
    order "diagonal"   anti-diagonals of blocks over TWO arrays -- the working form a neighbour in the same superblock
                       sees and the final form everyone else sees (an outside block differs between the two).
The fetch buffers of precision 2 and 3: schro_mode_decision allocates ONE buffer per reference (fd[ref], :2600-2609) and
schro_do_split2's bi-reference trial fetches all three components into it before it measures any (:1698-1747).  At
mv_precision > 1 the luma metric therefore sees V's prediction in its top-left width[2] x height[2] samples and U is
measured against V's prediction.  `_biref` keeps the buffers and so restates that; precision 0 and 1 point into the
frames and are not touched by it."""
import struct
from fractions import Fraction

import numpy as np

import oracle_lib as O
import subpel_ref as S

MV_DTYPE = O.MV_DTYPE
SB_DTYPE = np.dtype([("error", "<i4"), ("entropy", "<i4"), ("score", "<f8")])
INT_MAX = 0x7fffffff

# the table entry of a block (include/schro_hip.h)
T_INTS = 16
T_CHROMA = 0            # [ref]: the chroma SAD of schro_get_split2_metric; T_NONE: no source block, or no such reference
T_BI_OK, T_BI_LUMA, T_BI_CHROMA = 2, 3, 4
T_DC = 5                # [k]: dc[k]
T_DC_ERROR = 8          # the summed DC error; T_NONE: SCHRO_METRIC_INVALID_2
T_AREA = 9              # width[0] * height[0] + 2 * width[1] * height[1] as the bi-reference branch leaves them
T_NONE = -1

BEST_MV = bytes([0x11]) + bytes(19)     # best_mv = { 0 }; split = 2; pred_mode = 1


def _i32(v):
    return ((int(v) + 0x80000000) & 0xffffffff) - 0x80000000


def _i16(v):
    return ((int(v) + 0x8000) & 0xffff) - 0x8000


def pred_mode(rec):
    return rec[0] & 3


def set_mode(rec, mode):
    """mv->split = 2; mv->pred_mode = mode; mv->using_global = 0"""
    rec[0] = (rec[0] & 0xe0) | (2 << 3) | mode


def vec(rec, k):
    """k: 0 dx[0], 1 dx[1], 2 dy[0], 3 dy[1] -- or dc[k]"""
    return struct.unpack_from("<h", rec, 12 + 2 * k)[0]


def set_vec(rec, k, v):
    struct.pack_into("<h", rec, 12 + 2 * k, _i16(v))


def metric(rec):
    return struct.unpack_from("<I", rec, 4)[0]


def geometry(params, width, height):
    """(nbx, nby, the block of each component, the size of each component)."""
    hs, vs = params["h_shift"], params["v_shift"]
    xb, yb = params["xbsep_luma"], params["ybsep_luma"]
    cw, ch = (width + (1 << hs) - 1) >> hs, (height + (1 << vs) - 1) >> vs
    return (params["x_num_blocks"], params["y_num_blocks"], ((xb, yb), (xb >> hs, yb >> vs), (xb >> hs, yb >> vs)),
            ((width, height), (cw, ch), (cw, ch)))


# ---- what reads the pictures ------------------------------------------------------------------------------------------

class UpFrame(S.UpFrame):
    def block(self, x, y, prec, bw, bh):
        if prec == 0:                                   # schro_upsampled_frame_get_subdata_prec0: plane 0 at (x, y)
            return self.raw(2 * x, 2 * y, bw, bh)
        return S.UpFrame.block(self, x, y, prec, bw, bh)


def block_average(comp, x, y, w, h):
    """schro_block_average: (dc, error), or None for SCHRO_METRIC_INVALID_2."""
    ch, cw = comp.shape
    xmax, ymax = min(x + w, cw), min(y + h, ch)
    if x >= cw or y >= ch:
        return None
    n = total = 0
    for j in range(y, ymax):
        for i in range(x, xmax):
            total += int(comp[j, i])
        n += xmax - x
    if n == 0:
        return None
    ave = (total + n // 2) // n
    total = 0
    for j in range(y, ymax):
        for i in range(x, xmax):
            total += abs(ave - int(comp[j, i]))
    return ave - 128, total


def metric_biref(orig, a, b):
    """schro_metric_get_biref (.., weight 1, .., weight 1, shift 1, ..)"""
    return int(np.abs(orig - ((a + b + 1) >> 1)).sum())


def _biref(src, ups, dims, blocks, sizes, prec, ext, i, j, v0, v1, st):
    """The bi-reference branch of schro_do_split2 up to its metrics: (admissible, luma, chroma, width, height)."""
    xmin = ymin = -ext
    xmax, ymax = (sizes[0][0] << prec) + ext, (sizes[0][1] << prec) + ext
    buf = [np.zeros((4 * blocks[0][1], 4 * blocks[0][0]), np.int32) for _ in range(2)] if prec > 1 else None      # fd[ref].data
    width, height, ref_data, orig = [0] * 3, [0] * 3, [[None, None] for _ in range(3)], [None] * 3
    biref = True
    for k in range(3):
        cw, ch = blocks[k]
        x0, y0 = i * cw, j * ch
        width[k], height[k] = min(cw, sizes[k][0] - x0), min(ch, sizes[k][1] - y0)
        orig[k] = src[k][y0:y0 + height[k], x0:x0 + width[k]].astype(np.int32)
        tmp_x, tmp_y = i * (cw << prec), j * (ch << prec)
        for ref, (vx, vy) in enumerate((v0, v1)):
            dx = (vx >> (dims[0] if k else 0)) + tmp_x
            dy = (vy >> (dims[1] if k else 0)) + tmp_y
            if k == 0 and biref and (xmin > dx or ymin > dy or not xmax > dx + width[k] - 1 or not ymax > dy + height[k] - 1):
                biref = False
                break
            if not biref:                               # (the C text fetches on; nothing reads what it fetched)
                continue
            got = ups[ref][k].block(dx, dy, prec, width[k], height[k])
            if prec > 1:
                buf[ref][:height[k], :width[k]] = got
                ref_data[k][ref] = None                 # fd[ref] with this width and height: read when it is measured
            else:
                ref_data[k][ref] = got
    if not biref:
        return False, 0, 0, width, height

    def data(k, ref):
        return buf[ref][:height[k], :width[k]] if prec > 1 else ref_data[k][ref]
    luma = metric_biref(orig[0], data(0, 0), data(0, 1))
    st["shared_buffer"] = st.get("shared_buffer", 0) + int(prec > 1)
    chroma = sum(metric_biref(orig[k], data(k, 0), data(k, 1)) for k in (1, 2))
    return True, luma, chroma, width, height


def metric_tables(src, refs, params, fields, extension, stats=None):
    """The (records, T_INTS) int32 table.  src: [Y, U, V]; refs: num_refs x [Y, U, V]; fields: one MV_DTYPE sub-pel field
    per reference."""
    height, width = src[0].shape
    nbx, nby, blocks, sizes = geometry(params, width, height)
    prec, num_refs = params["mv_precision"], len(refs)
    dims = (params["h_shift"], params["v_shift"])
    for k in range(3):
        assert src[k].shape == sizes[k][::-1]
    st = stats if stats is not None else {}
    ups = [[UpFrame(r[k], extension, st) for k in range(3)] for r in refs]
    table = np.zeros((nbx * nby, T_INTS), np.int32)
    for j in range(nby):
        for i in range(nbx):
            n = j * nbx + i
            t = table[n]
            t[T_CHROMA], t[T_CHROMA + 1], t[T_DC_ERROR] = T_NONE, T_NONE, T_NONE
            if i * blocks[0][0] >= width or j * blocks[0][1] >= height:
                continue
            # schro_get_split2_metric, its chroma loop
            for ref in range(num_refs):
                v = fields[ref]["v"][n]
                total = 0
                for k in (1, 2):
                    cw, ch = blocks[k]
                    x0, y0 = i * cw, j * ch
                    assert x0 < sizes[k][0] and y0 < sizes[k][1]
                    w, h = min(cw, sizes[k][0] - x0), min(ch, sizes[k][1] - y0)
                    dx = (int(v[ref]) >> dims[0]) + ((i * cw) << prec)
                    dy = (int(v[2 + ref]) >> dims[1]) + ((j * ch) << prec)
                    got = ups[ref][k].block(dx, dy, prec, w, h)
                    total += int(np.abs(src[k][y0:y0 + h, x0:x0 + w].astype(np.int32) - got).sum())
                t[T_CHROMA + ref] = total
            if num_refs > 1:
                v0 = (int(fields[0]["v"][n][0]), int(fields[0]["v"][n][2]))
                v1 = (int(fields[1]["v"][n][1]), int(fields[1]["v"][n][3]))
                ok, luma, chroma, bw, bh = _biref(src, ups, dims, blocks, sizes, prec, extension, i, j, v0, v1, st)
                t[T_BI_OK], t[T_BI_LUMA], t[T_BI_CHROMA] = int(ok), luma, chroma
                t[T_AREA] = bw[0] * bh[0] + 2 * bw[1] * bh[1]
                st["bi_inadmissible"] = st.get("bi_inadmissible", 0) + int(not ok)
            error, ok = 0, True
            for k in range(3):
                got = block_average(src[k], i * blocks[k][0], j * blocks[k][1], blocks[k][0], blocks[k][1])
                if got is None:
                    ok = False
                else:
                    t[T_DC + k] = got[0]
                    error += got[1]
            if ok:
                t[T_DC_ERROR] = error
    return table


# ---- the walk -----------------------------------------------------------------------------------------------------------

def _median3(a, b, c):
    return sorted((a, b, c))[1]


def vector_prediction(get, x, y, mode):
    """schro_motion_vector_prediction"""
    vx, vy = [], []
    for cond, nx, ny in ((x > 0, x - 1, y), (y > 0, x, y - 1), (x > 0 and y > 0, x - 1, y - 1)):
        if cond:
            mv = get(nx, ny)
            if not (mv[0] >> 2) & 1 and pred_mode(mv) & mode:
                vx.append(vec(mv, mode - 1))
                vy.append(vec(mv, 2 + mode - 1))
    n = len(vx)
    if n == 0:
        return 0, 0
    if n == 1:
        return vx[0], vy[0]
    if n == 2:
        return (vx[0] + vx[1] + 1) >> 1, (vy[0] + vy[1] + 1) >> 1
    return _median3(*vx), _median3(*vy)


def mode_prediction(get, x, y):
    """schro_motion_get_mode_prediction"""
    if y == 0:
        return 0 if x == 0 else pred_mode(get(x - 1, 0))
    if x == 0:
        return pred_mode(get(0, y - 1))
    a, b, c = pred_mode(get(x - 1, y)), pred_mode(get(x, y - 1)), pred_mode(get(x - 1, y - 1))
    return (a & b) | (b & c) | (c & a)


def block_entropy(get, x, y, mv):
    """schro_motion_block_estimate_entropy for a split-2 record that predicts from a reference"""
    entropy = 0
    for mode in (1, 2):
        if pred_mode(mv) & mode:
            px, py = vector_prediction(get, x, y, mode)
            entropy += S.estimate_sint(vec(mv, mode - 1) - px) + S.estimate_sint(vec(mv, 2 + mode - 1) - py)
    return entropy


def _score(entropy, lam, error, fused):
    if fused:
        return float(Fraction(lam) * int(error) + entropy)
    return entropy + float(error) * lam                 # a rounded product, then a rounded sum


def choose_block(get, x, y, inside, num_refs, lam, fields, t, n, fused, st):
    """One round of schro_do_split2's loops: (the record the superblock sees, block->mv[jj][ii], best_error, best_entropy)."""
    if not inside:
        mv = bytearray(BEST_MV)
        mode = mode_prediction(get, x, y)
        if mode != 1 and mode != 2:
            mode = 1
        mv[0] = (mv[0] & ~3) | mode
        px, py = vector_prediction(get, x, y, 1)
        set_vec(mv, mode - 1, px)
        set_vec(mv, 2 + mode - 1, py)
        st["outside_mode"][mode] += 1
        return mv, bytearray(BEST_MV), 0, 2
    min_score = float("inf")
    entropy = [0, 0]
    best_entropy = best_error = INT_MAX
    best_mv = bytearray(BEST_MV)
    mv = None
    for ref in range(num_refs):
        mv = bytearray(fields[ref][n].tobytes())
        set_mode(mv, ref + 1)
        entropy[ref] = block_entropy(get, x, y, mv)
        # schro_get_split2_metric
        if metric(mv) == INT_MAX:
            error = INT_MAX
            st["int_max"] += 1
        else:
            assert t[T_CHROMA + ref] >= 0
            struct.pack_into("<I", mv, 8, int(t[T_CHROMA + ref]))
            error = _i32(int(t[T_CHROMA + ref]) + metric(mv))
        score = _score(entropy[ref], lam, error, fused)
        st["ties"] += int(score == min_score)
        if min_score > score:
            min_score, best_mv, best_entropy, best_error = score, bytearray(mv), entropy[ref], _i32(metric(mv))
    area = 0
    if num_refs > 1:
        for k in range(4):                              # dx[0], dy[0] of mv_ref[0]; dx[1], dy[1] of mv_ref[1]
            set_vec(mv, k, int(fields[k & 1]["v"][n][k]))
        set_mode(mv, 3)
        area = int(t[T_AREA])
        if t[T_BI_OK]:
            struct.pack_into("<II", mv, 4, int(t[T_BI_LUMA]), int(t[T_BI_CHROMA]))
            both = int(t[T_BI_LUMA]) + int(t[T_BI_CHROMA])
            score = _score(entropy[0] + entropy[1], lam, both, fused)
            st["ties"] += int(score == min_score)
            if min_score > score:
                min_score, best_mv, best_entropy, best_error = score, bytearray(mv), entropy[0] + entropy[1], _i32(both)
    if 4 * area < best_error:
        st["dc_considered"] += 1
        st["dc_considered_one_ref"] += int(num_refs == 1)
        set_mode(mv, 0)
        if t[T_DC_ERROR] != T_NONE:
            error = int(t[T_DC_ERROR])
            for k in range(3):
                set_vec(mv, k, int(t[T_DC + k]))
            struct.pack_into("<I", mv, 4, error)
            e = sum(S.estimate_sint(int(t[T_DC + k])) for k in range(3))
            if error < best_error:
                best_mv, best_error, best_entropy = bytearray(mv), error, e
                st["dc_leftover"] += int(mv[18] != 0 or mv[19] != 0)
    st["modes"][pred_mode(best_mv)] += 1
    return best_mv, bytearray(best_mv), best_error, best_entropy


def new_stats(stats=None):
    st = stats if stats is not None else {}
    for key in ("ties", "int_max", "dc_considered", "dc_considered_one_ref", "dc_leftover", "same_sb_outside_neighbour", "other_sb_outside_neighbour",
                "inside_with_outside_neighbour"):
        st.setdefault(key, 0)
    st.setdefault("modes", [0] * 4)
    st.setdefault("outside_mode", [0] * 3)
    return st


def _stale_get(get, stale, x, y):
    """`get` for block (x, y), with the neighbours the predicate names read as they were before the call."""
    if stale is None:
        return get
    return lambda nx, ny: bytearray(20) if stale(x, y, nx, ny) else get(nx, ny)


def choose(table, params, width, height, lam, fields, order="raster", fused=False, stats=None, stale=None):
    """(motion as MV_DTYPE, the superblock table as SB_DTYPE) from the metric table and the sub-pel fields.  `stale` exists
    only for the CPU assertions of tests/long_diagonal_cases.py: a predicate (x, y, nx, ny) that makes neighbour (nx, ny) of
    block (x, y), where it says so, the record as it was before the call (20 zero bytes), as a device that missed the
    neighbour's stores would read it."""
    nbx, nby, blocks, _ = geometry(params, width, height)
    assert nbx % 4 == 0 and nby % 4 == 0
    num_refs = len(fields)
    st = new_stats(stats)
    xb, yb = blocks[0]

    def inside(x, y):
        return x * xb < width and y * yb < height

    sbx = nbx // 4
    error, entropy = np.zeros(sbx * (nby // 4), np.int64), np.zeros(sbx * (nby // 4), np.int64)
    if order == "raster":
        motion = [bytearray(20) for _ in range(nbx * nby)]

        def get(x, y):
            return motion[y * nbx + x]
        for j in range(0, nby, 4):
            for i in range(0, nbx, 4):
                block = {}
                for jj in range(4):
                    for ii in range(4):
                        x, y = i + ii, j + jj
                        for nx, ny in ((x - 1, y), (x, y - 1), (x - 1, y - 1)):
                            if nx >= 0 and ny >= 0 and not inside(nx, ny):
                                same = (nx >> 2, ny >> 2) == (x >> 2, y >> 2)
                                st["inside_with_outside_neighbour"] += int(inside(x, y))
                                st["same_sb_outside_neighbour" if same else "other_sb_outside_neighbour"] += 1
                        work, final, e, h = choose_block(_stale_get(get, stale, x, y), x, y, inside(x, y), num_refs, lam, fields, table[y * nbx + x],
                                                         y * nbx + x, fused, st)
                        motion[y * nbx + x] = work
                        block[jj, ii] = final
                        error[(j // 4) * sbx + i // 4] += e
                        entropy[(j // 4) * sbx + i // 4] += h
                for (jj, ii), rec in block.items():     # schro_motion_copy_to
                    motion[(j + jj) * nbx + i + ii] = rec
        final = motion
    else:
        assert order == "diagonal"
        working = [None] * (nbx * nby)
        final = [None] * (nbx * nby)
        for d in range(nbx + nby - 1):
            done = {}
            for y in range(max(0, d - (nbx - 1)), min(d, nby - 1) + 1):
                x = d - y

                def get(nx, ny, x=x, y=y):
                    return (working if (nx >> 2, ny >> 2) == (x >> 2, y >> 2) else final)[ny * nbx + nx]
                done[x, y] = choose_block(_stale_get(get, stale, x, y), x, y, inside(x, y), num_refs, lam, fields, table[y * nbx + x], y * nbx + x,
                                          fused, st)
            for (x, y), (work, fin, e, h) in done.items():      # (a diagonal's blocks do not see one another)
                working[y * nbx + x], final[y * nbx + x] = work, fin
                error[(y // 4) * sbx + x // 4] += e
                entropy[(y // 4) * sbx + x // 4] += h
    sb = np.zeros(error.size, SB_DTYPE)
    for k in range(error.size):
        sb["error"][k], sb["entropy"][k] = _i32(error[k]), _i32(entropy[k])
        sb["score"][k] = _score(int(sb["entropy"][k]), lam, int(sb["error"][k]), fused)
    return np.frombuffer(b"".join(bytes(r) for r in final), MV_DTYPE).copy(), sb


def split2(src, refs, params, lam, fields, extension, order="raster", fused=False, stats=None):
    """(motion, superblock table, metric table)"""
    table = metric_tables(src, refs, params, fields, extension, stats)
    motion, sb = choose(table, params, src[0].shape[1], src[0].shape[0], lam, fields, order, fused, stats)
    return motion, sb, table
