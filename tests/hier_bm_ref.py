"""The reference's hierarchical block matching -- the DEFAULT encoder's motion search -- restated in numpy (checker only).

  hbm_scan_hint   schro_hierarchical_bm_scan_hint, schrohierbm.c:174-383
  hbm_scan        schro_hbm_scan, schrohierbm.c:158-172, and the level-0 call of schro_encoder_motion_predict_pel
                  (schromotionest.c:123-127)
  block_sad       schro_metric_block_sad_slow, schrometric.c:332-375 (what schro_metric_fast_block calls)

Written literally from the C text on analysis_ref.scan_setup / do_scan / get_min: the candidate list and its order (zero,
the five-point star of parents, left, above, above-left), the removal of duplicates that keeps the LAST occurrence, the
clamp of the candidates, the metric over all three components, the int16_t members and the arithmetic >> of negative
vectors.  Like rough_hint_ref it rests on the C text alone (the loop needs the full library); tests/test_hier_bm_ref.py
checks it against properties the C text implies.

Samples outside a plane are its edge-extended apron: coordinates are clamped (analysis_ref.block_at).  The literal checks
of schro_frame_block_is_valid and of SCHRO_ASSERT (-1 < min_m) stay as assertions: with extension >= max (xbsep, ybsep)
they cannot fire.  use_chroma is off (enable_chroma_me's default): the scan is luma only, chroma_metric is 0."""
import numpy as np

import analysis_ref as A
import oracle_lib as O

INT_MAX = 0x7fffffff
STAR = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))       # schrohierbm.c:266
STATS = ("blocks", "skipped", "cand", "dropped", "clamped", "order_ties", "all_duplicates")


def _int16(v):
    return int(np.int16(np.uint16(int(v) & 0xffff)))


def _clamp(x, a, b):
    return a if x < a else (b if x > b else x)


def round_up_shift(x, y):
    return (x + (1 << y) - 1) >> y


def split_of(shift):
    return 0 if shift > 1 else (1 if shift == 1 else 2)


def field_set(n, split, pred_mode):
    """schro_motion_field_set (schromotionest.c:417-432): pred_mode in bits 0-1, split in bits 3-4, everything else 0."""
    mvs = np.zeros(n, O.MV_DTYPE)
    mvs["flags"] = pred_mode | (split << 3)
    return mvs


def block_order(nbx, nby, skip, order):
    blocks = [(i, j) for j in range(0, nby, skip) for i in range(0, nbx, skip)]
    if order == "raster":
        return blocks
    assert order == "diagonal"
    return sorted(blocks, key=lambda b: ((b[0] + b[1]) // skip, -b[1]))


def candidates(mvs, hint_field, nbx, nby, i, j, shift, ref_index):
    """[(dx, dy)] of schrohierbm.c:258-294, unshifted, in the list's order."""
    skip, mask = 1 << shift, ~((1 << (shift + 1)) - 1)
    out = [(0, 0)]
    if hint_field is not None:
        l, k = i & mask, j & mask
        for (ox, oy) in STAR:
            ll, kk = l + ox * skip * 2, k + oy * skip * 2
            if 0 <= ll < nbx and 0 <= kk < nby:
                v = hint_field[kk * nbx + ll]["v"]
                out.append((int(v[ref_index]), int(v[2 + ref_index])))
    for ok, (l, k) in ((i > 0, (i - skip, j)), (j > 0, (i, j - skip)), (i > 0 and j > 0, (i - skip, j - skip))):
        if ok:
            v = mvs[k * nbx + l]["v"]
            out.append((int(v[ref_index]), int(v[2 + ref_index])))
    assert len(out) <= 9
    return out


def remove_duplicates(cands):
    """schrohierbm.c:298-321: entry k goes when a LATER entry equals it; the last entry always stays."""
    n = len(cands)
    return [c for k, c in enumerate(cands) if k == n - 1 or c not in cands[k + 1:]]


def first_occurrences(cands):
    out = []
    for c in cands:
        if c not in out:
            out.append(c)
    return out


def _block_is_valid(w, h, ext, x, y, sx, sy):
    return not (x < -ext or y < -ext or x + sx > w + ext or y + sy > h + ext)


def block_sad(frame, ref, x, y, dx, dy, xb, yb, h_shift, v_shift, extension):
    """schro_metric_block_sad_slow over the three components of frame and ref ((Y, U, V) planes)."""
    h, w = frame[0].shape
    if not _block_is_valid(w, h, extension, x, y, xb, yb) or not _block_is_valid(w, h, extension, x + dx, y + dy, xb, yb):
        return INT_MAX
    metric = 0
    for k in range(3):
        hs, vs = (h_shift, v_shift) if k else (0, 0)
        ph, pw = frame[k].shape
        fx, fy = x >> hs, y >> vs
        width, height = min(pw - fx, xb >> hs), min(ph - fy, yb >> vs)
        if width <= 0 or height <= 0:
            continue
        a = frame[k][fy:fy + height, fx:fx + width].astype(np.int32)
        b = A.block_at(ref[k], (x + dx) >> hs, (y + dy) >> vs, width, height).astype(np.int32)
        metric += int(np.abs(a - b).sum())
    return metric


def _choose(cands, metric_of):
    min_m, min_metric = -1, INT_MAX
    for m, c in enumerate(cands):
        metric = metric_of(c)
        if metric < min_metric:
            min_metric, min_m = metric, m
    assert min_m > -1           # SCHRO_ASSERT (-1 < min_m), schrohierbm.c:347
    return min_m


def hbm_scan_hint(frame, ref, params, shift, h_range, ref_index, hint_field, h_shift, v_shift, extension, order="raster", stats=None):
    """The motion field of schro_hierarchical_bm_scan_hint (O.MV_DTYPE records, x_num_blocks * y_num_blocks): frame and
    ref are the (Y, U, V) planes at pyramid level `shift`, hint_field the field of level shift + 1 or None."""
    nbx, nby, xb, yb = (int(params[k]) for k in ("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"))
    h, w = frame[0].shape
    for k in (1, 2):
        assert frame[k].shape == ref[k].shape == (round_up_shift(h, v_shift), round_up_shift(w, h_shift)), frame[k].shape
    assert extension >= max(xb, yb)
    if hint_field is not None:
        hint_field = np.asarray(hint_field)
        assert hint_field.dtype == O.MV_DTYPE and hint_field.size == nbx * nby
    mvs = field_set(nbx * nby, split_of(shift), ref_index + 1)
    skip = 1 << shift
    stats = stats if stats is not None else {}
    for key in STATS:
        stats.setdefault(key, 0)
    for (i, j) in block_order(nbx, nby, skip, order):
        x0, y0 = (i * xb) >> shift, (j * yb) >> shift
        if not (w > x0) or not (h > y0):
            stats["skipped"] += 1
            continue
        stats["blocks"] += 1
        width0, height0 = min(w - x0, xb), min(h - y0, yb)
        assert width0 > 0 and height0 > 0
        cands = candidates(mvs, hint_field, nbx, nby, i, j, shift, ref_index)
        left = remove_duplicates(cands)
        stats["cand"] += len(cands)
        stats["dropped"] += len(cands) - len(left)
        stats["all_duplicates"] += len(left) == 1 and len(cands) > 1

        def clamped(c):
            dx = _clamp((c[0] >> shift) + x0, -width0, w) - x0
            dy = _clamp((c[1] >> shift) + y0, -height0, h) - y0
            return dx, dy

        def metric_of(c):
            dx, dy = clamped(c)
            return block_sad(frame, ref, x0, y0, dx, dy, xb, yb, h_shift, v_shift, extension)

        stats["clamped"] += sum(clamped(c) != (c[0] >> shift, c[1] >> shift) for c in left)
        win = left[_choose(left, metric_of)]
        first = first_occurrences(cands)
        stats["order_ties"] += first[_choose(first, metric_of)] != win
        dx, dy = win[0] >> shift, win[1] >> shift
        dx = max(-width0 - x0, min(w - x0, dx))
        dy = max(-height0 - y0, min(h - y0, dy))
        s = dict(x=x0, y=y0, block_width=width0, block_height=height0, gravity_x=dx, gravity_y=dy, dx=dx, dy=dy)
        s["ref_x"], s["ref_y"], s["scan_width"], s["scan_height"] = A.scan_setup(x0, y0, width0, height0, w, h, extension, dx, dy, h_range)
        assert 0 < s["scan_width"] <= A.LIMIT_METRIC_SCAN and 0 < s["scan_height"] <= A.LIMIT_METRIC_SCAN
        dx, dy, m = A.get_min(A.do_scan(frame[0], ref[0], s), s)
        mv = mvs[j * nbx + i]
        mv["metric"] = m
        mv["chroma_metric"] = 0
        mv["v"][ref_index] = _int16(dx << shift)
        mv["v"][2 + ref_index] = _int16(dy << shift)
        mv["flags"] = (ref_index + 1) | (split_of(shift) << 3)         # pred_mode = ref + 1, using_global = 0
    return mvs


def chain_ranges(n_levels):
    """h_range by level of schro_hbm_scan: 20 at the top, halved per level, never under 3; level 0: 3."""
    out = {n_levels: 20, 0: 3}
    half = 20 >> 1
    for i in range(n_levels - 1, 0, -1):
        out[i] = max(3, half)
        half >>= 1
    return out


def pyramid3(planes, n_levels):
    """[level][component] of analysis_ref.pyramid per component."""
    per = [A.pyramid(p, n_levels) for p in planes]
    return [tuple(per[c][k] for c in range(3)) for k in range(n_levels + 1)]


def hbm_scan(frames, refs, params, n_levels, ref_index, h_shift, v_shift, extension, with_level0=True, order="raster", stats=None):
    """schro_hbm_scan, then (with_level0) schro_hierarchical_bm_scan_hint (hbm, 0, 3): frames[k], refs[k] are the (Y, U, V)
    planes at pyramid level k.  Returns the fields by level, entry 0 None without level 0."""
    assert n_levels > 0
    ranges = chain_ranges(n_levels)
    fields = [None] * (n_levels + 1)
    for k in range(n_levels, -1 if with_level0 else 0, -1):
        hint = fields[k + 1] if k < n_levels else None
        fields[k] = hbm_scan_hint(frames[k], refs[k], params, k, ranges[k], ref_index, hint, h_shift, v_shift, extension, order, stats)
    return fields
