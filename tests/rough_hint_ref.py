"""The reference's hint levels of the hierarchical rough motion search restated in numpy (checker only).

  rough_scan_hint   schro_rough_me_heirarchical_scan_hint, schroroughmotion.c:143-300
  rough_scan        schro_rough_me_heirarchical_scan, schroroughmotion.c:47-62

Written literally from the C text on analysis_ref.scan_setup / do_scan / get_min / rough_scan_nohint: the candidate list
and its order, the skip rules of the candidate test, the int16_t members and the arithmetic >> shift of negative vectors.
Like rough_scan_nohint it rests on the C text alone (the loop needs the full library); tests/test_rough_hint_ref.py checks
it against properties the C text implies.

One place where the C text gives no answer: a block of no width or height (x_num_blocks * xbsep beyond the plane) whose
window is valid.  Every candidate is skipped there, every SAD of the scan is 0, and schro_metric_scan_get_min takes its
starting minimum from metrics[] at the gravity position, which can lie OUTSIDE the window (a stale entry of the array).
An empty block has SAD 0 at every position, so the restatement reads 0 there: nothing is strictly smaller, the gravity
vector is kept with metric 0.  `stats` counts how often this happens."""
import numpy as np

import analysis_ref as A
import oracle_lib as O

NOHINT_DISTANCE, HINT_DISTANCE = 12, 4          # schroroughmotion.c:58-60


def _int16(v):
    return int(np.int16(np.uint16(int(v) & 0xffff)))


def block_order(nbx, nby, skip, order):
    """The blocks (i, j) of a level: "raster" as the C loops run, "diagonal" by anti-diagonals (i + j) / skip, the rows of
    a diagonal in any order (here: bottom to top, the opposite of raster)."""
    blocks = [(i, j) for j in range(0, nby, skip) for i in range(0, nbx, skip)]
    if order == "raster":
        return blocks
    assert order == "diagonal"
    return sorted(blocks, key=lambda b: ((b[0] + b[1]) // skip, -b[1]))


def candidates(mvs, hint_field, nbx, nby, i, j, shift, ref_index):
    """[(dx, dy)] of schroroughmotion.c:199-228, in the list's order."""
    skip, mask = 1 << shift, ~((1 << (shift + 1)) - 1)
    out = [(0, 0)]
    for m in range(4):
        l = (i + skip * (-1 + 2 * (m & 1))) & mask        # (a negative value masked stays negative)
        k = (j + skip * (-1 + (m & 2))) & mask
        if 0 <= l < nbx and 0 <= k < nby:
            v = hint_field[k * nbx + l]["v"]
            out.append((int(v[ref_index]), int(v[2 + ref_index])))
    for ok, (l, k) in ((i > 0, (i - skip, j)), (j > 0, (i, j - skip)), (i > 0 and j > 0, (i - skip, j - skip))):
        if ok:
            v = mvs[k * nbx + l]["v"]
            out.append((int(v[ref_index]), int(v[2 + ref_index])))
    return out


def rough_scan_hint(frame, ref, params, shift, distance, ref_index, hint_field, extension=0, order="raster", stats=None, sad=None):
    """The motion field of schro_rough_me_heirarchical_scan_hint (O.MV_DTYPE records, x_num_blocks * y_num_blocks);
    frame and ref are the luma planes at pyramid level `shift`, hint_field the field of level shift + 1.
    stats (a dict, or None) counts what the blocks met; sad (or None): sad (x0, y0, x, y, width, height) replaces the
    candidate test's metric (schro_metric_get)."""
    nbx, nby, xb, yb = (int(params[k]) for k in ("x_num_blocks", "y_num_blocks", "xbsep_luma", "ybsep_luma"))
    h, w = frame.shape
    hint_field = np.asarray(hint_field)
    assert hint_field.dtype == O.MV_DTYPE and hint_field.size == nbx * nby
    mvs = np.zeros(nbx * nby, O.MV_DTYPE)
    mvs["flags"] = 1            # schro_motion_field_set (mf, 0, 1)
    skip = 1 << shift
    stats = stats if stats is not None else {}
    for key in ("blocks", "cand", "skip_negative", "skip_empty", "skip_beyond", "all_skipped", "invalid_window", "empty_block_scan",
                "gravity_outside"):
        stats.setdefault(key, 0)
    f32, r32 = frame.astype(np.int32), ref.astype(np.int32)
    for (i, j) in block_order(nbx, nby, skip, order):
        stats["blocks"] += 1
        x0, y0 = (i * xb) >> shift, (j * yb) >> shift
        ow, oh = max(0, w - x0), max(0, h - y0)         # schro_frame_get_subdata: orig.width, orig.height
        cands = candidates(mvs, hint_field, nbx, nby, i, j, shift, ref_index)
        assert len(cands) <= 10
        min_m, min_metric = 0, A.METRIC_INVALID
        tested = 0
        for m, (dx, dy) in enumerate(cands):
            stats["cand"] += 1
            x, y = (i * xb + dx) >> shift, (j * yb + dy) >> shift
            if x < 0 or y < 0:
                stats["skip_negative"] += 1
                continue
            rw, rh = max(0, w - x), max(0, h - y)
            width, height = min(xb, ow), min(yb, oh)
            if width == 0 or height == 0:
                stats["skip_empty"] += 1
                continue
            if rw < width or rh < height:
                stats["skip_beyond"] += 1
                continue
            tested += 1
            if sad is not None:
                metric = sad(x0, y0, x, y, width, height)
            else:
                metric = int(np.abs(f32[y0:y0 + height, x0:x0 + width] - r32[y:y + height, x:x + width]).sum())
            if metric < min_metric:
                min_metric, min_m = metric, m
        if not tested:
            stats["all_skipped"] += 1
        dx, dy = cands[min_m][0] >> shift, cands[min_m][1] >> shift
        s = dict(x=(i >> shift) * xb, y=(j >> shift) * yb, gravity_x=dx, gravity_y=dy, dx=dx, dy=dy)
        s["block_width"], s["block_height"] = min(w - s["x"], xb), min(h - s["y"], yb)
        s["ref_x"], s["ref_y"], s["scan_width"], s["scan_height"] = A.scan_setup(
            s["x"], s["y"], s["block_width"], s["block_height"], w, h, extension, dx, dy, distance)
        assert s["scan_width"] <= A.LIMIT_METRIC_SCAN and s["scan_height"] <= A.LIMIT_METRIC_SCAN
        mv = mvs[j * nbx + i]
        if s["scan_width"] <= 0 or s["scan_height"] <= 0:
            stats["invalid_window"] += 1
            mv["v"][ref_index] = mv["v"][2 + ref_index] = 0
            mv["metric"] = A.METRIC_INVALID
            continue
        gi, gj = dx + s["x"] - s["ref_x"], dy + s["y"] - s["ref_y"]
        if s["block_width"] <= 0 or s["block_height"] <= 0:
            # SAD 0 everywhere, also at a gravity position outside the window (the module's docstring)
            stats["empty_block_scan"] += 1
            stats["gravity_outside"] += not (0 <= gi < s["scan_width"] and 0 <= gj < s["scan_height"])
            assert not tested and (dx, dy) == (0, 0)
            m = 0
        else:
            dx, dy, m = A.get_min(A.do_scan(frame, ref, s), s)
        mv["metric"] = m
        mv["v"][ref_index] = _int16(dx << shift)
        mv["v"][2 + ref_index] = _int16(dy << shift)
    return mvs


def rough_scan(frames, refs, params, n_levels, ref_index, extension=0, order="raster", stats=None):
    """schro_rough_me_heirarchical_scan: frames[k], refs[k] are the luma planes at pyramid level k (get_downsampled).
    Returns the fields by level: [None, field of level 1, ..., field of level n_levels]."""
    assert int(params["x_num_blocks"]) != 0 and int(params["y_num_blocks"]) != 0
    fields = [None] * (n_levels + 1)
    fields[n_levels] = A.rough_scan_nohint(frames[n_levels], refs[n_levels], params, n_levels, NOHINT_DISTANCE, ref_index, extension)
    for i in range(n_levels - 1, 0, -1):
        fields[i] = rough_scan_hint(frames[i], refs[i], params, i, HINT_DISTANCE, ref_index, fields[i + 1], extension, order, stats)
    return fields
