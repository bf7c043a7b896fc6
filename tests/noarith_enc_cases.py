"""Pictures, limits and refusals of the noarith (VLC) transform-data encoder, shared by its GPU tests, the CPU walk of
schro_hip_noarith_encode_check and the sanitizer walk (tests/c/noarith_walk.cpp reads the table tests/test_noarith_host_sanitized.py writes from this module).

The pictures are tiny: luma 16 x 8 at depth 2 in 4:2:0 has chroma bands of 2 x 1, so (2, 2) and (3, 2) codeblocks per
level leave codeblocks of no width or height; 32 x 16 runs at depths 1 and 3.

The limits the kernels introduce (schroedinger_amd/csrc/noarith_enc.hip, schro_hip_internal.h), each with a picture on
either side:
  GRID_X          a sub-band's pieces and head units are walked in strides by at most 1024 workgroups;
  LAYOUT_THREADS  the layout workgroup scans a picture's codeblocks one per thread up to 1024, in runs per thread above;
  WINDOW_CODES    the pack wave takes 64 codes per step into its LDS window (sized for 64 codes of the longest length).
A piece (a codeblock's part of a sub-band row) is never cut, so there is no piece length.
"""
import functools

import numpy as np

import noarith_enc_ref as ref

GRID_X = 1024
LAYOUT_THREADS = 1024
WINDOW_CODES = 64


def iwt_sizes(lw, lh, fmt, depth):
    """(width, height) per component at the transform's size (schro_params_calculate_iwt_sizes: rounded up to 1 << depth)."""
    cw = lw if fmt == 444 else (lw + 1) // 2
    ch = (lh + 1) // 2 if fmt == 420 else lh
    up = lambda v: (v + (1 << depth) - 1) >> depth << depth
    return [(up(lw), up(lh)), (up(cw), up(ch)), (up(cw), up(ch))]


class Case:
    def __init__(self, name, dtype, lw, lh, fmt, depth, counts, mode, fill, seed=1, qbase=4):
        self.name, self.dtype, self.depth, self.mode = name, np.dtype(dtype), depth, mode
        self.sizes = iwt_sizes(lw, lh, fmt, depth)
        counts = list(counts) + [counts[-1]] * (depth + 1 - len(counts))
        self.hc, self.vc = [c[0] for c in counts], [c[1] for c in counts]
        self.nsub = 1 + 3 * depth
        # one quant index per sub-band (trap c), unlike from sub-band to sub-band
        self.qidx = [[(qbase + 7 * k + 3 * i) % 61 for i in range(self.nsub)] for k in range(3)]
        rng = np.random.default_rng(seed)
        self.planes = [np.zeros((h, w), self.dtype) for w, h in self.sizes]
        fill(self, rng)

    def band(self, k, i):
        return ref.subband(self.planes[k], self.depth, i)

    def counts(self, i):
        return ref.codeblock_counts(i, self.hc, self.vc)

    def ncodeblocks(self):
        return sum(self.counts(i)[0] * self.counts(i)[1] for i in range(self.nsub))

    @functools.lru_cache(maxsize=None)
    def expected(self):
        """(bytes, subband_bits, stats) of the restatement: computed once, shared, never changed."""
        return ref.encode_transform_data(self.planes, self.depth, self.hc, self.vc, self.mode, self.qidx)

    def record_indices(self, k):
        """The quant index of every record of component k in schro_hip_codeblock_layout's order."""
        out = []
        for i in range(self.nsub):
            hc, vc = self.counts(i)
            out += [self.qidx[k][i]] * (hc * vc)
        return out


def fill_zero(case, rng):
    pass


def fill_random(case, rng, lim=300):
    for p in case.planes:
        v = rng.integers(-lim, lim + 1, p.shape)
        p[...] = np.where(rng.random(p.shape) < 0.45, 0, v)


def fill_sparse(case, rng):
    """Zero codeblocks among non-zero ones, whole zero sub-bands among them, and a zero last sub-band."""
    fill_random(case, rng, 40)
    for k in range(3):
        for i in range(case.nsub):
            b = case.band(k, i)
            hc, vc = case.counts(i)
            if (i + k) % 4 == 2:
                b[...] = 0
            for y in range(vc):
                for x in range(hc):
                    if (x + 2 * y + i + k) % 3 == 0:
                        ref.get_codeblock(b, x, y, hc, vc)[...] = 0
    case.band(2, case.nsub - 1)[...] = 0


def fill_extremes(case, rng):
    """The longest codes: +-32767 and -32768 on s16; +-(2^28 - 1) and 2^31 - 1 on s32."""
    if case.dtype == np.int16:
        pool = np.array([32767, -32767, -32768, 0, 1, -1, 255, -256], np.int64)
    else:
        pool = np.array([(1 << 28) - 1, -((1 << 28) - 1), (1 << 31) - 1, -((1 << 31) - 1), 0, 1, -1, 65535, -65536], np.int64)
    for p in case.planes:
        p[...] = pool[rng.integers(0, len(pool), p.shape)]


def fill_longest(case, rng):
    """Every value the longest code: 32 bits on s16, 64 on s32 -- a full window at every step.  (+-32767 on s16: rows
    of -32768 alone sum to a multiple of 65536 and the sub-band would be called zero.)"""
    for p in case.planes:
        p[...] = 32767 if case.dtype == np.int16 else (1 << 31) - 1
        p[:, 1::3] *= -1


def fill_trap_codeblock(case, rng):
    """Trap (a), one way: a row (-32768, -32768) alone in a codeblock -- its 16-bit row sum wraps to 0, the codeblock is
    called zero -- next to codeblocks that are written."""
    for k in range(3):
        for i in range(1, case.nsub):
            case.band(k, i)[...] = 5
    b = case.band(0, 1)
    cb = ref.get_codeblock(b, 0, 0, *case.counts(1))
    cb[...] = 0
    cb[0, :2] = -32768


def fill_trap_subband(case, rng):
    """Trap (a), the other way: a sub-band row (32767, 1 | 32767, 1) across two codeblocks sums to 65536: the sub-band is
    called zero though neither codeblock is."""
    fill_random(case, rng, 9)
    b = case.band(0, 2)
    hc, vc = case.counts(2)
    b[...] = 0
    for x in range(2):
        ref.get_codeblock(b, x, 0, hc, vc)[0, :2] = (32767, 1)


CB = {"one": [(1, 1)], "two": [(2, 2)], "three": [(3, 2)]}


def _cases():
    out = []
    for dtype in (np.int16, np.int32):
        t = "s16" if dtype == np.int16 else "s32"
        for cname, counts in CB.items():
            for mode in (0, 1):
                out.append(Case("%s-16x8-d2-%s-m%d" % (t, cname, mode), dtype, 16, 8, 420, 2, counts, mode, fill_random, 3))
        out.append(Case(t + "-32x16-d1-three-m1", dtype, 32, 16, 420, 1, CB["three"], 1, fill_random, 4))
        out.append(Case(t + "-32x16-d3-two-m0", dtype, 32, 16, 420, 3, CB["two"], 0, fill_random, 5))
        out.append(Case(t + "-32x16-d3-mixed-m1", dtype, 32, 16, 422, 3, [(1, 1), (2, 1), (3, 2), (4, 3)], 1, fill_sparse, 6))
        out.append(Case(t + "-zero-d2", dtype, 16, 8, 420, 2, CB["two"], 1, fill_zero))
        out.append(Case(t + "-zero-d6", dtype, 64, 64, 444, 6, CB["one"], 0, fill_zero))
        out.append(Case(t + "-sparse-d2", dtype, 16, 8, 420, 2, CB["three"], 0, fill_sparse, 7))
        out.append(Case(t + "-extremes-d1", dtype, 32, 16, 444, 1, CB["two"], 1, fill_extremes, 8))
        out.append(Case(t + "-d0", dtype, 10, 6, 420, 0, CB["two"], 1, fill_random, 9))
        # WINDOW_CODES: pieces of 64 and of 65 codes, each of the longest length
        out.append(Case(t + "-window-64", dtype, 128, 2, 444, 1, CB["one"], 0, fill_longest))
        out.append(Case(t + "-window-65", dtype, 130, 2, 444, 1, CB["one"], 0, fill_longest))
        # rows of 200 codes: four steps of the pack wave, the carry handed on three times
        out.append(Case(t + "-wide-400", dtype, 400, 4, 422, 1, [(1, 1), (1, 2)], 1, fill_random, 10))
    # trap (a) is the s16 test's
    out.append(Case("s16-trap-codeblock", np.int16, 16, 8, 420, 1, CB["two"], 0, fill_trap_codeblock))
    out.append(Case("s16-trap-subband", np.int16, 16, 8, 420, 1, CB["two"], 1, fill_trap_subband, 11))
    # GRID_X: bands of 16 x 8 at depth 1 cut into 127 / 128 columns of codeblocks: 8 * 127 + 2 = 1018 and 8 * 128 + 2 = 1026 units
    out.append(Case("s16-grid-1018", np.int16, 32, 16, 420, 1, [(1, 1), (127, 1)], 1, fill_random, 12))
    out.append(Case("s16-grid-1026", np.int16, 32, 16, 420, 1, [(1, 1), (128, 1)], 1, fill_random, 13))
    # LAYOUT_THREADS: 3 * (1 + 3 * 113) = 1020 and 3 * (1 + 3 * 114) = 1029 codeblocks in the picture
    out.append(Case("s32-scan-1020", np.int32, 32, 16, 420, 1, [(1, 1), (113, 1)], 0, fill_random, 14))
    out.append(Case("s32-scan-1029", np.int32, 32, 16, 420, 1, [(1, 1), (114, 1)], 1, fill_random, 15))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert BY_NAME["s16-grid-1018"].band(0, 1).shape[0] * 127 + 2 == 1018 < GRID_X < 1026
assert BY_NAME["s32-scan-1020"].ncodeblocks() * 3 == 1020 <= LAYOUT_THREADS < BY_NAME["s32-scan-1029"].ncodeblocks() * 3 == 1029
assert BY_NAME["s32-window-64"].band(0, 1).shape[1] == WINDOW_CODES == BY_NAME["s16-window-65"].band(0, 1).shape[1] - 1
# three unlike pictures in one call, per sample size
MIXED = {2: ["s16-16x8-d2-three-m1", "s16-32x16-d3-mixed-m1", "s16-trap-subband"],
         4: ["s32-16x8-d2-two-m0", "s32-extremes-d1", "s32-scan-1029"]}


# ---- the refusal table: (name, change to a valid picture description, fragment of the message) ---------------------------
# A description is a dict: bpp, depth, mode, sizes [(w, h)] * 3, hc, vc, stride [3], bytes [3], records [3] (lists of
# [dst_offset, dst_stride, width, height, src_offset, src_bytes, quant_index]), quant [3], out, capacity, result (addresses;
# nothing is dereferenced by the check).

def layout_records(w, h, depth, hc, vc, stride, bpp):
    """schro_hip_codeblock_layout restated (the decoder's loop, schrodecoder.c:3558-3577)."""
    recs = []
    for index in range(1 + 3 * depth):
        position = ref.position_of(index)
        level = position >> 2
        shift = depth - level
        bw, bh, bstride = w >> shift, h >> shift, stride << shift
        base = (bstride >> 1 if position & 2 else 0) + (bw * bpp if position & 1 else 0)
        nh, nv = ref.codeblock_counts(index, hc, vc)
        for y in range(nv):
            ymin, ymax = (bh * y) // nv, (bh * (y + 1)) // nv
            xmin, acc, cw = 0, 0, bw // nh
            inc = bw - nh * cw
            for x in range(nh):
                x0 = xmin
                xmin += cw
                acc += inc
                if acc >= nh:
                    acc -= nh
                    xmin += 1
                recs.append([base + ymin * bstride + x0 * bpp, bstride, xmin - x0, ymax - ymin, -1, 0, 0])
    return recs


def describe(lw=32, lh=16, fmt=420, depth=2, counts=((2, 2),), mode=1, bpp=2):
    sizes = iwt_sizes(lw, lh, fmt, depth)
    counts = list(counts) + [counts[-1]] * (depth + 1 - len(counts))
    d = {"bpp": bpp, "depth": depth, "mode": mode, "sizes": sizes, "hc": [c[0] for c in counts], "vc": [c[1] for c in counts]}
    d["stride"] = [(w * bpp + 63) // 64 * 64 for w, h in sizes]
    d["bytes"] = [s * h for s, (w, h) in zip(d["stride"], sizes)]
    d["records"] = [layout_records(w, h, depth, d["hc"], d["vc"], s, bpp) for (w, h), s in zip(sizes, d["stride"])]
    d["quant"] = [0x10000000, 0x20000000, 0x30000000]
    d["out"], d["capacity"], d["result"] = 0x40000000, 1 << 20, 0x50000000
    return d


def _set(key, value, k=None):
    def change(d):
        if k is None:
            d[key] = value
        else:
            d[key][k] = value
    return change


def _record(k, n, field, value):
    def change(d):
        d["records"][k][n][field] = value
    return change


def _size(k, w, h):
    def change(d):
        d["sizes"][k] = (w, h)
    return change


def _big(d):
    # depth 0, 4:4:4, 16384 wide: 3 * 16384 * h samples of 4 (s16) or 8 (s32) bytes reach 2^29 at h = 2731 / 1366
    d.update(describe(16384, 2731 if d["bpp"] == 2 else 1366, 444, 0, ((1, 1),), 0, d["bpp"]))


def _just_below(d):
    d.update(describe(16384, 2730 if d["bpp"] == 2 else 1365, 444, 0, ((1, 1),), 0, d["bpp"]))


REFUSALS = [
    ("bpp-1", _set("bpp", 1), "bytes_per_sample must be 2 or 4"),
    ("bpp-3", _set("bpp", 3), "bytes_per_sample must be 2 or 4"),
    ("depth-7", _set("depth", 7), "transform_depth 7"),
    ("depth-negative", _set("depth", -1), "transform_depth -1"),
    ("width-odd", _size(1, 18, 4), "picture 0, component 1"),
    ("height-zero", _size(2, 16, 0), "picture 0, component 2"),
    ("width-32768", _size(0, 32768, 16), "picture 0, component 0"),
    ("counts-zero", _set("hc", 0, 1), "codeblocks at level 1"),
    ("counts-32768", _set("vc", 32768, 0), "codeblocks at level 0"),
    ("mode-2", _set("mode", 2), "codeblock_mode_index 2"),
    ("out-null", _set("out", 0), "out is NULL"),
    ("result-null", _set("result", 0), "result is NULL or unaligned"),
    ("result-odd", _set("result", 0x50000002), "result is NULL or unaligned"),
    ("quant-null", _set("quant", 0, 1), "quant[1] is NULL or misaligned"),
    ("quant-odd", _set("quant", 0x30000001, 2), "quant[2] is NULL or misaligned"),
    ("stride-short", _set("stride", 62, 0), "stride[0] 62"),
    ("stride-odd", _set("stride", 65, 1), "stride[1] 65"),
    ("records-missing", lambda d: d["records"][1].pop(), "component 1: 27 records, the stated counts make 28"),
    ("record-offset", _record(0, 5, 0, 2), "component 0, sub-band 1, record 5"),
    ("record-stride", _record(2, 0, 1, 64), "component 2, sub-band 0, record 0"),
    ("record-width", _record(1, 9, 2, 3), "component 1, sub-band 2, record 9"),
    ("record-height", _record(0, 27, 3, 9), "component 0, sub-band 6, record 27"),
    ("quant-index-61", lambda d: [r.__setitem__(6, 61) for r in d["records"][0][4:8]], "sub-band 1, record 4: quant_index 61"),
    ("mixed-indices", _record(1, 14, 6, 9), "picture 0, component 1, sub-band 3: record 14 has quant index 9"),
    ("plane-short", _set("bytes", 64 * 16 - 1, 0), "component 0, sub-band"),
    ("out-overlaps", _set("out", 0x20000010), "out overlaps quant[1]"),
    ("bound-2^29", _big, "bit positions are 32-bit"),
]
# the other side of limits that have one: these descriptions pass
ACCEPTED = [
    ("plain", lambda d: None),
    ("depth-6", lambda d: d.update(describe(64, 64, 444, 6, ((1, 1),), 0, d["bpp"]))),
    ("depth-0", lambda d: d.update(describe(10, 6, 420, 0, ((2, 2),), 1, d["bpp"]))),
    ("counts-32767", lambda d: d.update(describe(32, 16, 420, 1, ((32767, 1), (1, 1)), 0, d["bpp"]))),
    ("quant-index-60", lambda d: [r.__setitem__(6, 60) for r in d["records"][0][4:8]]),
    ("width-32767-ish", lambda d: d.update(describe(32766, 2, 444, 1, ((1, 1),), 0, d["bpp"]))),
    ("plane-exact", _set("bytes", 64 * 15 + 32 * 2, 0)),
    ("capacity-huge", _set("capacity", (1 << 40))),
    ("below-2^29", _just_below),
]


def c_picture(d, L, C):
    """The _lib.NoarithPicture of a description (and what it points to)."""
    a = L.NoarithPicture()
    keep = []
    for k in range(3):
        tab = (L.Codeblock * max(len(d["records"][k]), 1))()
        for t, r in zip(tab, d["records"][k]):
            t.dst_offset, t.dst_stride, t.width, t.height, t.src_offset, t.src_bytes, t.quant_index = r
        keep.append(tab)
        a.quant[k], a.bytes[k], a.stride[k] = d["quant"][k] or None, d["bytes"][k], d["stride"][k]
        a.iwt_width[k], a.iwt_height[k] = d["sizes"][k]
        a.codeblocks[k], a.ncodeblocks[k] = tab, len(d["records"][k])
    a.transform_depth, a.codeblock_mode_index = d["depth"], d["mode"]
    for l in range(min(len(d["hc"]), 7)):
        a.horiz_codeblocks[l], a.vert_codeblocks[l] = d["hc"][l], d["vc"][l]
    a.out, a.capacity, a.result = d["out"] or None, d["capacity"], d["result"] or None
    return a, keep
