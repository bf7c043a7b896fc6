"""Guarded device allocations: what a kernel writes OUTSIDE its output, and what it reads outside its input.

DevicePlane.download () copies width x itemsize bytes of each of height rows, so a comparison with the oracle cannot see
a byte written into a row's stride padding, past the last row, in front of the plane or into a neighbouring plane.
A GuardedBlock is one device allocation filled with seeded random bytes (the canary) out of which the test carves its
planes; every plane is preceded by a guard of at least max (4096, 2 x stride) bytes and the last one is followed by
one.  After the call `check` downloads the whole block and reports, separately,

  * payload mismatches of the planes given an expected array, and
  * every byte outside the declared write footprints that is no longer the canary (a stray write).

Inputs declare an empty footprint, so "src is left untouched" is the same check; and since their padding and guards
hold random bytes, an output that depends on bytes outside its input rectangle shows up as a payload mismatch.

The bookkeeping (Layout, find_changes) is plain numpy and runs without a device (tests/test_guard_lib.py).
"""
import ctypes as C

import numpy as np

GUARD_MIN = 4096
CHUNK = 4096                    # the block crosses the host boundary as rows of CHUNK bytes


def guard_bytes(stride):
    return max(GUARD_MIN, 2 * int(stride))


def packed_row_bytes(fmt, width):
    """Bytes a packer writes per row (include/schro_hip.h, plane_frameops.cpp): YUYV / UYVY width / 2 four-byte
    groups, AYUV / ARGB 4 bytes per pixel, v216 8 bytes per pixel pair, v210 16 bytes per 6 pixels, AY64 8 per pixel."""
    return {0x100: 4 * (width // 2), 0x101: 4 * (width // 2), 0x102: 4 * width, 0x103: 4 * width,
            0x105: 8 * (width // 2), 0x106: 16 * (-(-width // 6)), 0x107: 8 * width}[fmt]


class Spec:
    """One region of a layout: a plane (height rows of width samples, `stride` bytes apart) or a span of bytes.

    footprint -- the bytes a call may write, relative to the region's origin:
      "rect"   the payload rectangle (the default);
      None     nothing (an input);
      [(byte_offset, row_stride, row_bytes, rows), ...]   a list of rectangles (dequant codeblocks);
      ("bytes", n)   [origin, origin + n) (a half-pel image)."""

    def __init__(self, name, offset, height, width, dtype, stride, footprint, extent):
        self.name, self.offset = name, int(offset)
        self.height, self.width, self.dtype, self.stride = int(height), int(width), np.dtype(dtype), int(stride)
        self.footprint, self.extent = footprint, int(extent)

    @property
    def row_bytes(self):
        return self.width * self.dtype.itemsize

    def footprint_mask(self, mask):
        """Set the bytes of the footprint in `mask` (the whole block's bool array)."""
        fp, o = self.footprint, self.offset
        if fp is None:
            return
        if fp == "rect":
            fp = [(0, self.stride, self.row_bytes, self.height)]
        elif isinstance(fp, tuple) and fp[0] == "bytes":
            mask[o:o + int(fp[1])] = True
            return
        for (off, st, rb, rows) in fp:
            if rb <= 0 or rows <= 0:
                continue
            for r in range(rows):
                a = o + off + r * st
                mask[a:a + rb] = True

    def payload(self, raw):
        """The (height, width) array of this plane inside the block's bytes `raw`."""
        v = np.lib.stride_tricks.as_strided(raw[self.offset:], shape=(self.height, self.row_bytes),
                                            strides=(self.stride, 1), writeable=False)
        return np.ascontiguousarray(v).view(self.dtype).reshape(self.height, self.width)


class Layout:
    """Where the regions of one block lie.  Each region starts at least guard_bytes (its stride) + `gap` bytes after the
    previous region's last byte (after the block start for the first), rounded up to `align`, plus `skew` bytes -- the
    lead alignment the test wants (256, 16 but not 64, bpp ...); the block ends guard_bytes after the last region."""

    def __init__(self, gap=0):
        self.specs, self.end, self.gap = [], 0, int(gap)

    def _place(self, stride, align, skew):
        start = self.end + guard_bytes(stride) + self.gap
        start = -(-start // align) * align + skew
        return start

    def plane(self, height, width, dtype, stride=None, align=256, skew=0, footprint="rect", name=None):
        dtype = np.dtype(dtype)
        row = int(width) * dtype.itemsize
        stride = row if stride is None else int(stride)
        assert stride >= row and skew < align
        off = self._place(stride, align, skew)
        extent = stride * (int(height) - 1) + row if height else 0
        s = Spec(name or "plane%d" % len(self.specs), off, height, width, dtype, stride, footprint, extent)
        self.specs.append(s)
        self.end = off + extent
        return s

    def span(self, nbytes, align=256, skew=0, footprint=None, name=None, stride=0):
        """A byte range (a slice buffer, vector records, a half-pel image)."""
        off = self._place(stride, align, skew)
        s = Spec(name or "span%d" % len(self.specs), off, 1, nbytes, np.uint8, max(int(nbytes), 1), footprint, nbytes)
        self.specs.append(s)
        self.end = off + int(nbytes)
        return s

    @property
    def nbytes(self):
        last = max((s.stride for s in self.specs), default=0)
        return -(-(self.end + guard_bytes(last)) // CHUNK) * CHUNK

    def footprint(self):
        mask = np.zeros(self.nbytes, bool)
        for s in self.specs:
            s.footprint_mask(mask)
        return mask

    def locate(self, offset):
        """(spec, row, column) of a block offset, relative to the origin of the last region that starts at or before it
        (the first region for the lead guard: a negative row)."""
        best = self.specs[0]
        for s in self.specs:
            if s.offset <= offset and s.offset >= best.offset:
                best = s
        row, col = divmod(offset - best.offset, best.stride)
        return best, row, col


def canary(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def find_changes(layout, before, after, expected=None):
    """(payload mismatches, stray writes) of a block whose bytes went from `before` to `after`.
    expected: {Spec: array} -- the payloads to compare.  Returns two lists of messages (empty: all well)."""
    mismatches, strays = [], []
    for s, want in (expected or {}).items():
        got = s.payload(after)
        want = np.asarray(want)
        if got.shape != want.shape or not np.array_equal(got, want.astype(s.dtype, copy=False)):
            bad = np.argwhere(got != want) if got.shape == want.shape else np.zeros((1, 2), int)
            y, x = (int(v) for v in bad[0])
            mismatches.append("%s: %d payload mismatches, first at (y,x)=(%d,%d) got %d want %d" % (
                s.name, len(bad), y, x, got[y, x], want[y, x]))
    changed = np.flatnonzero((before != after) & ~layout.footprint())
    if changed.size:
        groups = {}
        for off in changed:
            s = layout.locate(int(off))[0]
            groups.setdefault(s.name, []).append(int(off))
        for name, offs in groups.items():
            s, row, col = layout.locate(offs[0])
            strays.append("%s: %d stray bytes, first at (row,col)=(%d,%d) of its origin (stride %d, %d x %d): canary 0x%02x, "
                          "found 0x%02x" % (name, len(offs), row, col, s.stride, s.height, s.row_bytes, before[offs[0]],
                                            after[offs[0]]))
    return mismatches, strays


def report(mismatches, strays):
    if mismatches or strays:
        raise AssertionError("\n".join(["payload mismatch -- " + m for m in mismatches]
                                       + ["STRAY WRITE -- " + s for s in strays]))


# ---- on the device ------------------------------------------------------------------------------------------------

class GuardedPlane:
    """A plane (or span) of a GuardedBlock: .ptr / .stride / .width / .height / .dtype as the Context wrappers take
    them.  upload () writes only the payload bytes (schro_hip_upload_2d); padding and guards keep the canary."""

    def __init__(self, block, spec):
        self.block, self.spec, self.ctx = block, spec, block.ctx
        self.ptr = block.ptr + spec.offset
        self.stride, self.width, self.height, self.dtype = spec.stride, spec.width, spec.height, spec.dtype

    def upload(self, a):
        from schroedinger_amd import check
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.shape == (self.height, self.width), (a.shape, self.height, self.width)
        check(self.ctx.lib.schro_hip_upload_2d(self.ctx.h, self.ptr, self.stride, a.ctypes.data_as(C.c_void_p),
                                               a.strides[0], self.width * self.dtype.itemsize, self.height))
        self.block.before_payload(self.spec, a)
        return self

    def download(self):
        from schroedinger_amd import check
        out = np.empty((self.height, self.width), self.dtype)
        check(self.ctx.lib.schro_hip_download_2d(self.ctx.h, out.ctypes.data_as(C.c_void_p), out.strides[0], self.ptr,
                                                 self.stride, self.width * self.dtype.itemsize, self.height))
        return out

    def initial(self):
        """The plane's contents before the call (the canary, or what was uploaded)."""
        return self.spec.payload(self.block.before)

    def free(self):
        pass


class GuardedBlock:
    """One ctx.alloc block laid out by `layout`, every byte of it a seeded canary."""

    def __init__(self, ctx, layout, seed=0):
        self.ctx, self.layout = ctx, layout
        n = layout.nbytes
        self.ptr = ctx.alloc(n)
        self.before = canary(n, seed)
        self._copy(self.before, up=True)
        self.planes = {s: GuardedPlane(self, s) for s in layout.specs}

    def __getitem__(self, spec):
        return self.planes[spec]

    def _copy(self, host, up):
        from schroedinger_amd import check
        rows = host.reshape(-1, CHUNK)
        f = self.ctx.lib.schro_hip_upload_2d if up else self.ctx.lib.schro_hip_download_2d
        if up:
            check(f(self.ctx.h, self.ptr, CHUNK, rows.ctypes.data_as(C.c_void_p), CHUNK, CHUNK, rows.shape[0]))
        else:
            check(f(self.ctx.h, rows.ctypes.data_as(C.c_void_p), CHUNK, self.ptr, CHUNK, CHUNK, rows.shape[0]))

    def before_payload(self, spec, a):
        raw = a.view(np.uint8).reshape(spec.height, spec.row_bytes)
        for r in range(spec.height):
            o = spec.offset + r * spec.stride
            self.before[o:o + spec.row_bytes] = raw[r]

    def raw(self):
        out = np.empty(self.layout.nbytes, np.uint8)
        self._copy(out, up=False)
        return out

    def check(self, expected=None, extra=None):
        """Raise with every payload mismatch and stray write.  expected: {Spec or GuardedPlane: array};
        extra: more mismatch messages of the caller's (e.g. a half-pel image compared through its own download)."""
        exp = {(k.spec if isinstance(k, GuardedPlane) else k): v for k, v in (expected or {}).items()}
        mism, strays = find_changes(self.layout, self.before, self.raw(), exp)
        report(list(extra or []) + mism, strays)

    def free(self):
        if self.ptr:
            self.ctx.free(self.ptr)
            self.ptr = None
