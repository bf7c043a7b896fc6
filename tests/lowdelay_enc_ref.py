"""The checker of the low-delay slice encoder: schro_encoder_encode_lowdelay_transform_data restated in numpy / Python.

What is restated, file:line of the reference (schroedinger/):
  schrolowdelay.c:1150-1200  the slice loop and the accumulator that sizes the slices      encode ()
  schrolowdelay.c:1116-1148  schro_encoder_pick_slice_index                                 _pick ()
  schrolowdelay.c:927-1062   schro_encoder_estimate_slice (USE_TRAILING_DEAD_ZONE is off)   _Slice.estimate ()
  schrolowdelay.c:853-904    quantise_block, quantise_dc_block                              quantise_vec (), _Slice._ll ()
  schrolowdelay.c:765-783    schro_dc_predict (schro_divide3: schroutils.h:64)              dc_predict ()
  schrolowdelay.c:785-839    schro_encoder_encode_slice                                     _Slice.write ()
  schroutils.c:179-235       schro_quantise / schro_dequantise                              quantise_vec (), dequantise_vec ()
  schropack.c:137-226        schro_pack_encode_sint / schro_pack_estimate_sint              sint_codes (), estimate_sint_vec ()
  schroframe.c:1865-1884     schro_frame_data_get_codeblock                                 codeblock ()
  schroparams.c:319-368      schro_subband_get_frame_data / _get_position                   subband ()
The tables are the reference's numbers (tests/golden/quant_tables_encoder.json, through quant_ref.tables ()).

High bands are vectorised per slice; the LL recurrence and the index search are plain loops.  quant_data is int16_t in the
reference: every quantised value is wrapped when stored (w16) and the estimate, the dequantisation and the bits use the
wrapped value.  One departure, as in the library: where the reference asserts because even index 64 over-runs, the slice
is cut at its last bit and flagged."""
import numpy as np

import quant_ref as Q


def w16(v):
    return ((v + 32768) & 0xffff) - 32768


def ilog2up(x):
    """schrolowdelay.c:94-105: the bit length"""
    return int(x).bit_length()


def schro_pack_estimate_sint(value):
    """schropack.c:204-226 on a Python int"""
    value = abs(value)
    n_bits = (value + 1).bit_length()
    return n_bits + n_bits - 1 + (1 if value else 0)


def schro_pack_encode_sint(value):
    """schropack.c:148-178 on a Python int: the list of bits"""
    sign, value = (1, -value) if value < 0 else (0, value)
    v = value + 1
    n_bits = v.bit_length()
    bits = []
    for i in range(n_bits - 1):
        bits += [0, (v >> (n_bits - 2 - i)) & 1]
    bits.append(1)
    if value:
        bits.append(sign)
    return bits


def _tables():
    t = Q.tables()
    return np.array(t["schro_table_quant"], np.int64), np.array(t["schro_table_offset_1_2"], np.int64)


def quantise_vec(value, factor, offset):
    """schro_quantise (schroutils.c:197-229) on int64 arrays (factor / offset arrays or ints); NOT yet wrapped to int16"""
    value = np.asarray(value, np.int64)
    x = np.abs(value) << 2
    q = np.where(x < offset, 0, (x - (offset - factor // 2)) // factor)      # x - off >= 0 wherever x >= offset
    return np.where(value < 0, -q, q)


def dequantise_vec(q, factor, offset):
    """schro_dequantise (schroutils.c:179-189)"""
    q = np.asarray(q, np.int64)
    r = (np.abs(q) * factor + offset + 2) >> 2
    return np.where(q == 0, 0, np.where(q < 0, -r, r))


def bit_length_vec(v):
    """bit length of positive int64 values below 2^53"""
    return np.frexp(np.asarray(v, np.float64))[1].astype(np.int64)


def estimate_sint_vec(q):
    """schro_pack_estimate_sint (schropack.c:214-226)"""
    mag = np.abs(np.asarray(q, np.int64))
    n = bit_length_vec(mag + 1)
    return 2 * n - 1 + (mag != 0)


def sint_codes(q):
    """schro_pack_encode_sint: (code right-aligned, length) per value"""
    q = np.asarray(q, np.int64)
    mag = np.abs(q)
    v = mag + 1
    n = bit_length_vec(v)
    d = v - (1 << (n - 1))                      # the n - 1 bits under the leading one, each sent as "0 b"
    d = (d | (d << 8)) & 0x00ff00ff
    d = (d | (d << 4)) & 0x0f0f0f0f
    d = (d | (d << 2)) & 0x33333333
    d = (d | (d << 1)) & 0x55555555
    code = np.where(mag == 0, 1, (d << 2) | 2 | (q < 0))
    return code, np.where(mag == 0, 1, 2 * n)


def bits_of(code, length):
    """the codes one behind the other, MSB first: a uint8 array of bits"""
    code, length = np.asarray(code, np.int64), np.asarray(length, np.int64)
    total = int(length.sum())
    if total == 0:
        return np.zeros(0, np.uint8)
    which = np.repeat(np.arange(code.size), length)
    j = np.arange(total) - np.repeat(np.cumsum(length) - length, length)
    return ((code[which] >> (length[which] - 1 - j)) & 1).astype(np.uint8)


def dc_predict(rec, x, y):
    """schro_dc_predict (schrolowdelay.c:765-783) on the reconstructed band (int16 values as Python ints)"""
    if y > 0:
        if x > 0:
            return ((int(rec[y, x - 1]) + int(rec[y - 1, x]) + int(rec[y - 1, x - 1]) + 1) * 21845 + 10922) >> 16
        return int(rec[y - 1, x])
    return int(rec[y, x - 1]) if x > 0 else 0


def subband(plane, index, depth, w_iwt, h_iwt):
    """schro_subband_get_frame_data (schroparams.c:319-352) as a writable view of the interleaved coefficient plane"""
    position = 0 if index == 0 else ((index - 1) // 3 + 1) * 4 - 3 + (index - 1) % 3
    shift = depth - (position >> 2)
    w, h = w_iwt >> shift, h_iwt >> shift
    row0 = (1 << shift) >> 1 if position & 2 else 0
    col0 = w if position & 1 else 0
    return plane[row0::1 << shift, col0:col0 + w][:h]


def codeblock(w, h, x, y, nh, nv):
    """schro_frame_data_get_codeblock (schroframe.c:1865-1884): xmin, xmax, ymin, ymax"""
    return (w * x) // nh, (w * (x + 1)) // nh, (h * y) // nv, (h * (y + 1)) // nv


def slice_sizes(P):
    """schrolowdelay.c:1171-1190: the bytes of every slice, raster order"""
    n_bytes, remainder = P["slice_bytes_num"] // P["slice_bytes_denom"], P["slice_bytes_num"] % P["slice_bytes_denom"]
    acc, out = 0, []
    for _ in range(P["n_horiz_slices"] * P["n_vert_slices"]):
        acc += remainder
        extra = 0
        if acc >= P["slice_bytes_denom"]:
            extra = 1
            acc -= P["slice_bytes_denom"]
        out.append(n_bytes + extra)
    return out


class _Slice:
    """One slice: its samples in coding order, and the reference's state around it."""

    def __init__(self, enc, sx, sy, slice_bytes):
        self.enc, self.sx, self.sy, self.slice_bytes = enc, sx, sy, slice_bytes
        P = enc.P
        self.hi, self.band, self.where = [], [], []
        for c in range(3):
            vals, band, where = [], [], []
            for i in range(1, enc.nsub):
                b = enc.bands[c][i]
                x0, x1, y0, y1 = codeblock(b.shape[1], b.shape[0], sx, sy, P["n_horiz_slices"], P["n_vert_slices"])
                block = b[y0:y1, x0:x1]
                vals.append(block.reshape(-1).astype(np.int64))
                band.append(np.full(block.size, i, np.int64))
                where.append((i, x0, x1, y0, y1))
            self.hi.append(np.concatenate(vals) if vals else np.zeros(0, np.int64))
            self.band.append(np.concatenate(band) if band else np.zeros(0, np.int64))
            self.where.append(where)
        self.ll = []
        for c in range(3):
            b = enc.bands[c][0]
            self.ll.append(codeblock(b.shape[1], b.shape[0], sx, sy, P["n_horiz_slices"], P["n_vert_slices"]))

    def _ll(self, c, qi):
        """quantise_dc_block (:874-904): the block's quantised values; the reconstruction is left in enc.recon[c]"""
        enc = self.enc
        factor, offset = int(enc.factor[qi]), int(enc.offset[qi])
        x0, x1, y0, y1 = self.ll[c]
        src, rec, out = enc.bands[c][0], enc.recon[c], []
        for y in range(y0, y1):
            for x in range(x0, x1):
                pred = dc_predict(rec, x, y)
                q = w16(Q.schro_quantise(int(src[y, x]) - pred, factor, offset))       # stored as int16_t
                rec[y, x] = w16(pred + Q.schro_dequantise(q, factor, offset))
                out.append(q)
        return np.array(out, np.int64)

    def quantised(self, base_index):
        """The three components' quant_data at base_index, coding order (LL first)."""
        enc = self.enc
        out = []
        for c in range(3):
            qi = np.clip(base_index - enc.qm[self.band[c]], 0, 60)             # :965, :1010
            hi = w16(quantise_vec(self.hi[c], enc.factor[qi], enc.offset[qi]))
            ll = self._ll(c, int(np.clip(base_index - enc.qm[0], 0, 60)))
            out.append(np.concatenate([ll, hi]))
        return out

    def estimate(self, base_index):
        """schro_encoder_estimate_slice (:927-1062): (n_bits, state for write ())"""
        y, u, v = self.quantised(base_index)
        n_bits = 7 + ilog2up(8 * self.slice_bytes)
        y_bits = int(estimate_sint_vec(y).sum())
        nz = np.flatnonzero(y)
        y_tz = y.size - 1 - int(nz[-1]) if nz.size else y.size                  # :992-996
        uv_bits = int(estimate_sint_vec(u).sum() + estimate_sint_vec(v).sum())
        nz = np.flatnonzero((u != 0) | (v != 0))
        uv_tz = 2 * (u.size - 1 - int(nz[-1]) if nz.size else u.size)           # :1052-1058
        state = dict(base_index=base_index, y=y, u=u, v=v, y_bits=y_bits, y_tz=y_tz, uv_tz=uv_tz)
        return n_bits + y_bits + uv_bits - y_tz - uv_tz, state

    def write(self, st):
        """schro_encoder_encode_slice (:785-839): (bytes, over-run, the bits written before the padding or the cut)"""
        length_bits = ilog2up(8 * self.slice_bytes)
        y_length = st["y_bits"] - st["y_tz"]
        head = bits_of([st["base_index"], y_length & ((1 << length_bits) - 1)], [7, length_bits])
        ny, nuv = st["y"].size - st["y_tz"], st["u"].size - st["uv_tz"] // 2
        uv = np.empty(2 * nuv, np.int64)
        uv[0::2], uv[1::2] = st["u"][:nuv], st["v"][:nuv]
        bits = np.concatenate([head, bits_of(*sint_codes(st["y"][:ny])), bits_of(*sint_codes(uv))])
        room, written = 8 * self.slice_bytes, bits.size
        overrun = written > room
        if overrun:
            bits = bits[:room]                  # (the reference asserts, :826-830)
        else:
            bits = np.concatenate([bits, np.ones(room - bits.size, np.uint8)])
        return np.packbits(bits), overrun, written

    def dequantise_high(self, st):
        """schro_encoder_dequantise_slice (:1064-1114) into the encoder's reconstruction (not into the input)"""
        enc = self.enc
        for c, key in enumerate("yuv"):
            qi = np.clip(st["base_index"] - enc.qm[self.band[c]], 0, 60)
            nll = (self.ll[c][1] - self.ll[c][0]) * (self.ll[c][3] - self.ll[c][2])
            deq = dequantise_vec(st[key][nll:], enc.factor[qi], enc.offset[qi])
            at = 0
            for (i, x0, x1, y0, y1) in self.where[c]:
                n = (x1 - x0) * (y1 - y0)
                enc.rec_bands[c][i][y0:y1, x0:x1] = w16(deq[at:at + n]).reshape(y1 - y0, x1 - x0)
                at += n


class _Encoder:
    def __init__(self, planes, P):
        self.P = P
        self.depth = P["transform_depth"]
        self.nsub = 1 + 3 * self.depth
        self.factor, self.offset = _tables()
        self.qm = np.array(list(P["quant_matrix"])[:self.nsub], np.int64)
        sizes = [(P["iwt_luma_width"], P["iwt_luma_height"])] + [(P["iwt_chroma_width"], P["iwt_chroma_height"])] * 2
        self.planes = [np.ascontiguousarray(p[:h, :w], dtype=np.int16) for p, (w, h) in zip(planes, sizes)]
        self.rec_planes = [np.zeros_like(p) for p in self.planes]
        self.bands = [[subband(p, i, self.depth, w, h) for i in range(self.nsub)] for p, (w, h) in zip(self.planes, sizes)]
        self.rec_bands = [[subband(p, i, self.depth, w, h) for i in range(self.nsub)]
                          for p, (w, h) in zip(self.rec_planes, sizes)]
        # lowdelay.reconstructed_frame (:1164-1166): here the LL bands of the reconstruction itself (int16)
        self.recon = [b[0] for b in self.rec_bands]


def _pick(sl, trace=None):
    """schro_encoder_pick_slice_index (:1116-1148): the state of the final estimate"""
    room = sl.slice_bytes * 8
    n, st = sl.estimate(0)
    if trace is not None:
        trace.append((0, n))
    if n <= room:
        return st
    i, size = 0, 32
    while size >= 1:
        n, _ = sl.estimate(i + size)
        if trace is not None:
            trace.append((i + size, n))
        if n >= room:
            i += size
        size >>= 1
    n, st = sl.estimate(i + 1)
    if trace is not None:
        trace.append((i + 1, n))
    return st


def encode(planes, P, traces=None):
    """planes: the Y, U, V coefficient planes (int16, at least the iwt sizes).  Returns a dict: `bytes` (uint8, what the
    reference appends to frame->pack), `index` (uint8 per slice), `overrun` (bool per slice), `count` (their number), `used`
    (the bits the writer put into every slice before the padding or the cut, counted from what it wrote) and `recon` --
    the encoder's reconstruction, three int16 planes: high bands dequantised, LL as reconstructed.  traces: a list that receives per slice its probes [(index, estimate)]."""
    enc = _Encoder(planes, P)
    nh, nv = P["n_horiz_slices"], P["n_vert_slices"]
    sizes = slice_sizes(P)
    out, index, overrun, used = [], [], [], []
    for s, slice_bytes in enumerate(sizes):
        sl = _Slice(enc, s % nh, s // nh, slice_bytes)
        trace = [] if traces is not None else None
        st = _pick(sl, trace)
        if traces is not None:
            traces.append(trace)
        data, over, written = sl.write(st)
        sl.dequantise_high(st)
        out.append(data)
        index.append(st["base_index"])
        overrun.append(over)
        used.append(written)
    data = np.concatenate(out) if out else np.zeros(0, np.uint8)
    assert data.size == (P["slice_bytes_num"] * nh * nv) // P["slice_bytes_denom"]
    return dict(bytes=data, index=np.array(index, np.uint8), overrun=np.array(overrun, bool), count=int(np.sum(overrun)),
                used=np.array(used, np.int64), recon=enc.rec_planes)
