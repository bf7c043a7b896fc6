"""The reference encoder's quantisation arithmetic restated in numpy (checker only).

  quantise_s16        schro_frame_data_quantise on an s16 codeblock, schroencoder.c:3485-3553: one of four 16-bit Orc
                      programs by quant index -- copy (index 0), orc_quantdequant2_s16 (multiples of 4),
                      orc_quantdequant3_s16 (index 3), orc_quantdequant1_s16 (the rest; quant_offset-- above index 8);
                      bodies schroorc-dist.c:10746, :10929, :11131.  Every step wraps at 16 bits.
  quantise_s32        schro_quantise_s32, schroutils.c:248-257: C int arithmetic, truncating division (|x| < 2^28)
  schro_quantise / schro_dequantise   schroutils.c:179-235 taken literally (Python ints wrapped to 32 bits)
  quantise_dc         schro_frame_data_quantise_dc_predict, schroencoder.c:3591-3667, as ONE raster-order recurrence
                      over the band: a codeblock never reads its right neighbour, so the codeblock loop of
                      schro_encoder_quantise_subband (:3754-3782) visits every sample after its left, upper and
                      upper-left neighbours exactly as the raster order does; each sample takes its own codeblock's index
  quantise_plane      the records of one plane (SchroHipCodeblock geometry), quantised values, reconstruction, summaries
  subtract            orc_subtract_s16 / orc_subtract_s16_u8 (schroorc-dist.c:3639, :4625): 16-bit wrapping dst - src

The four tables are the reference's numbers (tests/golden/quant_tables_encoder.json).

tests/test_quant_ref.py pins quantise_s16 on the reference's compiled kernels: for every index 0 .. 60, intra and
inter, all 65 536 s16 values through the program schro_frame_data_quantise would pick, with its arguments
(tests/golden/quant_ref_digests.json, recorded by tests/golden/make_quant_golden.py from oracle/_ref; where oracle/_ref
is built the kernels themselves are run as well).  `subtract` is pinned the same way.

What stays UNPINNED: schro_frame_data_quantise_dc_predict is static in schroencoder.c, which cannot be compiled here
(the full library needs liborc), and schro_quantise_s32 lives in schroutils.c, the same.  quantise_dc and quantise_s32
rest on this restatement of their C text, on the round trip through the decoder's dequantisation (oracle_lib, pinned
on the reference decoder) and, on the device, through schro_hip_dequant_batch + schro_hip_dc_predict_batch."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLES_PATH = os.path.join(HERE, "golden", "quant_tables_encoder.json")
_TABLES = None


def tables():
    """{name: [61 ints]} for schro_table_quant, _offset_1_2, _offset_3_8, _inverse_quant."""
    global _TABLES
    if _TABLES is None:
        _TABLES = json.load(open(TABLES_PATH))
    return _TABLES


def quant_factor(qi):
    return tables()["schro_table_quant"][qi]


def quant_offset(qi, is_intra):
    return tables()["schro_table_offset_1_2" if is_intra else "schro_table_offset_3_8"][qi]


def _w16(v):
    """wrap to int16 (array of int64 or a Python int)"""
    return ((v + 32768) & 0xffff) - 32768


def _w32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


def program_for(qi, is_intra):
    """(name, arguments) of the Orc program schro_frame_data_quantise runs on an s16 codeblock, the arguments as it
    passes them (ints, before loadpw truncates them); name None: the copy of index 0."""
    t = tables()
    factor, inv = t["schro_table_quant"][qi], t["schro_table_inverse_quant"][qi]
    real = quant_offset(qi, is_intra)
    shift = (qi >> 2) + 2
    off = real - (factor >> 1)
    if qi == 0:
        return None, ()
    if (qi & 3) == 0:
        return "orc_quantdequant2_s16", (shift, off, factor, real + 2)
    if qi == 3:
        return "orc_quantdequant3_s16", (inv, off, shift + 16, factor, real + 2, 32768)
    if qi > 8:
        off -= 1
    return "orc_quantdequant1_s16", (inv, off, shift, factor, real + 2)


def _tail(e, sign, factor, offs2):
    """the common end of the three programs from the unsigned quotient e: (q, reconstruction)"""
    q = _w16(e * sign)
    s2 = np.clip(q, -1, 1)
    f = _w16(e * _w16(factor))
    g = _w16(f + _w16(offs2))
    return q, _w16((g >> 2) * s2)


def _head(x, off):
    x = np.asarray(x).astype(np.int64)
    sign = np.clip(x, -1, 1)
    a = _w16(np.abs(x))                         # absw: -32768 stays
    b = _w16(a << 2)
    return sign, _w16(b - _w16(off)) & 0xffff   # as mulhuw / shruw see it


def quantdequant1_s16(x, p1, p2, p3, p4, p5):
    sign, c = _head(x, p2)
    d = (c * (_w16(p1) & 0xffff)) >> 16
    return _tail(_w16(d >> p3), sign, p4, p5)


def quantdequant2_s16(x, p1, p2, p3, p4):
    sign, c = _head(x, p2)
    return _tail(_w16(c >> p1), sign, p3, p4)


def quantdequant3_s16(x, p1, p2, p3, p4, p5, p6):
    sign, c = _head(x, p2)
    m = (c * (_w16(p1) & 0xffff) + p6) & 0xffffffff      # muluwl, addl; shrul sees 32 unsigned bits
    return _tail(_w16(m >> p3), sign, p4, p5)


_PROGRAMS = {"orc_quantdequant1_s16": quantdequant1_s16, "orc_quantdequant2_s16": quantdequant2_s16,
             "orc_quantdequant3_s16": quantdequant3_s16}


def quantise_s16(x, qi, is_intra):
    """(quantised, reconstructed), both int16, of an s16 array."""
    name, args = program_for(qi, is_intra)
    x = np.asarray(x, np.int16)
    if name is None:
        return x.copy(), x.copy()
    q, r = _PROGRAMS[name](x, *args)
    return q.astype(np.int16), r.astype(np.int16)


def quantise_s16_orc(x, qi, is_intra):
    """quantise_s16 by the reference's compiled program (oracle/_ref), called with schro_frame_data_quantise's arguments"""
    import oracle_lib as O
    name, args = program_for(qi, is_intra)
    r = np.ascontiguousarray(x, np.int16).copy().reshape(-1)
    if name is None:                # orc_memcpy: the coefficients stay
        return r.copy().reshape(np.shape(x)), r.reshape(np.shape(x))
    q = np.zeros_like(r)
    getattr(O.reforc(), name)(q.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                              *[C.c_int(a) for a in args], C.c_int(r.size))
    return q.reshape(np.shape(x)), r.reshape(np.shape(x))


def subtract_orc(dst, src):
    """one row of orc_subtract_s16 / orc_subtract_s16_u8 (oracle/_ref)"""
    import oracle_lib as O
    d, s = np.ascontiguousarray(dst, np.int16), np.ascontiguousarray(src)
    assert d.ndim == 1 and d.shape == s.shape and s.dtype in (np.int16, np.uint8)
    f = O.reforc().orc_subtract_s16_u8 if s.dtype == np.uint8 else O.reforc().orc_subtract_s16
    out = np.zeros_like(d)
    f(out.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), C.c_int(d.size))
    return out


def all_s16():
    return np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)


def subtract_pin_inputs(u8):
    """the seeded rows the subtract digests were recorded on"""
    rng = np.random.default_rng(31 + u8)
    d = rng.integers(-32768, 32768, 4096).astype(np.int16)
    s = rng.integers(0, 256, 4096).astype(np.uint8) if u8 else rng.integers(-32768, 32768, 4096).astype(np.int16)
    return d, s


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def schro_quantise(value, factor, offset):
    """schroutils.c:197-230 on Python ints, every int expression wrapped to 32 bits"""
    if value == 0:
        return 0
    x = _w32(abs(value) << 2) if value != -(1 << 31) else 0
    if x < offset:
        x = 0
    else:
        n = _w32(x - (offset - factor // 2))
        x = abs(n) // factor * (1 if n >= 0 else -1)         # C division truncates
    return -x if value < 0 else x


def schro_dequantise(q, factor, offset):
    """schroutils.c:179-189"""
    if q == 0:
        return 0
    if q < 0:
        return _w32(-(_w32(_w32(-q * factor) + offset + 2) >> 2))
    return _w32(_w32(q * factor) + offset + 2) >> 2


def quantise_s32(x, qi, is_intra):
    """(quantised, reconstructed), both int32: schro_quantise_s32 vectorised (the contract: |x| < 2^28)."""
    factor, offset = quant_factor(qi), quant_offset(qi, is_intra)
    v = np.asarray(x).astype(np.int64)
    mag = _w32(np.abs(v) << 2)
    n = _w32(mag - (offset - factor // 2))
    quo = np.where(n >= 0, np.abs(n) // factor, -(np.abs(n) // factor))
    qm = np.where(mag < offset, 0, quo)
    q = np.where(v < 0, -qm, qm)
    q = np.where(v == 0, 0, q)
    d = _w32(_w32(np.abs(q) * factor) + offset + 2) >> 2
    r = np.where(q < 0, _w32(-d), d)
    r = np.where(q == 0, 0, r)
    return _w32(q).astype(np.int32), r.astype(np.int32)


def quantise_codeblock(x, qi, is_intra):
    x = np.asarray(x)
    return quantise_s16(x, qi, is_intra) if x.dtype == np.int16 else quantise_s32(x, qi, is_intra)


def quantise_dc(band, qi_map, is_intra=True):
    """The intra LL band: band h x w (int16 / int32), qi_map h x w the quant index of each sample's codeblock.
    Returns (quantised, reconstructed) of the band's dtype."""
    band = np.asarray(band)
    s16 = band.dtype == np.int16
    h, w = band.shape
    line = [[int(v) for v in row] for row in band]
    quant = [[0] * w for _ in range(h)]
    t = tables()
    fac, off = t["schro_table_quant"], t["schro_table_offset_1_2" if is_intra else "schro_table_offset_3_8"]
    wrap = _w16 if s16 else _w32
    truncated = 0
    for j in range(h):
        cur, up, qrow, qi_row = line[j], line[j - 1] if j else None, quant[j], qi_map[j]
        for i in range(w):
            if j > 0:
                if i > 0:
                    a = cur[i - 1] + up[i] + up[i - 1] + 1
                    pred = ((a * 21845 + 10922) >> 16) if s16 else a // 3       # schro_divide3 / schro_divide (a, 3)
                else:
                    pred = up[i]
            else:
                pred = cur[i - 1] if i > 0 else 0
            qi = int(qi_row[i])
            q = schro_quantise(_w32(cur[i] - pred), fac[qi], off[qi])
            r = _w32(schro_dequantise(q, fac[qi], off[qi]) + pred)
            cur[i], qrow[i] = wrap(r), wrap(q)
            truncated += cur[i] != r or qrow[i] != q
    quantise_dc.truncated = truncated           # (stores that did not hold the value: the tests want to know their case has some)
    return np.array(quant, band.dtype).reshape(h, w), np.array(line, band.dtype).reshape(h, w)


def _cells(rec, itemsize, shape):
    """flat sample indices (h x w) of a record (dst_offset, dst_stride, width, height, quant_index) in a plane buffer"""
    off, stride, w, h = rec[:4]
    assert off % itemsize == 0 and stride % itemsize == 0
    idx = off // itemsize + np.arange(h)[:, None] * (stride // itemsize) + np.arange(w)[None, :]
    assert idx.size == 0 or idx.max() < shape
    return idx


def summary_of(q):
    """(nonzero, max_abs) of a codeblock's quantised values"""
    a = np.abs(np.asarray(q).astype(np.int64))
    return int(np.count_nonzero(a)), int(a.max()) if a.size else 0


def quantise_plane(coeffs, records, is_intra, dc_first=0, dc_size=None):
    """coeffs: the plane's buffer, a 2-D C-contiguous array whose row pitch is the frame stride (padding included);
    records: (dst_offset, dst_stride, width, height, quant_index) each, offsets in bytes from the buffer's start.
    dc_first > 0: the first dc_first records tile the dc_size = (width, height) band at the buffer's start (pitch = their
    dst_stride) and are quantised with DC prediction.  Returns (quant, recon, [(nonzero, max_abs)]): quant holds zero
    outside the records, recon the coefficients there."""
    coeffs = np.ascontiguousarray(coeffs)
    flat = coeffs.reshape(-1)
    quant, recon = np.zeros_like(flat), flat.copy()
    isz = coeffs.dtype.itemsize
    summ = [None] * len(records)
    if dc_first:
        bw, bh = dc_size
        pitch = records[0][1] // isz
        bidx = np.arange(bh)[:, None] * pitch + np.arange(bw)[None, :]
        qi_map = np.full((bh, bw), -1, np.int64)
        for rec in records[:dc_first]:
            assert rec[1] == records[0][1]
            y, x = divmod(rec[0] // isz, pitch)
            assert x + rec[2] <= bw and y + rec[3] <= bh
            qi_map[y:y + rec[3], x:x + rec[2]] = rec[4]
        assert (qi_map >= 0).all(), "the DC records do not cover the band"
        q, r = quantise_dc(flat[bidx], qi_map, is_intra)
        quant[bidx], recon[bidx] = q, r
        for n, rec in enumerate(records[:dc_first]):
            summ[n] = summary_of(quant[_cells(rec, isz, flat.size)])
    for n, rec in enumerate(records):
        if n < dc_first:
            continue
        idx = _cells(rec, isz, flat.size)
        q, r = quantise_codeblock(flat[idx], rec[4], is_intra)
        quant[idx], recon[idx] = q, r
        summ[n] = summary_of(q)
    return quant.reshape(coeffs.shape), recon.reshape(coeffs.shape), summ


def subtract(dst, src):
    """dst (s16) - src (s16 | u8 zero-extended) over the common size, 16-bit wrap; the rest of dst unchanged."""
    d = np.ascontiguousarray(dst, np.int16).copy()
    s = np.asarray(src)
    assert s.dtype in (np.int16, np.uint8)
    h, w = min(d.shape[0], s.shape[0]), min(d.shape[1], s.shape[1])
    d[:h, :w] = _w16(d[:h, :w].astype(np.int64) - s[:h, :w].astype(np.int64)).astype(np.int16)
    return d
