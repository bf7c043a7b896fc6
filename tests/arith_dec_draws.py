"""Drawn pictures and hostile byte strings for schro_hip_arith_decode_batch.  TEST INFRASTRUCTURE.

The reference stream has one geometry (320 x 240 4:2:0 s16, depth 4, one codeblock in the coarse bands, every quant offset
0).  What it lacks is drawn here at the smallest shapes where the kernel can go wrong and written by
arith_dec_ref.write_transform_data; the expected planes and result are arith_dec_ref.decode_transform_data's.  Each draw
names its WITNESS -- the trap it is meant to hit -- and tests/test_arith_dec_draws.py asserts it without a device."""
import functools

import numpy as np

import arith_dec_ref as AR
import noarith_enc_ref as enc

CLEAN = dict(error=0, truncated=0, not_consumed=0, overran=0, long_codes=0, clamped_quant=0)


class Case:
    """One picture of a call.  sizes: (width, height) per component at the transform's size."""

    def __init__(self, name, dtype, sizes, depth, hc, vc, mode, compat, is_intra, data, data_bytes=None, witness=None, clean=True):
        self.name, self.dtype, self.sizes, self.depth = name, np.dtype(dtype), [tuple(s) for s in sizes], depth
        self.hc, self.vc, self.mode, self.compat, self.is_intra = list(hc), list(vc), mode, compat, is_intra
        self.data = bytes(data)
        self.data_bytes = len(self.data) if data_bytes is None else data_bytes
        self.witness, self.clean = witness, clean
        self._expected = None

    def expected(self, nbytes=None):
        """(coefficient planes, quant planes, result dict) of the restatement over the first `nbytes` (data_bytes) bytes;
        the planes are None for a picture with the error.  Computed once, never changed."""
        if nbytes is None and self._expected is not None:
            return self._expected
        n = self.data_bytes if nbytes is None else nbytes
        coeffs = [np.full((h, w), 0x5b, self.dtype) for w, h in self.sizes]
        quant = [np.full((h, w), 0x5c, self.dtype) for w, h in self.sizes]
        result = AR.decode_transform_data(self.data[:n], coeffs, quant, self.depth, self.hc, self.vc, self.mode, self.is_intra, self.compat)
        out = (None, None, result) if result["error"] else (coeffs, quant, result)
        if nbytes is None:
            self._expected = out
        return out


def chroma(w, h, fmt):
    return {444: (w, h), 422: (w // 2, h), 420: (w // 2, h // 2)}[fmt]


def sizes_of(w, h, fmt):
    return [(w, h), chroma(w, h, fmt), chroma(w, h, fmt)]


def fill(rng, sizes, depth, amplitude=6, zeros=0.5):
    """Quantised planes: sparse small values, larger and denser in the coarse bands."""
    planes = []
    for w, h in sizes:
        p = np.zeros((h, w), np.int64)
        for i in range(1 + 3 * depth):
            b = enc.subband(p, depth, i)
            level = 0 if i == 0 else (i - 1) // 3 + 1
            amp = max(1, amplitude * (depth + 1 - level))
            v = rng.integers(-amp, amp + 1, b.shape)
            b[...] = np.where(rng.random(b.shape) < min(0.9, zeros + 0.08 * level), 0, v)
        planes.append(p)
    return planes


def drawn(name, dtype, w, h, fmt, depth, hc, vc, mode, compat, is_intra, seed, qidx=None, offsets=None, edit=None, witness=None,
          clean=True, **kw):
    rng = np.random.default_rng(seed)
    sizes = sizes_of(w, h, fmt)
    planes = fill(rng, sizes, depth, **kw)
    if edit:
        planes = edit(planes) or planes
    nsub = 1 + 3 * depth
    qidx = qidx or [[(5 + 3 * k + 2 * i) % 24 for i in range(nsub)] for k in range(3)]
    data, stored, used, after = AR.write_transform_data(planes, depth, hc, vc, mode, compat, qidx, is_intra, offsets=offsets, dtype=dtype,
                                                        clean=clean)
    case = Case(name, dtype, sizes, depth, hc, vc, mode, compat, is_intra, data, witness=witness, clean=clean)
    case.planes, case.stored, case.used, case.compat_after, case.qidx = planes, stored, used, after, qidx
    return case


# ---- the edits and witnesses ----------------------------------------------------------------------------------------------

def zero_parents(planes):
    """Luma: sub-band 1 all zero (a zero-LENGTH parent of sub-band 4), the first codeblock of sub-band 2 zero (a zero
    CODEBLOCK as the parent of sub-band 5's first values and as the left / up neighbour of sub-band 2's other codeblocks),
    and their children dense."""
    p = planes[0]
    enc.subband(p, 2, 1)[...] = 0
    b2 = enc.subband(p, 2, 2)
    enc.get_codeblock(b2, 0, 0, 2, 2)[...] = 0
    enc.get_codeblock(b2, 1, 0, 2, 2)[...] = 3
    enc.get_codeblock(b2, 0, 1, 2, 2)[...] = -2
    enc.subband(p, 2, 4)[...] = 2
    enc.subband(p, 2, 5)[...] = -1


def witness_zero_parents(case):
    assert (0, 1) not in case.used and (0, 4) in case.used
    assert case.used[0, 2][0, 0] == -1 and (case.used[0, 2].ravel()[1:] >= 0).all()
    assert not enc.subband(case.stored[0], 2, 1).any() and enc.subband(case.stored[0], 2, 4).all()


def multiple_of_65536(planes):
    """Luma sub-band 0 at quant index 0 (factor 4, intra offset 1: the value is stored as it is read): 65536 and 131072 in
    front of small values.  On s16 both are STORED as 0, so the values behind them see a zero neighbourhood."""
    b = enc.subband(planes[0], 1, 0)
    b[...] = 0
    b[0, 0], b[0, 1], b[0, 2] = 65536, 1, -131072
    b[1, 1] = 2
    v = enc.subband(planes[0], 1, 1)        # the vertically oriented band: the sign context is the upper value's
    v[...] = 0
    v[0, 0], v[1, 0] = -65536, 5


def witness_multiple_of_65536(case):
    ll = enc.subband(case.stored[0], 1, 0)
    assert case.dtype == np.int16 and case.qidx[0][0] == 0 and case.qidx[0][1] == 0
    assert ll[0, 0] == 0 and ll[0, 1] == 1 and ll[0, 2] == 0 and enc.subband(case.planes[0], 1, 0)[0, 0] == 65536
    # the same values on s32 planes are stored as read, and the context of (0, 1) differs: the bytes differ
    again = AR.write_transform_data(case.planes, case.depth, case.hc, case.vc, case.mode, case.compat, case.qidx, case.is_intra, dtype=np.int32)
    assert enc.subband(again[1][0], 1, 0)[0, 0] == 65536 and again[0] != case.data


def offsets_wild(k, i, x, y):
    """Carried from codeblock to codeblock and clamped at both ends."""
    return [0, 70, -3, -90, 5, 64, -61, 2, -1][(x + 3 * y + i + k) % 9]


def witness_offsets(case):
    r = case.expected()[2]
    qis = np.concatenate([u.ravel() for u in case.used.values()])
    assert r["clamped_quant"] > 4 and 0 in qis and 60 in qis and len(set(qis.tolist())) > 6 and case.hc[0] * case.vc[0] > 1


def witness_compat(case):
    r = case.expected()[2]
    assert case.compat == 0 and case.compat_after == 1 == r["compat_quant_offset"] and case.mode == 1
    assert case.hc == [1] * len(case.hc) and all((k, 0) in case.used for k in range(3))
    # in state 1 from the start the same bytes decode to the same planes; in state 0 WITHOUT the switch they could not:
    # components 1 and 2 would read an offset
    again = Case(case.name, case.dtype, case.sizes, case.depth, case.hc, case.vc, 1, 1, case.is_intra, case.data).expected()
    assert all(np.array_equal(a, b) for a, b in zip(again[0], case.expected()[0]))


def big_first(planes):
    for p in planes:
        enc.subband(p, 2, 0)[0, 0] = 1 << 20


def witness_narrow(case):
    assert enc.subband(case.planes[0], 1, 1).shape == (1, 5) and case.hc == [3, 3]
    assert [AR.rectangle(5, 1, 3, 1, x, 0)[2] - AR.rectangle(5, 1, 3, 1, x, 0)[0] for x in range(3)] == [1, 2, 2]


def witness_deep(case):
    assert case.depth == 6 and enc.subband(case.planes[0], 6, 0).shape == (1, 1)
    assert sum((0, i) in case.used for i in range(19)) >= 15         # parents through the levels


def witness_none(case):
    pass


@functools.lru_cache(maxsize=None)
def draws():
    D = []
    D.append(drawn("d0-2x2", np.int16, 2, 2, 444, 0, [1], [1], 0, 0, 1, 1, zeros=0.1, witness=witness_none))
    D.append(drawn("d1-2x2", np.int16, 2, 2, 444, 1, [1, 1], [1, 1], 1, 1, 0, 2, zeros=0.1, witness=witness_none))
    D.append(drawn("d6-64-s16", np.int16, 64, 64, 444, 6, [1, 1, 1, 1, 2, 2, 3], [1, 1, 1, 1, 1, 2, 2], 1, 1, 1, 3, witness=witness_deep))
    D.append(drawn("d6-64-s32", np.int32, 64, 64, 444, 6, [1, 1, 1, 1, 2, 2, 3], [1, 1, 1, 1, 1, 2, 2], 0, 0, 0, 4, amplitude=4000,
                   witness=witness_deep))
    D.append(drawn("narrow-5x1", np.int16, 10, 2, 444, 1, [3, 3], [1, 1], 0, 0, 0, 5, zeros=0.2, witness=witness_narrow))
    D.append(drawn("offsets-420", np.int16, 32, 16, 420, 2, [2, 3, 2], [2, 1, 3], 1, 0, 0, 6, offsets=offsets_wild, witness=witness_offsets))
    D.append(drawn("offsets-422-s32", np.int32, 32, 16, 422, 2, [3, 2, 2], [1, 2, 2], 1, 1, 1, 7, offsets=offsets_wild, amplitude=300,
                   witness=witness_offsets))
    D.append(drawn("zero-parents", np.int16, 16, 16, 444, 2, [1, 2, 2], [1, 2, 2], 0, 0, 0, 8, edit=zero_parents, witness=witness_zero_parents))
    D.append(drawn("65536-s16", np.int16, 8, 4, 444, 1, [1, 1], [1, 1], 0, 0, 1, 9, qidx=[[0, 0, 3, 3]] * 3, edit=multiple_of_65536,
                   witness=witness_multiple_of_65536))
    # the compat peek: sub-band 0's first value is large, so that the sint the decoder peeks leaves 0 .. 60
    D.append(drawn("compat-on", np.int16, 16, 8, 420, 2, [1, 1, 1], [1, 1, 1], 1, 0, 0, 10, qidx=[[40 + i for i in range(7)]] * 3,
                   edit=big_first, witness=witness_compat))
    return D


# ---- hostile ---------------------------------------------------------------------------------------------------------------

def header(length, qi):
    pack = enc.Pack()
    pack.encode_uint(length)
    if length:
        pack.encode_uint(qi)
    pack.sync()
    return bytes(pack.data)


def picture_of(payloads, qi=12):
    """Transform data whose coded sub-bands are `payloads` (None: length 0), in stream order."""
    return b"".join(header(len(p), qi) + p if p else header(0, 0) for p in payloads)


def long_code(planes):
    """33 and 31 data bins: bits wraps, (int) (bits - 1) is 5 and INT_MIN."""
    b = enc.subband(planes[0], 1, 0)
    b[...] = 0
    b[0, 1], b[1, 0], b[1, 1] = (1 << 33) + 5, -(1 << 31), 3


@functools.lru_cache(maxsize=None)
def hostile():
    H = []
    sizes, depth, one = sizes_of(16, 8, 420), 1, [1, 1]
    base = drawn("base", np.int16, 16, 8, 420, 1, [2, 1], [1, 2], 1, 0, 0, 20)
    n = len(base.data)
    H.append(Case("cut-middle", np.int16, sizes, depth, base.hc, base.vc, 1, 0, 0, base.data, n // 2, clean=False))
    H.append(Case("cut-in-first-header", np.int16, sizes, depth, base.hc, base.vc, 1, 0, 0, base.data, 1, clean=False))
    H.append(Case("empty", np.int16, sizes, depth, base.hc, base.vc, 1, 0, 0, b"", clean=False))
    H.append(Case("length-past-input", np.int32, sizes, depth, one, one, 0, 0, 1, header(4000, 7) + b"\x5a\x00\xc3", clean=False))
    H.append(Case("zeros-64", np.int16, sizes, depth, one, one, 0, 0, 0, picture_of([bytes(64)] + [None] * 11), clean=False))
    H.append(Case("zeros-64-mode1-s32", np.int32, sizes, depth, [2, 2], [2, 2], 1, 0, 0, picture_of([None, bytes(64)] * 6), clean=False))
    H.append(Case("ff-payloads", np.int16, sizes, depth, [2, 1], [1, 2], 1, 0, 1, picture_of([b"\xff" * 9] * 12), clean=False))
    H.append(Case("random-payloads", np.int16, sizes, depth, [2, 2], [1, 2], 1, 0, 0,
                  picture_of([np.random.default_rng(30 + i).integers(0, 256, 5 + 3 * i, dtype=np.uint8).tobytes() for i in range(12)]), clean=False))
    for dtype in (np.int16, np.int32):
        H.append(drawn("long-codes-" + np.dtype(dtype).name, dtype, 16, 8, 420, 1, one, one, 0, 0, 0, 21, qidx=[[60, 59, 58, 57]] * 3,
                       edit=long_code, clean=False))
    H.append(Case("index-61", np.int16, sizes, depth, one, one, 1, 1, 0, base.data[:0] + header(3, 12) + b"abc" + header(2, 61) + b"xy", clean=False))
    return H


def error_picture(dtype):
    return Case("index-61-" + np.dtype(dtype).name, dtype, sizes_of(16, 8, 420), 1, [1, 1], [1, 1], 1, 1, 0,
                header(3, 12) + b"abc" + header(2, 61) + b"xy", clean=False)
