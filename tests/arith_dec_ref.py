"""The reference's arithmetic-coded core-syntax transform-data DECODER restated over the picture's transform-data bytes,
with a writer (an arithmetic ENCODER of the test's own) for drawn pictures.  TEST INFRASTRUCTURE.

Decoder: schro_decoder_parse_transform_data (schrodecoder.c:2939-2987, the headers: tests/noarith_dec_ref.py's walk) and
schro_decoder_decode_transform_data (:2990-3015) for !is_noarith over schro_decoder_decode_subband (:3525-3638),
schro_decoder_setup_codeblocks (:3279-3308), schro_decoder_test_quant_offset_compat (:3324-3352),
schro_decoder_decode_codeblock (:3452-3522) and the generic line decoder (:3018-3217).  The bin is
oracle/dirac_stream.py's Arith, which the reference decoder's digests pin; everything around it is stated again here and
must agree with dirac_stream.Decoder.decode_coefficients on the reference's stream (tests/test_arith_dec_ref.py).

Where the reference is undefined, this file defines (and schro_hip_arith_decode_batch follows):
  * a uint keeps `bits` mod 2^32, the value is bits - 1 as a 32-bit int; a code of 31 or more data bins counts in
    long_codes (the quant offset's loop stops after 30, so it never does); a wrapped value of 0 has no sign bin;
  * offset + factor * v + 2 wraps at 32 bits, the shift is arithmetic, the negation wraps; then truncation to the type;
  * quant index + offset is clamped to 0 .. 60 from the exact sum (clamped_quant);
  * the headers' undefined cases -- a quant index above 60, a length past the input -- as tests/noarith_dec_ref.py.
After a sub-band: schro_arith_decode_flush; offset < length - 1 counts in not_consumed, offset > length + 4 in overran.
bins counts every binary decision of the payloads but the compat peeks'.

Writer: any bytes the decoder reads back as the drawn values serve, so the encoder below is not the reference's.  It keeps
`low` as an exact integer: the decoder decides bin after bin whether x - low >= range_x_prob for the number x the payload
spells (0xff bytes behind its end), and the bits of x it has not fetched yet never reach the 16 bits the comparison looks
at; so x decodes to the coded bins exactly when low <= x < low + range throughout, and the shortest such byte string
followed by 1-bits is taken.  Pinned by the round trip through the decoder (tests/test_arith_dec_ref.py)."""
import numpy as np

import noarith_dec_ref as ND
import noarith_enc_ref as enc
import stream_lib as S

D = S.D
M32 = 0xffffffff
MAX_SUBBANDS = ND.MAX_SUBBANDS
s32, truncate, flags_of = ND.s32, ND.truncate, ND.flags_of

_tables = {}


def tables():
    """(lut, quant factor, offset_1_2, offset_3_8)"""
    if not _tables:
        import oracle_lib as O
        t = S.load_tables()
        qf, qo12 = O.quant_tables()
        _tables["t"] = (t["arith_lut"], [int(v) for v in qf], [int(v) for v in qo12], [int(v) for v in t["schro_table_offset_3_8"]])
    return _tables["t"]


class Dec:
    """The decoding side of a walk: a bin is read."""

    def __init__(self, payload):
        self.a = D.Arith(bytes(payload), tables()[0])
        self.bins = 0

    def bit(self, ctx, known=None):
        self.bins += 1
        return self.a.bit(ctx)

    def end_offset(self):
        """schro_arith_decode_flush"""
        return self.a.offset + (self.a.cntr < 8)


class Enc:
    """The encoding side: the known bin is coded and handed back."""

    def __init__(self):
        self.lut = tables()[0]
        self.low, self.range, self.shifts = 0, 0xffff0000, 0
        self.prob = [0x8000] * D.CTX_LAST
        self.bins = 0

    def bit(self, ctx, known):
        self.bins += 1
        while self.range <= 0x40000000:
            self.range <<= 1
            self.low <<= 1
            self.shifts += 1
        p = self.prob[ctx]
        rxp = ((self.range >> 16) * p) & 0xffff0000
        if known:
            self.low += rxp
            self.range -= rxp
            self.prob[ctx] = p - self.lut[p >> 8]
        else:
            self.range = rxp
            self.prob[ctx] = p + self.lut[255 - (p >> 8)]
        return known

    def end_offset(self):
        """Where the decoder's offset stands behind the same bins and its flush."""
        return 3 + 2 * (self.shifts // 16) + ((16 - self.shifts % 16) < 8)

    def finish(self, clean=True):
        """The shortest bytes (one at least) that, followed by 1-bits, spell a number of [low, low + range); clean: 0xff
        bytes are appended until the decoder does not overrun them (offset <= length + 4)."""
        total = 32 + self.shifts
        high = self.low + self.range - 1
        out = None
        for k in range(1, (total + 7) // 8 + 1):
            rem = total - 8 * k
            if rem <= 0:
                out = (high << -rem).to_bytes(k, "big")
                break
            P = ((high + 1) >> rem) - 1
            if P >= 0 and ((P + 1) << rem) - 1 >= self.low:
                out = P.to_bytes(k, "big")
                break
        if clean and len(out) < self.end_offset() - 4:
            out += b"\xff" * (self.end_offset() - 4 - len(out))
        return out


def code_uint(io, cont, value_ctx, known=None, limit=None):
    """_schro_arith_decode_uint (limit: the 30 of _schro_arith_decode_sint): (bits - 1 as a 32-bit int, data bins).
    known: the non-negative number to code, of any size."""
    bits, count = 1, 0
    if known is not None:
        kbits = known + 1
        n = kbits.bit_length() - 1
        assert limit is None or n < limit
    while True:
        if io.bit(cont, None if known is None else int(count == n)):
            break
        bits = ((bits << 1) | io.bit(value_ctx, None if known is None else (kbits >> (n - 1 - count)) & 1)) & M32
        cont = D.FOLLOW[cont]
        count += 1
        if limit is not None and count == limit:
            break
    return s32((bits - 1) & M32), count


def code_sint(io, known=None):
    """_schro_arith_decode_sint with the quantiser's contexts."""
    v, _ = code_uint(io, D.CTX_Q_CONT, D.CTX_Q_VALUE, None if known is None else abs(known), 30)
    if v and io.bit(D.CTX_Q_SIGN, None if known is None else int(known < 0)):
        v = -v
    return v


def dequantise(v, factor, offset):
    """(offset + factor * v + 2) >> 2 in 32-bit two's complement."""
    return s32((offset + factor * v + 2) & M32) >> 2


def rectangle(bw, bh, hc, vc, x, y):
    return (x * bw) // hc, (y * bh) // vc, ((x + 1) * bw) // hc, ((y + 1) * bh) // vc


def walk_subband(io, fd, qd, parent, index, hc, vc, quant_index, have_quant_offset, is_intra, result, known=None, offsets=None,
                 zero_codeblocks=True, used=None):
    """The codeblocks of one coded sub-band.  fd: the band in the coefficient plane (written as stored), qd: in the quant
    plane or None, parent: the band index - 3 or None.  Decoding (known None) reads; writing takes the quantised values
    from known (a band-shaped array of Python ints or numbers) and offsets (x, y) -> the quant offset of a codeblock."""
    lut, qf, qo12, qo38 = tables()
    qoff = qo12 if is_intra else qo38
    dtype = fd.dtype
    bh, bw = fd.shape
    orient = 0 if index == 0 else (index - 1) % 3 + 1
    have_zero_flags = hc > 1 or vc > 1
    rows = [[int(v) for v in r] for r in fd]
    prow = [[int(v) for v in r] for r in parent] if parent is not None else None
    for y in range(vc):
        for x in range(hc):
            x0, y0, x1, y1 = rectangle(bw, bh, hc, vc, x, y)
            if have_zero_flags:
                zero = None
                if known is not None:
                    zero = int(zero_codeblocks and not any(known[j][i] for j in range(y0, y1) for i in range(x0, x1)))
                if io.bit(D.CTX_ZERO_CODEBLOCK, zero):
                    for j in range(y0, y1):
                        rows[j][x0:x1] = [0] * (x1 - x0)
                    if qd is not None:
                        qd[y0:y1, x0:x1] = 0
                    continue
            if have_quant_offset:
                q = quant_index + code_sint(io, None if known is None else int(offsets(x, y)) if offsets else 0)
                quant_index = min(max(q, 0), 60)
                result["clamped_quant"] += q != quant_index
            if used is not None:
                used[y, x] = quant_index
            factor, offset = qf[quant_index], qoff[quant_index]
            for j in range(y0, y1):
                line = rows[j]
                prev = rows[j - 1] if j > 0 else None
                par = prow[j >> 1] if prow is not None else None
                for i in range(x0, x1):
                    left = line[i - 1] if i > 0 else 0
                    up = prev[i] if prev is not None else 0
                    nhood = left | up | (prev[i - 1] if prev is not None and i > 0 else 0)
                    if par is not None and par[i >> 1] != 0:
                        cont = D.CTX_NPNN_F1 if nhood else D.CTX_NPZN_F1
                    else:
                        cont = D.CTX_ZPNN_F1 if nhood else D.CTX_ZPZN_F1
                    pv = left if orient == 2 else up if orient == 1 else 0
                    sign = D.CTX_SIGN_NEG if pv < 0 else D.CTX_SIGN_POS if pv > 0 else D.CTX_SIGN_ZERO
                    k = None if known is None else int(known[j][i])
                    v, count = code_uint(io, cont, D.CTX_COEFF_DATA, None if k is None else abs(k))
                    result["long_codes"] += count >= 31
                    stored = asread = 0
                    if v:
                        d = dequantise(v, factor, offset)
                        if io.bit(sign, None if k is None else int(k < 0)):
                            d, v = s32(-d & M32), s32(-v & M32)
                        stored, asread = truncate(d & M32, dtype), truncate(v & M32, dtype)
                    line[i] = stored
                    if qd is not None:
                        qd[j, i] = asread
    fd[...] = np.array(rows, np.int64).astype(dtype) if bh * bw else fd
    return quant_index


def empty_result(compat):
    r = ND.empty_result(compat)
    r["bins"] = 0
    return r


def decode_transform_data(data, coeffs, quant, depth, horiz_codeblocks, vert_codeblocks, codeblock_mode_index, is_intra, compat,
                          band_bins=None):
    """coeffs, quant: Y, U, V planes of the transform's size (int16 or int32) holding whatever they held; they are written
    in place exactly where the decoder writes (quant may be None) -- everywhere, unless the header walk sets the error.
    The LL band of an intra picture is not DC-predicted.  Returns the result block as a dict.  band_bins: a dict that takes
    the bins of every coded sub-band, by (component, index)."""
    result = empty_result(compat)
    bands = ND.parse_transform_data(data, depth, result)
    if bands is None:
        return result
    coded = {(k, i): rest for k, i, *rest in bands}
    for component in range(3):
        for i in range(1 + 3 * depth):
            fd = enc.subband(coeffs[component], depth, i)
            qd = enc.subband(quant[component], depth, i) if quant is not None else None
            if (component, i) not in coded:
                fd[...] = 0
                if qd is not None:
                    qd[...] = 0
                continue
            quant_index, length, payload = coded[component, i]
            hc, vc = enc.codeblock_counts(i, horiz_codeblocks, vert_codeblocks)
            _, have_quant_offset = flags_of(hc, vc, codeblock_mode_index, compat)
            # schro_decoder_test_quant_offset_compat: a sint peeked on a copy of the fresh coder
            if have_quant_offset and hc == 1 and vc == 1 and i == 0:
                if not 0 <= quant_index + code_sint(Dec(payload)) <= 60:
                    compat = 1
                    have_quant_offset = False
            io = Dec(payload)
            parent = enc.subband(coeffs[component], depth, i - 3) if i >= 4 else None
            walk_subband(io, fd, qd, parent, i, hc, vc, quant_index, have_quant_offset, is_intra, result)
            offset = io.end_offset()
            result["not_consumed"] += offset < length - 1
            result["overran"] += offset > length + 4
            result["bins"] = min(result["bins"] + io.bins, M32)
            if band_bins is not None:
                band_bins[component, i] = io.bins
    result["compat_quant_offset"] = int(compat)
    return result


def write_transform_data(planes, depth, horiz_codeblocks, vert_codeblocks, codeblock_mode_index, compat, quant_indices, is_intra,
                         offsets=None, zero_codeblocks=True, clean=True, dtype=np.int16):
    """The bytes a decoder in state `compat` reads back as `planes` (Y, U, V planes of quantised values: arrays, or nested
    lists of Python ints for magnitudes past 32 bits).  quant_indices[component][index] is the header's; offsets
    (component, index, x, y) -> the quant offset in front of a codeblock (default 0), wherever the decoder reads one.  A
    sub-band without a non-zero value takes the zero form.  The contexts come from the values as the decoder will have
    STORED them, so the writer dequantises and truncates to `dtype` as it goes.  The compat test is the decoder's: where it
    would peek, the band is first written without an offset and the peek taken on those bytes.  Returns (bytes, coefficient planes as stored,
    {(component, index): (vc, hc) array of the quant index in use, -1 zero codeblock}, compat after)."""
    pack = enc.Pack()
    used = {}
    result = empty_result(compat)
    stored = [np.zeros(np.asarray(p, object).shape, dtype) for p in planes]
    for component in range(3):
        src = np.asarray(planes[component], object)
        for i in range(1 + 3 * depth):
            pack.sync()
            kd = enc.subband(src, depth, i)
            fd = enc.subband(stored[component], depth, i)
            if not any(v != 0 for v in kd.ravel()):
                pack.encode_uint(0)
                continue
            hc, vc = enc.codeblock_counts(i, horiz_codeblocks, vert_codeblocks)
            _, have_quant_offset = flags_of(hc, vc, codeblock_mode_index, compat)
            quant_index = int(quant_indices[component][i])
            band_offsets = (lambda x, y, component=component, i=i: offsets(component, i, x, y)) if offsets else None
            parent = enc.subband(stored[component], depth, i - 3) if i >= 4 else None

            def attempt(with_offset):
                io, qis = Enc(), np.full((vc, hc), -1, np.int64)
                walk_subband(io, fd, None, parent, i, hc, vc, quant_index, with_offset, is_intra, result, known=kd.tolist(),
                             offsets=band_offsets, zero_codeblocks=zero_codeblocks, used=qis)
                return io.finish(clean), qis
            if have_quant_offset and hc == 1 and vc == 1 and i == 0:
                # the decoder peeks a sint: were the band written without an offset and the peek left 0 .. 60, it would turn
                # compat on and read that form; else it must find an offset, and one that stays inside
                payload, qis = attempt(False)
                if not 0 <= quant_index + code_sint(Dec(payload)) <= 60:
                    compat = 1
                else:
                    assert 0 <= quant_index + (int(band_offsets(0, 0)) if band_offsets else 0) <= 60
                    payload, qis = attempt(True)
            else:
                payload, qis = attempt(have_quant_offset)
            used[component, i] = qis
            pack.encode_uint(len(payload))
            pack.encode_uint(quant_index)
            pack.sync()
            pack.append(payload)
    pack.sync()
    return bytes(pack.data), stored, used, int(compat)
