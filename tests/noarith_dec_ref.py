"""The reference's VLC (noarith) core-syntax transform-data DECODER restated, with a writer that follows the decoder's
rules and a model of the device's chunk summaries.

Decoder: schro_decoder_parse_transform_data (schrodecoder.c:2939-2987) and schro_decoder_decode_transform_data (:2990-3015)
over schro_decoder_decode_subband (:3525-3625), schro_decoder_setup_codeblocks (:3279-3308),
schro_decoder_test_quant_offset_compat (:3324-3352) and schro_decoder_decode_codeblock_noarith (:3355-3449), with the bit
reader of schrounpack.c: both unpacks have guard bit 1, so a read past the end gives 1-bits.

The DECODER's rules differ from the encoder's (tests/noarith_enc_ref.py): a zero flag is read whenever the sub-band has
more than one codeblock, sub-band 0 included, and a quant offset whenever codeblock_mode_index is 1 unless the instance is
in compat mode and the sub-band has one codeblock.  The two agree where sub-band 0 has 1 x 1 codeblocks and either the
mode is 0 or compat is on.

Pinned by the hand-derived byte strings of tests/test_noarith_dec_ref.py and, on reference-produced data, by
tests/test_noarith_twin.py: the quantised planes of the reference's own stream through `write_transform_data` decode to the
stream's coefficients for all 100 pictures (s16, one quant index per sub-band, one codeblock in sub-band 0).

Where the reference is undefined, this file defines (and schro_hip_noarith_decode_batch follows):
  * a code of 31 or more data bits (`1 << count` overflows in schro_unpack_decode_uint): v = 1; per data bit
    v = (v << 1 | b) mod 2^32; the magnitude is v - 1 mod 2^32; a code with data bits always has a sign bit (the reference
    skips it when the wrapped magnitude is 0); then the sign, then truncation to the sample type.  Such codes are counted
    in long_codes (those of the headers, the quant offsets and the values; the compat test's peek is not counted);
  * a `length` that reaches past the input: the payload is cut at the input's end (`truncated` counts the sub-bands);
  * a header quant index above 60: error, first_error = component * 19 + index, nothing decoded, the compat state as
    it came in, the header fields and counters as they stood when the walk stopped;
  * bytes_read: the outer unpack's position in whole bytes (rounded up), saturated at 2^32 - 1.
"""
import numpy as np

import noarith_enc_ref as enc
import oracle_lib

MAX_SUBBANDS = enc.MAX_SUBBANDS
M32 = 0xffffffff
A, D, F, S = 0, 1, 2, 3         # code start, data bit, follow bit after data, sign bit


class Reader:
    """schrounpack.c with guard bit 1 over data[:limit]; positions in bits."""

    def __init__(self, data, pad):
        data = bytes(data)
        self.nbits = 8 * len(data)
        self.bits = "".join("{:08b}".format(b) for b in data) + "1" * 72
        self.pos = 0
        self.long_codes = 0

    def decode_bit(self):
        b = 1 if self.pos >= self.nbits else int(self.bits[self.pos] == "1")
        self.pos += 1
        return b

    def _code(self, pos):
        """(v mod 2^32, data bits, position behind the follow 1).  Data bits are 0-bits' neighbours, so the walk never
        leaves the bytes by more than the padding."""
        if pos >= self.nbits:
            return 1, 0, pos + 1
        bits, v, n = self.bits, 1, 0
        while bits[pos] == "0":
            v = ((v << 1) | (bits[pos + 1] == "1")) & M32
            n += 1
            pos += 2
        return v, n, pos + 1

    def decode_uint(self, count=True):
        v, n, self.pos = self._code(self.pos)
        if count and n >= 31:
            self.long_codes += 1
        return (v - 1) & M32

    def decode_sint32(self, count=True):
        """The value as 32 bits (two's complement)."""
        v, n, pos = self._code(self.pos)
        m = (v - 1) & M32
        if n:
            if pos >= self.nbits or self.bits[pos] == "1":
                m = (-m) & M32
            pos += 1
        self.pos = pos
        if count and n >= 31:
            self.long_codes += 1
        return m

    def peek_sint32(self):
        pos = self.pos
        m = self.decode_sint32(count=False)
        self.pos = pos
        return m

    def byte_sync(self):
        self.pos = (self.pos + 7) & ~7


def s32(m):
    return m - (1 << 32) if m & 0x80000000 else m


def truncate(m, dtype):
    if np.dtype(dtype) == np.int16:
        m &= 0xffff
        return m - 0x10000 if m & 0x8000 else m
    return s32(m)


def flags_of(hc, vc, codeblock_mode_index, compat):
    """schro_decoder_setup_codeblocks: have_zero_flags, have_quant_offset."""
    one = hc == 1 and vc == 1
    return not one, codeblock_mode_index == 1 and not (compat and one)


def empty_result(compat):
    return {"bytes_read": 0, "error": 0, "first_error": 0, "compat_quant_offset": int(compat), "truncated": 0, "not_consumed": 0,
            "overran": 0, "long_codes": 0, "clamped_quant": 0, "subband_length": np.zeros((3, MAX_SUBBANDS), np.int64),
            "subband_quant_index": np.zeros((3, MAX_SUBBANDS), np.int64)}


def parse_transform_data(data, depth, result):
    """schro_decoder_parse_transform_data: [(component, index, quant index, stated length, payload bytes)] of the coded
    sub-bands, or None on the error."""
    un = Reader(data, 64)
    out = []
    for component in range(3):
        for i in range(1 + 3 * depth):
            un.byte_sync()
            length = un.decode_uint()
            if length == 0:
                un.byte_sync()
                continue
            quant_index = un.decode_uint()
            if quant_index > 60:
                result["error"], result["first_error"] = 1, component * MAX_SUBBANDS + i
                result["bytes_read"] = min((un.pos + 7) >> 3, M32)
                result["long_codes"] = un.long_codes
                return None
            un.byte_sync()
            first = un.pos >> 3
            payload = bytes(data[first:first + length]) if first < len(data) else b""
            result["truncated"] += len(payload) < length
            result["subband_length"][component, i] = length
            result["subband_quant_index"][component, i] = quant_index
            out.append((component, i, quant_index, length, payload))
            un.pos += 8 * length
    un.byte_sync()
    result["bytes_read"] = min(un.pos >> 3, M32)
    result["long_codes"] = un.long_codes
    return out


def decode_transform_data(data, coeffs, quant, depth, horiz_codeblocks, vert_codeblocks, codeblock_mode_index, is_intra, compat):
    """coeffs, quant: Y, U, V planes of the transform's size (int16 or int32) holding whatever they held; they are written
    in place exactly where the decoder writes (quant may be None).  Returns the result block as a dict."""
    result = empty_result(compat)
    bands = parse_transform_data(data, depth, result)
    if bands is None:
        return result
    dtype = coeffs[0].dtype
    arith = 1 if dtype == np.int16 else 0
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
            un = Reader(payload, fd.size + hc * vc)
            have_zero_flags, have_quant_offset = flags_of(hc, vc, codeblock_mode_index, compat)
            for y in range(vc):
                for x in range(hc):
                    cb = enc.get_codeblock(fd, x, y, hc, vc)
                    if have_zero_flags and un.decode_bit():
                        cb[...] = 0
                        if qd is not None:
                            enc.get_codeblock(qd, x, y, hc, vc)[...] = 0
                        continue
                    # schro_decoder_test_quant_offset_compat
                    if have_quant_offset and hc == 1 and vc == 1 and i == 0:
                        if not 0 <= quant_index + s32(un.peek_sint32()) <= 60:
                            compat = 1
                            have_quant_offset = False
                    if have_quant_offset:
                        q = quant_index + s32(un.decode_sint32())
                        quant_index = min(max(q, 0), 60)
                        result["clamped_quant"] += q != quant_index
                    h, w = cb.shape
                    values = np.array([truncate(un.decode_sint32(), dtype) for _ in range(h * w)], dtype).reshape(h, w)
                    if qd is not None:
                        enc.get_codeblock(qd, x, y, hc, vc)[...] = values
                    if h * w:
                        oracle_lib.dequant_codeblock(cb, values, quant_index, is_intra, arith)
            offset = un.pos // 8
            result["not_consumed"] += offset < length - 1
            result["overran"] += offset > length
            result["long_codes"] += un.long_codes
    result["compat_quant_offset"] = int(compat)
    return result


# ---- a writer that follows the decoder's rules ---------------------------------------------------------------------------

def write_transform_data(planes, depth, horiz_codeblocks, vert_codeblocks, codeblock_mode_index, compat, quant_indices,
                         offsets=None, zero_codeblocks=True):
    """The bytes a decoder in state `compat` reads back as `planes` (Y, U, V quant planes).  quant_indices[component][index]
    is the header's; offsets (component, index, x, y) -> the quant offset written in front of that codeblock (default 0),
    wherever the DECODER reads one.  A sub-band without a non-zero value takes the zero form, a codeblock without one (and
    with a flag) the zero flag, unless zero_codeblocks is False.  Returns (bytes, {(component, index): (vc, hc) array of
    the quant index every codeblock is dequantised with -- the carried, clamped one})."""
    pack = enc.Pack()
    used = {}
    for component in range(3):
        for i in range(1 + 3 * depth):
            pack.sync()
            qd = enc.subband(planes[component], depth, i)
            if not np.any(qd != 0):
                pack.encode_uint(0)
                continue
            hc, vc = enc.codeblock_counts(i, horiz_codeblocks, vert_codeblocks)
            have_zero_flags, have_quant_offset = flags_of(hc, vc, codeblock_mode_index, compat)
            sub = enc.Pack()
            quant_index = int(quant_indices[component][i])
            qis = np.full((vc, hc), -1, np.int64)
            for y in range(vc):
                for x in range(hc):
                    cb = enc.get_codeblock(qd, x, y, hc, vc)
                    if have_zero_flags:
                        zero = zero_codeblocks and not np.any(cb != 0)
                        sub.encode_bit(1 if zero else 0)
                        if zero:
                            continue
                    if have_quant_offset:
                        off = int(offsets(component, i, x, y)) if offsets else 0
                        sub.encode_sint(off)
                        quant_index = min(max(quant_index + off, 0), 60)
                    qis[y, x] = quant_index
                    for row in cb:
                        for v in row.tolist():
                            sub.encode_sint(v)
            sub.flush()
            used[component, i] = qis
            pack.encode_uint(sub.get_offset())
            pack.encode_uint(int(quant_indices[component][i]))
            pack.sync()
            pack.append(sub.data)
    pack.sync()
    return bytes(pack.data), used


# ---- the device's parallel form, modelled ---------------------------------------------------------------------------------
# The code is a four-state machine over bits.  A chunk's summary is, per entry state, (exit state, codes completed in the
# chunk); summaries compose associatively, so every chunk's entry state and the number of codes completed before it
# follow from a scan.  A lane then decodes the codes that START in its chunk, following the last one past the boundary.

CHUNK = 64


def step(state, bit):
    """(next state, 1 when a code completed)."""
    if state == A:
        return (A, 1) if bit else (D, 0)
    if state == D:
        return F, 0
    if state == F:
        return (S, 0) if bit else (D, 0)
    return A, 1


def summarize(bits):
    """bits: a string of '0' / '1' (one chunk).  [(exit state, completions)] per entry state."""
    out = []
    for state in (A, D, F, S):
        n = 0
        for b in bits:
            state, done = step(state, b == "1")
            n += done
        out.append((state, n))
    return out


def compose(first, then):
    return [(then[e][0], n + then[e][1]) for e, n in first]


IDENTITY = [(s, 0) for s in (A, D, F, S)]


def serial_codes(bits, entry):
    """From `entry` at bit 0: the 32-bit values of the codes that start in `bits` (1-bits behind its end), in order."""
    r = Reader(b"", 0)
    r.bits, r.nbits = bits + "1" * 72, len(bits)
    state, pos = entry, 0
    while state != A and pos < len(bits):       # the rest of a code that started before
        state, _ = step(state, r.bits[pos] == "1")
        pos += 1
    if state != A:
        return []
    out = []
    r.pos = pos
    while r.pos < len(bits):
        out.append(r.decode_sint32())
    return out


def chunked_codes(bits, entry, chunk=CHUNK):
    """The same by summaries, a scan and a decode per chunk."""
    chunks = [bits[i:i + chunk] for i in range(0, len(bits), chunk)]
    chunks[-1] = chunks[-1] + "1" * (chunk - len(chunks[-1])) if chunks else ""
    sums = [summarize(c) for c in chunks]
    entries, before, run = [], [], IDENTITY
    for s in sums:
        entries.append(run[entry][0])
        before.append(run[entry][1])
        run = compose(run, s)
    padded = "".join(chunks)
    out = []
    for j, (e, n) in enumerate(zip(entries, before)):
        # index of the first code that starts here: completions before, and the one under way
        first = n + (e != A)
        got = []
        r = Reader(b"", 0)
        r.bits, r.nbits = padded[j * chunk:] + "1" * 72, len(padded) - j * chunk
        state, pos = e, 0
        while state != A and pos < chunk:
            state, _ = step(state, r.bits[pos] == "1")
            pos += 1
        if state == A:
            r.pos = pos
            while r.pos < chunk:
                got.append(r.decode_sint32())
        assert first == len(out) + (entry != A), (j, first, len(out))
        out += got
    # codes that start in the last chunk's padding are not part of `bits`
    return out, sums
