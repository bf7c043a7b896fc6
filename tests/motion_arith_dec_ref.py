"""A restatement of the motion data of an arithmetic-coded picture as the DEVICE decoder defines it (include/schro_hip.h,
schro_hip_motion_arith_decode_batch): schro_decoder_parse_block_data and schro_decoder_decode_block_data / _decode_macroblock
/ _decode_prediction_unit (schrodecoder.c:2531-2814) for !params->is_noarith.  TEST INFRASTRUCTURE.

The header walk and the field rules are tests/motion_dec_ref.py's (the VLC twin's); the bin is oracle/dirac_stream.py's
Arith, which the reference decoder's digests pin.  What this file adds is what lies between: nine coders, one per section,
every probability 0x8000, and per section a fixed chain of contexts --

  splits   _schro_arith_decode_uint (SB_F1 -> SB_F2 -> SB_F2 .., SB_DATA); `bits` kept mod 2^32, value bits - 1 mod 2^32,
           31 or more data bins count in long_codes;
  modes    a bin in BLOCK_MODE_REF1, with two references one in BLOCK_MODE_REF2, and with have_global_motion, where the mode
           is not 0, one in GLOBAL_BLOCK;
  vectors  _schro_arith_decode_sint (CONT_BIN1 .. CONT_BIN5 (repeats), VALUE, SIGN), the loop stopped after 30 data bins;
  DCs      the same over CONT_BIN1, CONT_BIN2 (repeats), VALUE, SIGN.

No context depends on a decoded neighbour, so a section's k-th value is the same whatever the field is.  Two forms, held
equal by tests/test_motion_arith_dec_ref.py: decode (the reference's order: superblock by superblock, nine coders in
lockstep) and decode_phased (motion_arith_dec.hip's: a section's chain decoded for as many values as the walk before it
found, then the walk).  Both yield the whole SchroHipMotionArithDecodeResult as a dict: per section the coder's `offset`
behind the last bin asked (3 if none was, 0 for an absent section) and its bins; not_consumed where offset < length and
overran where offset > length + 6 (:2594, :2598; `length` as the header states it; no flush is involved).

The writer is arith_dec_ref.Enc with its exact-integer `low`: values_of_field gives the nine sections' values of a field,
write frames them as the stream frames them -- per section uint length, byte_sync, payload."""
import numpy as np

import arith_dec_ref as AD
import motion_dec_ref as VD
import noarith_enc_ref as enc
from motion_enc_ref import (SECTIONS, Motion, dc_prediction, global_prediction, mode_prediction, split_prediction, units,
                            vector_prediction)
from schroedinger_amd import MV_DTYPE

D = AD.D
M32 = 0xffffffff
absent, diagonals = VD.absent, VD.diagonals

MV_CTX = (D.CTX_MV_CONT1, D.CTX_MV_VALUE, D.CTX_MV_SIGN)
DC_CTX = (D.CTX_DC_CONT1, D.CTX_DC_VALUE, D.CTX_DC_SIGN)
MODE_CTX = (D.CTX_MODE_REF1, D.CTX_MODE_REF2, D.CTX_GLOBAL)


def sint_ctx(s):
    return MV_CTX if s < 6 else DC_CTX


def parse(data, num_refs):
    """The header walk of motion_dec_ref.parse with the stated lengths: per section (first byte, kept bytes, stated length)
    or None, the truncated mask, `bytes`, the headers' long codes."""
    data = bytes(data)
    u = VD.Bits(data)
    sections, truncated = [None] * SECTIONS, 0
    for s in range(SECTIONS):
        if absent(num_refs, s):
            continue
        u.sync()
        length = u.code(False)
        u.sync()
        first = u.pos >> 3
        kept = min(length, len(data) - first) if first < len(data) else 0
        truncated |= (kept < length) << s
        sections[s] = (first if kept else 0, kept, length)
        u.pos += 8 * length
    return sections, truncated, min((u.pos + 7) >> 3, len(data)), u.longs


def code_uint(io, cont, value_ctx, known=None, limit=None):
    """arith_dec_ref.code_uint, which a code of exactly `limit` data bins may pass too (its loop then ends without a
    continuation bin): (bits - 1 mod 2^32, data bins).  known: the non-negative number to code, of any size."""
    bits, count = 1, 0
    if known is not None:
        kbits = known + 1
        n = kbits.bit_length() - 1
        assert limit is None or n <= limit
    while True:
        if io.bit(cont, None if known is None else int(count == n)):
            break
        bits = ((bits << 1) | io.bit(value_ctx, None if known is None else (kbits >> (n - 1 - count)) & 1)) & M32
        cont = D.FOLLOW[cont]
        count += 1
        if limit is not None and count == limit:
            break
    return (bits - 1) & M32, count


def code_sint(io, s, known=None):
    """_schro_arith_decode_sint over section s's contexts: the value as 32 bits (a negative one as its two's complement)."""
    cont, value, sign = sint_ctx(s)
    v, _ = code_uint(io, cont, value, None if known is None else abs(known), 30)
    if v and io.bit(sign, None if known is None else int(known < 0)):
        v = -v
    return v & M32


class Section:
    """One section's coder and the values it has yielded so far."""

    def __init__(self, s, payload):
        self.s, self.io = s, AD.Dec(payload)
        self.values, self.units, self.longs = [], 0, 0

    def next(self):
        if self.s == 0:
            v, count = code_uint(self.io, D.CTX_SB_F1, D.CTX_SB_DATA)
            self.longs += count >= 31
        else:
            v = code_sint(self.io, self.s)
        self.values.append(v)
        return v

    def fill(self, n):
        """The chain: n values, one after the other."""
        assert not self.values
        for _ in range(n):
            self.next()
        self.units = n

    def take(self):
        self.units += 1
        return self.next()

    def value(self, i):
        return self.values[i]       # (a walk asks only for what the chain decoded)

    def bit(self, ctx):
        return self.io.bit(ctx)


def _open(data, nbx, nby, num_refs):
    data = bytes(data)
    sections, truncated, nbytes, longs = parse(data, num_refs)
    coder = {s: Section(s, data[sec[0]:sec[0] + sec[1]]) for s, sec in enumerate(sections) if sec is not None}
    return sections, truncated, nbytes, longs, coder


def _close(m, nbx, nby, num_refs, sections, truncated, nbytes, longs, coder, mode_units):
    field = np.zeros(nbx * nby, MV_DTYPE)
    field["flags"] = [p | (g << 2) | (s << 3) for p, g, s in zip(m.pred_mode, m.using_global, m.split)]
    field["v"] = m.v
    kept, units_, offset, bins = [0] * SECTIONS, [0] * SECTIONS, [0] * SECTIONS, [0] * SECTIONS
    overran = not_consumed = 0
    for s, c in coder.items():
        kept[s], length = sections[s][1], sections[s][2]
        units_[s] = mode_units if s == 1 else c.units
        offset[s], bins[s] = c.io.a.offset, min(c.io.bins, M32)
        not_consumed |= (offset[s] < length) << s
        overran |= (offset[s] > length + 6) << s
    bad = [k for k in range(nbx * nby) if m.pred_mode[k] == 0 and any(not -128 <= m.v[k][i] <= 127 for i in range(3))]
    result = {"bytes": nbytes, "section_bytes": kept, "section_units": units_, "section_offset": offset, "section_bins": bins,
              "truncated": truncated, "overran": overran, "not_consumed": not_consumed,
              "long_codes": longs + coder[0].longs, "unverified": len(bad), "first_unverified": bad[0] if bad else -1}
    return field, result


def decode(data, nbx, nby, num_refs, have_global_motion, log=None):
    """(field, result) in the reference's order.  log: nine lists that take every value a section yields at the top level,
    as dirac_stream.Decoder.decode_block_data logs them (residuals as signed numbers)."""
    hg = int(bool(have_global_motion))
    sections, truncated, nbytes, longs, coder = _open(data, nbx, nby, num_refs)
    m = Motion(np.zeros(nbx * nby, MV_DTYPE), nbx, nby, num_refs, hg)
    mode_units = 0

    def copy(dst, src):
        m.pred_mode[dst], m.using_global[dst], m.split[dst], m.v[dst] = m.pred_mode[src], m.using_global[src], m.split[src], list(m.v[src])

    def mode_bin(k):
        b = coder[1].bit(MODE_CTX[k])
        if log is not None:
            log[1].append(b)
        return b

    def prediction_unit(x, y):
        nonlocal mode_units
        k = m.at(x, y)
        mode_units += 1
        m.pred_mode[k] = mode_prediction(m, x, y) ^ mode_bin(0)
        if num_refs > 1:
            m.pred_mode[k] ^= mode_bin(1) << 1
        m.using_global[k] = 0
        if m.pred_mode[k] and hg:
            m.using_global[k] = global_prediction(m, x, y) ^ mode_bin(2)
        VD._values(m, coder, x, y)

    for j in range(0, nby, 4):
        for i in range(0, nbx, 4):
            k = m.at(i, j)
            m.split[k] = (split_prediction(m, i, j) + coder[0].take()) % 3
            step = 4 >> m.split[k]
            for l in range(0, 4, step):
                for c in range(0, 4, step):
                    o = m.at(i + c, j + l)
                    m.split[o] = m.split[k]
                    prediction_unit(i + c, j + l)
                    for ll in range(step):
                        for cc in range(step):
                            if ll or cc:
                                copy(m.at(i + c + cc, j + l + ll), o)
    if log is not None:
        for s, c in coder.items():
            if s != 1:
                log[s].extend(v if s == 0 else AD.s32(v) for v in c.values)
    return _close(m, nbx, nby, num_refs, sections, truncated, nbytes, longs, coder, mode_units)


def decode_phased(data, nbx, nby, num_refs, have_global_motion):
    """(field, result) in the phases of motion_arith_dec.hip: a chain, then the walk it feeds."""
    hg = int(bool(have_global_motion))
    sections, truncated, nbytes, longs, coder = _open(data, nbx, nby, num_refs)
    m = Motion(np.zeros(nbx * nby, MV_DTYPE), nbx, nby, num_refs, hg)
    nsbx, nsby = nbx // 4, nby // 4

    # 1. the split chain, the split walk, every superblock's first unit
    coder[0].fill(nsbx * nsby)
    for sx, sy in diagonals(nsbx, nsby):
        m.split[m.at(4 * sx, 4 * sy)] = (split_prediction(m, 4 * sx, 4 * sy) + coder[0].value(sy * nsbx + sx)) % 3
    split = [m.split[m.at(4 * (k % nsbx), 4 * (k // nsbx))] for k in range(nsbx * nsby)]
    unit_first = np.concatenate([[0], np.cumsum([1 << (2 * s) for s in split])]).tolist()
    mode_units = unit_first[-1]

    def origin(x, y):
        sp = split[(y >> 2) * nsbx + (x >> 2)]
        step = 4 >> sp
        return None if (x | y) & (step - 1) else (sp, step)

    def spread(x, y, sp, step):
        k = m.at(x, y)
        for l in range(step):
            for c in range(step):
                o = m.at(x + c, y + l)
                m.pred_mode[o], m.using_global[o], m.split[o] = m.pred_mode[k], m.using_global[k], sp

    def stream_units():
        for sb in range(nsbx * nsby):
            step = 4 >> split[sb]
            for l in range(0, 4, step):
                for c in range(0, 4, step):
                    yield 4 * (sb % nsbx) + c, 4 * (sb // nsbx) + l, split[sb], step

    # 2. the mode chain and the mode walk -- or, with global motion, one walk in stream order that decodes as it predicts
    nbits = 1 + (num_refs > 1)
    if not hg:
        bins = [[coder[1].bit(MODE_CTX[b]) for b in range(nbits)] for _ in range(mode_units)]
        for x, y in diagonals(nbx, nby):
            o = origin(x, y)
            if o is None:
                continue
            sp, step = o
            n = unit_first[(y >> 2) * nsbx + (x >> 2)] + (((y & 3) >> (2 - sp)) << sp) + ((x & 3) >> (2 - sp))
            m.pred_mode[m.at(x, y)] = mode_prediction(m, x, y) ^ sum(b << i for i, b in enumerate(bins[n]))
            spread(x, y, sp, step)
    else:
        for x, y, sp, step in stream_units():
            k = m.at(x, y)
            m.pred_mode[k] = mode_prediction(m, x, y) ^ coder[1].bit(MODE_CTX[0])
            if num_refs > 1:
                m.pred_mode[k] ^= coder[1].bit(MODE_CTX[1]) << 1
            m.using_global[k] = global_prediction(m, x, y) ^ coder[1].bit(MODE_CTX[2]) if m.pred_mode[k] else 0
            spread(x, y, sp, step)
    # 3. which value a unit owns: prefix counts in stream order
    count, index = [0, 0, 0], {}
    for x, y, sp, step in stream_units():
        k = m.at(x, y)
        mode, ug = m.pred_mode[k], m.using_global[k]
        index[k] = (count[2] if mode == 0 else count[0], count[1])
        count[0] += bool(mode & 1) and not ug
        count[1] += bool(mode & 2) and not ug
        count[2] += mode == 0
    # 4. the value chains, then the value walk
    for s in range(2, SECTIONS):
        if s in coder:
            coder[s].fill(count[0 if s < 4 else 1 if s < 6 else 2])
    for x, y in diagonals(nbx, nby):
        o = origin(x, y)
        if o is None:
            continue
        k = m.at(x, y)
        VD._values(m, coder, x, y, index[k])
        for l in range(o[1]):
            for c in range(o[1]):
                m.v[m.at(x + c, y + l)] = list(m.v[k])
    return _close(m, nbx, nby, num_refs, sections, truncated, nbytes, longs, coder, mode_units)


# ---- the writer --------------------------------------------------------------------------------------------------------------

def values_of_field(field, nbx, nby, num_refs, have_global_motion):
    """Nine lists: what each section codes for `field`, in stream order -- split residuals, (context, bit) pairs, signed
    residuals.  The sections are schro_encoder_encode_superblock_split .. _dc_data's (tests/motion_enc_ref.encode)."""
    m = Motion(field, nbx, nby, num_refs, have_global_motion)
    log = [[] for _ in range(SECTIONS)]
    for j in range(0, nby, 4):
        for i in range(0, nbx, 4):
            log[0].append((m.split[m.at(i, j)] - split_prediction(m, i, j) + 3) % 3)
    for x, y in units(m):
        k = m.at(x, y)
        r = m.pred_mode[k] ^ mode_prediction(m, x, y)
        log[1].append((MODE_CTX[0], r & 1))
        if num_refs > 1:
            log[1].append((MODE_CTX[1], r >> 1))
        if m.pred_mode[k] and have_global_motion:
            log[1].append((MODE_CTX[2], m.using_global[k] ^ global_prediction(m, x, y)))
        if m.pred_mode[k] == 0:
            pred = dc_prediction(m, x, y)
            for comp in range(3):
                log[6 + comp].append(m.v[k][comp] - pred[comp])
        elif not m.using_global[k]:
            for ref in range(num_refs):
                if m.pred_mode[k] & (1 << ref):
                    px, py = vector_prediction(m, x, y, 1 << ref)
                    log[2 + 2 * ref].append(m.dx(k, ref) - px)
                    log[3 + 2 * ref].append(m.dy(k, ref) - py)
    return log


def write_section(s, values, num_refs=2, clean=True):
    """The payload of section s for `values` (mode bins: (context, bit) pairs, or bare bits of a picture without global
    motion).  clean: 0xff bytes are appended until the decoder does not overrun them (offset <= length + 6)."""
    io = AD.Enc()
    nbits = 1 + (num_refs > 1)
    for n, v in enumerate(values):
        if s == 0:
            code_uint(io, D.CTX_SB_F1, D.CTX_SB_DATA, int(v))
        elif s == 1:
            ctx, bit = v if isinstance(v, tuple) else (MODE_CTX[n % nbits], v)
            io.bit(ctx, int(bit))
        else:
            code_sint(io, s, int(v))
    if not values:
        return b""
    out = io.finish(False)
    offset = 3 + 2 * (io.shifts // 16)          # the decoder's, behind the same bins
    if clean and len(out) < offset - 6:
        out += b"\xff" * (offset - 6 - len(out))
    return out


def frame(payloads, num_refs, lengths=None):
    """Per section the stream has: byte_sync, uint length, byte_sync, payload (schrodecoder.c:2531-2553).  lengths: the
    stated lengths where they are not the payloads'."""
    pack = enc.Pack()
    for s in range(SECTIONS):
        if absent(num_refs, s):
            continue
        pack.sync()
        pack.encode_uint(len(payloads[s]) if lengths is None else lengths[s])
        pack.sync()
        pack.append(payloads[s])
    return bytes(pack.data)


def write(log, num_refs, clean=True):
    """The bytes of nine lists of values."""
    return frame([b"" if absent(num_refs, s) else write_section(s, log[s], num_refs, clean) for s in range(SECTIONS)], num_refs)


def write_field(field, nbx, nby, num_refs, have_global_motion, clean=True):
    return write(values_of_field(field, nbx, nby, num_refs, have_global_motion), num_refs, clean)


def payloads_of(data, num_refs):
    data = bytes(data)
    return [b"" if sec is None else data[sec[0]:sec[0] + sec[1]] for sec in parse(data, num_refs)[0]]


# ---- the reference's stream ---------------------------------------------------------------------------------------------------

_stream = []


def stream_pictures():
    """Per inter picture of tests/golden/test_stream.drc in coded order: (Picture as dirac_stream parses it, the parse
    unit's payload, the motion data re-serialised from Picture.motion_buffers -- per section uint length, sync, payload).
    Parsed once."""
    if not _stream:
        import noarith_twin as T
        import stream_lib as S
        dec = T._decoder()
        for code, payload in D.parse_units(S.load_stream()):
            if code == 0x00:
                dec.fmt = D.parse_sequence_header(payload)
            elif code & 8:
                pic = dec.parse_picture(code, payload)
                if pic.num_refs:
                    bufs = [b"" if b is None else bytes(b) for b in pic.motion_buffers]
                    _stream.append((pic, bytes(payload), frame(bufs, pic.num_refs)))
    return _stream


def stream_motion(number):
    for pic, payload, data in stream_pictures():
        if pic.number == number:
            return data
    raise KeyError(number)
