"""A restatement of the motion data of a noarith (VLC) picture as the DEVICE decoder defines it (include/schro_hip.h,
schro_hip_motion_decode_batch): schro_decoder_parse_block_data and schro_decoder_decode_block_data / _decode_macroblock /
_decode_prediction_unit (schrodecoder.c:2531-2814) for params->is_noarith, over the predictors of motion_enc_ref, with the
rules for hostile input that the reference leaves undefined:

  - bits behind a section's kept payload read 1;
  - a header is byte_sync, uint, byte_sync; the length is cut at the input's end (`truncated`); a header that starts
    behind the input reads guard bits and gives 0;
  - a code is v = 1; v = (v << 1 | b) mod 2^32 per data bit, value v - 1 mod 2^32; a signed code with data bits always has
    a sign bit; codes of 31 or more data bits are `long_codes`: those of the headers, and per section those among the
    codes it can be asked for at all (blocks; superblocks for the splits), asked for or not;
  - a split is (pred + value) % 3 without a second wrap; vectors and DCs are (int16_t) (pred + value).

Pinned by the hand-derived byte strings of tests/test_motion_dec_ref.py and, on reference-produced data, by
tests/test_noarith_twin.py: `decode` reads the stream's fields back from the noarith twin of the reference's own stream
(tests/noarith_twin.py) for all 96 inter pictures, every counter 0.

Three forms, held equal by tests/test_motion_dec_ref.py: decode (the reference's serial order), decode_wavefront (the
phases of motion_dec.hip: splits over anti-diagonals of superblocks, unit prefix sum, modes over anti-diagonals of blocks,
code-index prefix sums, values over anti-diagonals of blocks) and, for the code extraction alone, extract_chunked (64-bit
chunks, a summary per entry state, a scan, every chunk decoded on its own).
"""
import numpy as np

from motion_enc_ref import (SECTIONS, Motion, dc_prediction, global_prediction, mode_prediction, s16, split_prediction,
                            vector_prediction)
from schroedinger_amd import MV_DTYPE

M32 = 0xffffffff
A, D, F, S = range(4)           # code start, data bit, follow bit, sign bit
CHUNK = 64


class Bits:
    """The bits of `data`, MSB first; behind them every bit reads 1."""

    def __init__(self, data):
        self.data = bytes(data)
        self.nbits = 8 * len(self.data)
        self.pos = 0
        self.longs = 0

    def bit(self):
        p = self.pos
        self.pos += 1
        if p >= self.nbits:
            return 1
        return (self.data[p >> 3] >> (7 - (p & 7))) & 1

    def sync(self):
        self.pos = (self.pos + 7) & ~7

    def code(self, signed):
        """The value as 32 bits (a negative one as its two's complement)."""
        v, n = 1, 0
        while not self.bit():
            v = ((v << 1) | self.bit()) & M32
            n += 1
        self.longs += n >= 31
        m = (v - 1) & M32
        if signed and n and self.bit():
            m = -m & M32
        return m


def absent(num_refs, s):
    return num_refs < 2 and s in (4, 5)


def parse(data, num_refs):
    """The header walk: per section (first byte, kept bytes) or None, the truncated mask, `bytes`, the headers' long codes."""
    data = bytes(data)
    u = Bits(data)
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
        sections[s] = (first if kept else 0, kept)
        u.pos += 8 * length
    return sections, truncated, min((u.pos + 7) >> 3, len(data)), u.longs


def extract(payload, signed, ceiling):
    """The codes of a section that start in its payload, `ceiling` at most: (values, the position behind each, long codes)."""
    r = Bits(payload)
    values, ends = [], []
    while len(values) < ceiling and r.pos < r.nbits:
        values.append(r.code(signed))
        ends.append(r.pos)
    return values, ends, r.longs


class Section:
    """One VLC section as the walks see it: code i by index (0 behind the payload), the bits n codes were read for."""

    def __init__(self, payload, signed, ceiling):
        self.values, self.ends, self.longs = extract(payload, signed, ceiling)
        self.units = 0

    def value(self, i):
        return self.values[i] if i < len(self.values) else 0

    def take(self):
        self.units += 1
        return self.value(self.units - 1)

    def bits(self, n):
        if n == 0:
            return 0
        if n <= len(self.ends):
            return self.ends[n - 1]
        return (self.ends[-1] if self.ends else 0) + n - len(self.ends)


def _open(data, nbx, nby, num_refs):
    data = bytes(data)
    sections, truncated, nbytes, longs = parse(data, num_refs)
    payload = [b"" if sec is None else data[sec[0]:sec[0] + sec[1]] for sec in sections]
    vlc = {s: Section(payload[s], s != 0, nbx * nby // 16 if s == 0 else nbx * nby) for s in range(SECTIONS) if s != 1}
    return sections, truncated, nbytes, longs, payload, vlc


def _close(m, nbx, nby, num_refs, sections, truncated, nbytes, longs, vlc, mode_units, mode_bits):
    field = np.zeros(nbx * nby, MV_DTYPE)
    field["flags"] = [p | (g << 2) | (s << 3) for p, g, s in zip(m.pred_mode, m.using_global, m.split)]
    field["v"] = m.v
    units = [0] * SECTIONS
    bits = [0] * SECTIONS
    for s in range(SECTIONS):
        if absent(num_refs, s):
            continue
        units[s] = mode_units if s == 1 else vlc[s].units
        bits[s] = mode_bits if s == 1 else vlc[s].bits(vlc[s].units)
    kept = [0 if sec is None else sec[1] for sec in sections]
    bad = [k for k in range(nbx * nby) if m.pred_mode[k] == 0 and any(not -128 <= m.v[k][i] <= 127 for i in range(3))]
    result = {"bytes": nbytes, "section_bytes": kept, "section_units": units, "section_bits": [min(b, M32) for b in bits],
              "truncated": truncated,
              "overran": sum((bits[s] > 8 * kept[s]) << s for s in range(SECTIONS)),
              "not_consumed": sum((bits[s] + 8 <= 8 * kept[s]) << s for s in range(SECTIONS)),
              "long_codes": longs + sum(v.longs for v in vlc.values()),
              "unverified": len(bad), "first_unverified": bad[0] if bad else -1}
    return field, result


def _values(m, vlc, x, y, index=None):
    """The vectors or DCs of the unit at (x, y), its mode and global flag decided: residuals in turn (index None) or by
    index (ref-1 or DC, ref-2)."""
    k = m.at(x, y)
    get = (lambda s, which: vlc[s].take()) if index is None else (lambda s, which: vlc[s].value(index[which]))
    if m.pred_mode[k] == 0:
        pred = dc_prediction(m, x, y)
        m.v[k] = [s16(pred[i] + get(6 + i, 0)) for i in range(3)] + [0]
    elif not m.using_global[k]:
        v = [0, 0, 0, 0]
        for ref in range(2):
            if m.pred_mode[k] & (1 << ref):
                pred_x, pred_y = vector_prediction(m, x, y, 1 << ref)
                v[ref] = s16(pred_x + get(2 + 2 * ref, ref))
                v[2 + ref] = s16(pred_y + get(3 + 2 * ref, ref))
        m.v[k] = v
    else:
        m.v[k] = [0, 0, 0, 0]


def decode(data, nbx, nby, num_refs, have_global_motion):
    """(field, result) in the reference's order: superblock by superblock, nine readers in lockstep."""
    hg = int(bool(have_global_motion))
    sections, truncated, nbytes, longs, payload, vlc = _open(data, nbx, nby, num_refs)
    modes = Bits(payload[1])
    m = Motion(np.zeros(nbx * nby, MV_DTYPE), nbx, nby, num_refs, hg)
    mode_units = 0

    def copy(dst, src):
        m.pred_mode[dst], m.using_global[dst], m.split[dst], m.v[dst] = m.pred_mode[src], m.using_global[src], m.split[src], list(m.v[src])

    def prediction_unit(x, y):
        nonlocal mode_units
        k = m.at(x, y)
        mode_units += 1
        m.pred_mode[k] = mode_prediction(m, x, y) ^ modes.bit()
        if num_refs > 1:
            m.pred_mode[k] ^= modes.bit() << 1
        m.using_global[k] = 0
        if m.pred_mode[k] and hg:
            m.using_global[k] = global_prediction(m, x, y) ^ modes.bit()
        _values(m, vlc, x, y)

    for j in range(0, nby, 4):
        for i in range(0, nbx, 4):
            k = m.at(i, j)
            m.split[k] = (split_prediction(m, i, j) + vlc[0].take()) % 3
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
    return _close(m, nbx, nby, num_refs, sections, truncated, nbytes, longs, vlc, mode_units, modes.pos)


def diagonals(cols, rows):
    for d in range(cols + rows - 1):
        for y in range(max(0, d - (cols - 1)), min(d, rows - 1) + 1):
            yield d - y, y


def decode_wavefront(data, nbx, nby, num_refs, have_global_motion):
    """(field, result) in the phases of motion_dec.hip."""
    hg = int(bool(have_global_motion))
    sections, truncated, nbytes, longs, payload, vlc = _open(data, nbx, nby, num_refs)
    modes = Bits(payload[1])
    m = Motion(np.zeros(nbx * nby, MV_DTYPE), nbx, nby, num_refs, hg)
    nsbx, nsby = nbx // 4, nby // 4

    # 1. splits over anti-diagonals of superblocks: superblock k's residual is the k-th uint of section 0
    for sx, sy in diagonals(nsbx, nsby):
        m.split[m.at(4 * sx, 4 * sy)] = (split_prediction(m, 4 * sx, 4 * sy) + vlc[0].value(sy * nsbx + sx)) % 3
    vlc[0].units = nsbx * nsby
    # 2. every superblock's first unit
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

    # 3. modes: over anti-diagonals of blocks, unit n's bits at n * bits -- or, with global motion, in stream order
    nbits = 1 + (num_refs > 1)
    if not hg:
        for x, y in diagonals(nbx, nby):
            o = origin(x, y)
            if o is None:
                continue
            sp, step = o
            n = unit_first[(y >> 2) * nsbx + (x >> 2)] + (((y & 3) >> (2 - sp)) << sp) + ((x & 3) >> (2 - sp))
            modes.pos = n * nbits
            r = modes.bit()
            if num_refs > 1:
                r |= modes.bit() << 1
            m.pred_mode[m.at(x, y)] = mode_prediction(m, x, y) ^ r
            spread(x, y, sp, step)
        mode_bits = mode_units * nbits
    else:
        for x, y, sp, step in stream_units():
            k = m.at(x, y)
            m.pred_mode[k] = mode_prediction(m, x, y) ^ modes.bit()
            if num_refs > 1:
                m.pred_mode[k] ^= modes.bit() << 1
            m.using_global[k] = global_prediction(m, x, y) ^ modes.bit() if m.pred_mode[k] else 0
            spread(x, y, sp, step)
        mode_bits = modes.pos
    # 4. which code a unit owns: prefix counts in stream order
    count, index = [0, 0, 0], {}
    for x, y, sp, step in stream_units():
        k = m.at(x, y)
        mode, ug = m.pred_mode[k], m.using_global[k]
        index[k] = (count[2] if mode == 0 else count[0], count[1])
        count[0] += bool(mode & 1) and not ug
        count[1] += bool(mode & 2) and not ug
        count[2] += mode == 0
    for s in range(2, SECTIONS):
        vlc[s].units = 0 if absent(num_refs, s) else count[0 if s < 4 else 1 if s < 6 else 2]
    # 5. values over anti-diagonals of blocks
    for x, y in diagonals(nbx, nby):
        o = origin(x, y)
        if o is None:
            continue
        k = m.at(x, y)
        _values(m, vlc, x, y, index[k])
        for l in range(o[1]):
            for c in range(o[1]):
                m.v[m.at(x + c, y + l)] = list(m.v[k])
    return _close(m, nbx, nby, num_refs, sections, truncated, nbytes, longs, vlc, mode_units, mode_bits)


# ---- the chunk machine ---------------------------------------------------------------------------------------------------

def step(state, bit, signed):
    """(the next state, 1 if a code completed) for one bit."""
    if state == A:
        return (A, 1) if bit else (D, 0)
    if state == D:
        return F, 0
    if state == F:
        if not bit:
            return D, 0
        return (S, 0) if signed else (A, 1)
    return A, 1


def summary(r, chunk, signed):
    """Per entry state (the exit state, the codes completed) over the 64 bits of chunk `chunk` of reader r."""
    out = []
    for state in range(4):
        done = 0
        r.pos = CHUNK * chunk
        for _ in range(CHUNK):
            state, d = step(state, r.bit(), signed)
            done += d
        out.append((state, done))
    return out


def extract_chunked(payload, signed, ceiling):
    """extract's values, found as motion_dec.hip finds them: summaries, their scan, every chunk on its own.  Also the
    entry states met."""
    r = Bits(payload)
    nchunks = (len(payload) + 7) // 8
    sums = [summary(r, c, signed) for c in range(nchunks)]
    state, done, entries = A, 0, []
    for c in range(nchunks):
        entries.append((state, done + (state != A)))
        state, d = sums[c][state]
        done += d
    started = min(done + (state != A), ceiling)
    values = {}
    for c, (state, n) in enumerate(entries):
        r.pos = CHUNK * c
        while state != A and r.pos < CHUNK * (c + 1):
            state, _ = step(state, r.bit(), signed)
        if state != A:
            continue            # a code that started before covers the chunk
        while r.pos < CHUNK * (c + 1) and n < ceiling:
            assert n not in values
            values[n] = r.code(signed)
            n += 1
    assert sorted(values) == list(range(started)), (sorted(values)[:4], started)
    return [values[i] for i in range(started)], {e for e, _ in entries}
