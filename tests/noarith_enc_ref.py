"""A literal restatement of the reference's VLC (noarith) core-syntax transform data, encoder and decoder.

Encoder: schro_encoder_encode_transform_data (schroencoder.c:3462-3483) over schro_encoder_encode_subband_noarith
(:4072-4192) WITHOUT its quantiser call -- the quant planes are the input --, schro_frame_data_is_zero (:4043-4070,
orc_accw: absw then accw, 16-bit), schro_frame_data_get_codeblock (schroframe.c:1865-1886), schro_subband_get_frame_data
(schroparams.c:319-352) and the bit writer of schropack.c:60-178.  The reference's encoder cannot be built without
liborc, so tests/test_noarith_enc_ref.py pins this file with hand-derived byte strings and with the round trip.

Decoder: schro_decoder_decode_subband / _decode_codeblock_noarith (schrodecoder.c:3355-3600) with the bit reader of
schrounpack.c (a read past the end gives 1-bits).  It reads a zero flag and a quant offset exactly where the ENCODER writes
one (schro_decoder_setup_codeblocks decides both without looking at the sub-band index or the codeblock count).

Planes are numpy arrays of the transform's size in the reference's in-place layout: sub-band `index` of a depth-d
transform is plane[r0::step, c0:c0 + bw] with step = 1 << shift.
"""
import numpy as np

MAX_SUBBANDS = 19


class Pack:
    """schropack.c: schro_pack_encode_init .. schro_pack_encode_sint."""

    def __init__(self):
        self.data = bytearray()
        self.value = 0
        self.shift = 7

    def get_offset(self):
        return len(self.data)

    def _shift_out(self):
        self.data.append(self.value)
        self.value = 0
        self.shift = 7

    def sync(self):
        if self.shift != 7:
            self._shift_out()

    flush = sync

    def append(self, data):
        assert self.shift == 7, "appending to unsyncronized pack"
        self.data += data

    def encode_bit(self, value):
        value &= 1
        self.value |= value << self.shift
        self.shift -= 1
        if self.shift < 0:
            self._shift_out()

    def encode_uint(self, value):
        value += 1
        n_bits = value.bit_length()             # maxbit
        for i in range(n_bits - 1):
            self.encode_bit(0)
            self.encode_bit((value >> (n_bits - 2 - i)) & 1)
        self.encode_bit(1)

    def encode_sint(self, value):
        value = int(value)
        sign = 0
        if value < 0:
            sign = 1
            value = -value
        self.encode_uint(value)
        if value:
            self.encode_bit(sign)


class Unpack:
    """schrounpack.c with guard bit 1."""

    def __init__(self, data):
        self.data = bytes(data)
        self.pos = 0

    def decode_bit(self):
        byte = self.pos >> 3
        bit = 1 if byte >= len(self.data) else (self.data[byte] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return bit

    def decode_uint(self):
        value = 1
        while not self.decode_bit():
            value = (value << 1) | self.decode_bit()
        return value - 1

    def decode_sint(self):
        value = self.decode_uint()
        if value and self.decode_bit():
            value = -value
        return value

    def byte_sync(self):
        self.pos = (self.pos + 7) & ~7


def position_of(index):
    """schro_subband_get_position."""
    return 0 if index == 0 else (((index - 1) // 3) << 2) | ((index - 1) % 3 + 1)


def subband(plane, depth, index):
    """schro_subband_get_frame_data: the view of sub-band `index` in a plane of the transform's size."""
    position = position_of(index)
    shift = depth - (position >> 2)
    h, w = plane.shape
    bw, bh = w >> shift, h >> shift
    r0 = (1 << shift) >> 1 if position & 2 else 0
    c0 = bw if position & 1 else 0
    return plane[r0::1 << shift, c0:c0 + bw][:bh]


def codeblock_counts(index, horiz_codeblocks, vert_codeblocks):
    """schroencoder.c:4113-4121: entry [0] for sub-band 0, [SCHRO_SUBBAND_SHIFT (position) + 1] else."""
    if index == 0:
        return horiz_codeblocks[0], vert_codeblocks[0]
    level = position_of(index) >> 2
    return horiz_codeblocks[level + 1], vert_codeblocks[level + 1]


def get_codeblock(fd, x, y, hc, vc):
    """schro_frame_data_get_codeblock."""
    h, w = fd.shape
    xmin, xmax = (w * x) // hc, (w * (x + 1)) // hc
    ymin, ymax = (h * y) // vc, (h * (y + 1)) // vc
    return fd[ymin:ymax, xmin:xmax]


def is_zero(fd):
    """schro_frame_data_is_zero: s32 the true test; s16 per row the 16-bit sum of the 16-bit abs (abs (-32768) stays -32768)."""
    if fd.dtype == np.int32:
        return not np.any(fd != 0)
    for row in fd:
        acc = 0
        for v in row.tolist():
            acc = (acc + ((-v if v < 0 else v) & 0xffff)) & 0xffff
        if acc != 0:
            return False
    return True


def flags_of(index, hc, vc, codeblock_mode_index):
    """have_zero_flags, have_quant_offset (schroencoder.c:4122-4136: the encoder's rules)."""
    many = hc > 1 or vc > 1
    return many and index > 0, many and codeblock_mode_index == 1


def encode_subband(pack, qd, index, hc, vc, codeblock_mode_index, quant_index, stats):
    """schro_encoder_encode_subband_noarith behind its quantiser call; quant_index: that of codeblock (0, 0)."""
    if is_zero(qd):
        if np.any(qd != 0):
            stats["false_zero_subbands"] += 1
        pack.encode_uint(0)
        return
    sub = Pack()
    have_zero_flags, have_quant_offset = flags_of(index, hc, vc, codeblock_mode_index)
    for y in range(vc):
        for x in range(hc):
            cb = get_codeblock(qd, x, y, hc, vc)
            if have_zero_flags:
                zero_codeblock = is_zero(cb)
                sub.encode_bit(1 if zero_codeblock else 0)
                if zero_codeblock:
                    if np.any(cb != 0):
                        stats["false_zero_codeblocks"] += 1
                    continue
            if have_quant_offset:
                sub.encode_sint(0)
            for row in cb:
                for v in row.tolist():
                    sub.encode_sint(v)
    sub.flush()
    pack.encode_uint(sub.get_offset())
    if sub.get_offset() > 0:
        pack.encode_uint(quant_index)
        pack.sync()
        pack.append(sub.data)


def encode_transform_data(planes, depth, horiz_codeblocks, vert_codeblocks, codeblock_mode_index, quant_indices):
    """schro_encoder_encode_transform_data for is_noarith from a synchronised pack, plus the final sync.
    planes: Y, U, V quant planes; quant_indices[component][index]: the quant index of the sub-band's codeblock (0, 0).
    Returns (bytes, subband_bits (3 x 19), {"false_zero_codeblocks", "false_zero_subbands"})."""
    pack = Pack()
    bits = np.zeros((3, MAX_SUBBANDS), np.int64)
    stats = {"false_zero_codeblocks": 0, "false_zero_subbands": 0}
    for component in range(3):
        for i in range(1 + 3 * depth):
            pack.sync()
            bits[component, i] = -pack.get_offset() * 8
            hc, vc = codeblock_counts(i, horiz_codeblocks, vert_codeblocks)
            encode_subband(pack, subband(planes[component], depth, i), i, hc, vc, codeblock_mode_index,
                           int(quant_indices[component][i]), stats)
            bits[component, i] += pack.get_offset() * 8
    pack.sync()
    return bytes(pack.data), bits, stats


def decode_transform_data(data, shapes, dtype, depth, horiz_codeblocks, vert_codeblocks, codeblock_mode_index):
    """The quant planes and the quant index of every codeblock back from the bytes.  shapes: (height, width) per
    component.  Returns (planes, quant_indices[component][index] -- a (vc, hc) array, None for a zero sub-band --, bytes read)."""
    un = Unpack(data)
    planes = [np.zeros(s, dtype) for s in shapes]
    indices = [[None] * (1 + 3 * depth) for _ in range(3)]
    for component in range(3):
        for i in range(1 + 3 * depth):
            un.byte_sync()
            length = un.decode_uint()
            if length == 0:
                continue                # schro_decoder_zero_block over the sub-band
            quant_index = un.decode_uint()
            un.byte_sync()
            first = un.pos >> 3
            sub = Unpack(data[first:first + length])
            un.pos += 8 * length
            fd = subband(planes[component], depth, i)
            hc, vc = codeblock_counts(i, horiz_codeblocks, vert_codeblocks)
            have_zero_flags, have_quant_offset = flags_of(i, hc, vc, codeblock_mode_index)
            qis = np.zeros((vc, hc), np.int64)
            for y in range(vc):
                for x in range(hc):
                    cb = get_codeblock(fd, x, y, hc, vc)
                    qis[y, x] = quant_index
                    if have_zero_flags and sub.decode_bit():
                        continue
                    if have_quant_offset:
                        quant_index = min(max(quant_index + sub.decode_sint(), 0), 60)
                        qis[y, x] = quant_index
                    for r in range(cb.shape[0]):
                        for c in range(cb.shape[1]):
                            cb[r, c] = sub.decode_sint()
            indices[component][i] = qis
    un.byte_sync()
    return planes, indices, un.pos >> 3
