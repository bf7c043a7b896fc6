"""A literal restatement of the reference's motion data of a noarith (VLC) picture, encoder and decoder.

Encoder: what schro_encoder_encode_picture appends between the prediction parameters and the transform parameters
(schroencoder.c:2505-2515): schro_encoder_encode_superblock_split, _prediction_modes, _vector_data (ref, xy) and _dc_data
(comp), :2841-3142, in their params->is_noarith branches, over schro_motion_dc_prediction (schromotion.c:163-210),
schro_motion_get_global_prediction (:213-239), schro_motion_vector_prediction (:315-368), schro_motion_split_prediction
(:371-399), schro_motion_get_mode_prediction (:402-430) and the bit writer of schropack.c:79-178 (noarith_enc_ref.Pack).
The reference's encoder cannot be built without liborc, so tests/test_motion_enc_ref.py pins this file with hand-derived
byte strings and with the round trip, and tests/test_noarith_twin.py with the noarith twin of the reference's own stream
(tests/noarith_twin.py, made without this file): `encode` writes the twin's bytes for all 96 inter pictures.  The stream
has split 2, full-pel vectors and no global motion only; the rest stays with the hand-derived strings.

Decoder: schro_decoder_parse_block_data, schro_decoder_decode_block_data / _decode_macroblock / _decode_prediction_unit
(schrodecoder.c:2525-2814) for noarith, with the bit reader of schrounpack.c (noarith_enc_ref.Unpack).

A field is a numpy array of MV_DTYPE records, x_num_blocks * y_num_blocks of them in raster order: flags = pred_mode |
using_global << 2 | split << 3, v = dx[0], dx[1], dy[0], dy[1] -- or dc[0 .. 2] in the same bytes.
"""
import numpy as np

from noarith_enc_ref import Pack, Unpack
from schroedinger_amd import MV_DTYPE

SECTIONS = 9
SECTION_NAMES = ["superblock split", "prediction modes", "ref-1 x", "ref-1 y", "ref-2 x", "ref-2 y", "dc Y", "dc U", "dc V"]


def s16(x):
    """(short) x / a store to an int16_t."""
    return ((int(x) + 32768) & 0xffff) - 32768


def divide3(a):
    """schro_divide3 (schroutils.h:64): ((a) * 21845 + 10922) >> 16, an arithmetic shift of an int."""
    return (a * 21845 + 10922) >> 16


class Motion:
    """The parts of SchroMotion / SchroParams the functions read, the records as Python lists."""

    def __init__(self, field, nbx, nby, num_refs, have_global_motion):
        assert field.dtype == MV_DTYPE and field.size == nbx * nby
        self.nbx, self.nby, self.num_refs, self.have_global_motion = nbx, nby, num_refs, int(bool(have_global_motion))
        flags = field["flags"].tolist()
        self.pred_mode = [f & 3 for f in flags]
        self.using_global = [(f >> 2) & 1 for f in flags]
        self.split = [(f >> 3) & 3 for f in flags]
        self.v = field["v"].tolist()          # dx[0], dx[1], dy[0], dy[1]; dc[i] = v[i]

    def at(self, x, y):
        return y * self.nbx + x               # SCHRO_MOTION_GET_BLOCK

    def dx(self, i, ref):
        return self.v[i][ref]

    def dy(self, i, ref):
        return self.v[i][2 + ref]


def dc_prediction(m, x, y):
    pred = [0, 0, 0]
    for i in range(3):
        total, n = 0, 0
        if x > 0:
            k = m.at(x - 1, y)
            if m.pred_mode[k] == 0:
                total += m.v[k][i]
                n += 1
        if y > 0:
            k = m.at(x, y - 1)
            if m.pred_mode[k] == 0:
                total += m.v[k][i]
                n += 1
        if x > 0 and y > 0:
            k = m.at(x - 1, y - 1)
            if m.pred_mode[k] == 0:
                total += m.v[k][i]
                n += 1
        if n == 0:
            pred[i] = 0
        elif n == 1:
            pred[i] = s16(total)
        elif n == 2:
            pred[i] = (total + 1) >> 1
        else:
            pred[i] = divide3(total + 1)
    return pred


def global_prediction(m, x, y):
    if x == 0 and y == 0:
        return 0
    if y == 0:
        return m.using_global[m.at(x - 1, 0)]
    if x == 0:
        return m.using_global[m.at(0, y - 1)]
    total = m.using_global[m.at(x - 1, y)] + m.using_global[m.at(x, y - 1)] + m.using_global[m.at(x - 1, y - 1)]
    return int(total >= 2)


def median3(a, b, c):
    if a < b:
        if b < c:
            return b
        if c < a:
            return a
        return c
    if a < c:
        return a
    if c < b:
        return b
    return c


def vector_prediction(m, x, y, mode):
    vx, vy = [], []
    where = []
    if x > 0:
        where.append(m.at(x - 1, y))
    if y > 0:
        where.append(m.at(x, y - 1))
    if x > 0 and y > 0:
        where.append(m.at(x - 1, y - 1))
    for k in where:
        if not m.using_global[k] and (m.pred_mode[k] & mode):
            vx.append(m.dx(k, mode - 1))
            vy.append(m.dy(k, mode - 1))
    n = len(vx)
    if n == 0:
        return 0, 0
    if n == 1:
        return vx[0], vy[0]
    if n == 2:
        return (vx[0] + vx[1] + 1) >> 1, (vy[0] + vy[1] + 1) >> 1
    return median3(*vx), median3(*vy)


def split_prediction(m, x, y):
    if y == 0:
        return 0 if x == 0 else m.split[m.at(x - 4, 0)]
    if x == 0:
        return m.split[m.at(x, y - 4)]
    total = m.split[m.at(x, y - 4)] + m.split[m.at(x - 4, y)] + m.split[m.at(x - 4, y - 4)]
    return (total + 1) // 3


def mode_prediction(m, x, y):
    if y == 0:
        return 0 if x == 0 else m.pred_mode[m.at(x - 1, 0)]
    if x == 0:
        return m.pred_mode[m.at(0, y - 1)]
    a, b, c = m.pred_mode[m.at(x - 1, y)], m.pred_mode[m.at(x, y - 1)], m.pred_mode[m.at(x - 1, y - 1)]
    return (a & b) | (b & c) | (c & a)


def units(m):
    """The coded units in stream order: superblocks in raster order, (l, k) in steps of 4 >> split of the top-left record.
    A split of 3 would not terminate in the reference (4 >> 3 == 0); it is walked as split 2."""
    for j in range(0, m.nby, 4):
        for i in range(0, m.nbx, 4):
            step = 4 >> min(m.split[m.at(i, j)], 2)
            for l in range(0, 4, step):
                for k in range(0, 4, step):
                    yield i + k, j + l


def verify(m):
    """schro_motion_verify (schromotion.c:441-525) without its early return: the raster indices of the blocks it rejects."""
    bad = []
    for y in range(m.nby):
        for x in range(m.nbx):
            k, sb = m.at(x, y), m.at(x & ~3, y & ~3)
            same = lambda a, b: (m.pred_mode[a], m.using_global[a], m.split[a], m.v[a]) == (m.pred_mode[b], m.using_global[b], m.split[b], m.v[b])
            wrong = m.split[k] != m.split[sb]
            if m.split[sb] == 0:
                wrong |= not same(k, sb)
            elif m.split[sb] == 1:
                wrong |= not same(k, m.at(x & ~1, y & ~1))
            if m.pred_mode[k] == 0:
                wrong |= any(not -128 <= m.v[k][i] <= 127 for i in range(3))
            elif m.pred_mode[k] >= 2:
                wrong |= m.num_refs < 2
            if not m.have_global_motion:
                wrong |= bool(m.using_global[k])
            if wrong:
                bad.append(k)
    return bad


def encode(field, nbx, nby, num_refs, have_global_motion):
    """(bytes, result): the bytes appended to a synchronised frame->pack and a dict like SchroHipMotionEncodeResult.
    schro_motion_vector_is_equal compares whole records; the metrics, which the stream does not carry, are compared in
    `unverified` too."""
    m = Motion(field, nbx, nby, num_refs, have_global_motion)
    section_bytes, section_units, asserted = [0] * SECTIONS, [0] * SECTIONS, 0
    frame_pack = Pack()

    def close(section, pack, count):
        frame_pack.sync()
        pack.flush()
        frame_pack.encode_uint(pack.get_offset())
        frame_pack.sync()
        frame_pack.append(pack.data)
        section_bytes[section], section_units[section] = pack.get_offset(), count

    # schro_encoder_encode_superblock_split
    pack, count = Pack(), 0
    for j in range(0, nby, 4):
        for i in range(0, nbx, 4):
            split = m.split[m.at(i, j)]
            asserted += split >= 3            # SCHRO_ASSERT (mv->split < 3)
            pack.encode_uint((split - split_prediction(m, i, j) + 3) % 3)
            count += 1
    close(0, pack, count)

    # schro_encoder_encode_prediction_modes
    pack, count = Pack(), 0
    for x, y in units(m):
        k = m.at(x, y)
        pred_mode = m.pred_mode[k] ^ mode_prediction(m, x, y)
        pack.encode_bit(pred_mode & 1)
        if num_refs > 1:
            pack.encode_bit(pred_mode >> 1)
        if m.pred_mode[k] != 0:
            if m.have_global_motion:
                pack.encode_bit(m.using_global[k] ^ global_prediction(m, x, y))
            else:
                asserted += m.using_global[k] != 0   # SCHRO_ASSERT (mv->using_global == FALSE)
        count += 1
    close(1, pack, count)

    # schro_encoder_encode_vector_data (ref, xy)
    for ref in range(num_refs):
        for xy in range(2):
            pack, count = Pack(), 0
            for x, y in units(m):
                k = m.at(x, y)
                if (m.pred_mode[k] & (1 << ref)) and not m.using_global[k]:
                    pred_x, pred_y = vector_prediction(m, x, y, 1 << ref)
                    pack.encode_sint(m.dx(k, ref) - pred_x if xy == 0 else m.dy(k, ref) - pred_y)
                    count += 1
            close(2 + 2 * ref + xy, pack, count)

    # schro_encoder_encode_dc_data (comp)
    for comp in range(3):
        pack, count = Pack(), 0
        for x, y in units(m):
            k = m.at(x, y)
            if m.pred_mode[k] == 0:
                pack.encode_sint(m.v[k][comp] - dc_prediction(m, x, y)[comp])
                count += 1
        close(6 + comp, pack, count)

    bad = verify(m)
    metrics = np.flatnonzero(unequal_metrics(field, m))
    bad = sorted(set(bad) | set(metrics.tolist()))
    data = bytes(frame_pack.data)
    return data, {"bytes": len(data), "section_bytes": section_bytes, "section_units": section_units, "asserted": int(asserted),
                  "unverified": len(bad), "first_unverified": bad[0] if bad else -1}


def unequal_metrics(field, m):
    """Blocks of split-0 / split-1 superblocks whose metric, chroma metric or upper flag bits differ from their origin's."""
    nbx, nby = m.nbx, m.nby
    rest = np.stack([field["flags"] >> 5, field["metric"], field["chroma_metric"]], axis=1).reshape(nby, nbx, 3)
    ys, xs = np.mgrid[0:nby, 0:nbx]
    split = ((field["flags"] >> 3) & 3).reshape(nby, nbx)[ys & ~3, xs & ~3]
    oy = np.where(split == 0, ys & ~3, np.where(split == 1, ys & ~1, ys))
    ox = np.where(split == 0, xs & ~3, np.where(split == 1, xs & ~1, xs))
    return (rest != rest[oy, ox]).any(axis=2).reshape(-1)


def section_of(data, num_refs, byte):
    """The section byte `byte` of an encoded picture lies in, as a name (for messages)."""
    u = Unpack(data)
    for s in range(SECTIONS):
        if num_refs < 2 and s in (4, 5):
            continue
        u.byte_sync()
        length = u.decode_uint()
        u.byte_sync()
        end = (u.pos >> 3) + length
        if byte < end:
            return SECTION_NAMES[s]
        u.pos = 8 * end
    return "past the last section"


def decode(data, nbx, nby, num_refs, have_global_motion):
    """schro_decoder_parse_block_data + schro_decoder_decode_block_data: the field the bytes decode to."""
    have_global_motion = int(bool(have_global_motion))
    u = Unpack(data)
    unpack = [None] * SECTIONS
    for s in range(SECTIONS):
        if num_refs < 2 and s in (4, 5):
            continue
        u.byte_sync()
        length = u.decode_uint()
        u.byte_sync()
        start = u.pos >> 3
        unpack[s] = Unpack(data[start:start + length])
        u.pos = 8 * (start + length)
    field = np.zeros(nbx * nby, MV_DTYPE)
    m = Motion(field, nbx, nby, num_refs, have_global_motion)

    def copy(dst, src):
        m.pred_mode[dst], m.using_global[dst], m.split[dst], m.v[dst] = m.pred_mode[src], m.using_global[src], m.split[src], list(m.v[src])

    def prediction_unit(x, y):
        k = m.at(x, y)
        m.pred_mode[k] = mode_prediction(m, x, y)
        m.pred_mode[k] ^= unpack[1].decode_bit()
        if num_refs > 1:
            m.pred_mode[k] ^= unpack[1].decode_bit() << 1
        if m.pred_mode[k] == 0:
            pred = dc_prediction(m, x, y)
            for i in range(3):
                m.v[k][i] = s16(pred[i] + unpack[6 + i].decode_sint())
        else:
            if have_global_motion:
                m.using_global[k] = global_prediction(m, x, y) ^ unpack[1].decode_bit()
            else:
                m.using_global[k] = 0
            if not m.using_global[k]:
                for ref in range(2):
                    if m.pred_mode[k] & (1 << ref):
                        pred_x, pred_y = vector_prediction(m, x, y, 1 << ref)
                        m.v[k][ref] = s16(pred_x + unpack[2 + 2 * ref].decode_sint())
                        m.v[k][2 + ref] = s16(pred_y + unpack[3 + 2 * ref].decode_sint())
            else:
                m.v[k] = [0, 0, 0, 0]

    for j in range(0, nby, 4):
        for i in range(0, nbx, 4):
            k = m.at(i, j)
            m.split[k] = (split_prediction(m, i, j) + unpack[0].decode_uint()) % 3
            if m.split[k] == 0:
                prediction_unit(i, j)
                for l in range(4):
                    for c in range(4):
                        if l or c:
                            copy(m.at(i + c, j + l), k)
            elif m.split[k] == 1:
                for l in (0, 2):
                    for c in (0, 2):
                        o = m.at(i + c, j + l)
                        m.split[o] = 1
                        prediction_unit(i + c, j + l)
                        copy(m.at(i + c + 1, j + l), o)
                    # memcpy (mv + x_num_blocks, mv, 4 * sizeof (*mv)) after both units of the row
                    for c in range(4):
                        copy(m.at(i + c, j + l + 1), m.at(i + c, j + l))
            else:
                for l in range(4):
                    for c in range(4):
                        m.split[m.at(i + c, j + l)] = 2
                        prediction_unit(i + c, j + l)
    field["flags"] = [p | (g << 2) | (s << 3) for p, g, s in zip(m.pred_mode, m.using_global, m.split)]
    field["v"] = m.v
    return field


def canonical(field):
    """What a stream carries of a field: the flags (mode, global, split) and the slots the block's mode uses -- three DCs,
    or the vector of each reference the mode names unless the block is global --, everything else zero."""
    out = np.zeros(field.size, MV_DTYPE)
    flags = field["flags"] & 31
    mode, ug = flags & 3, (flags >> 2) & 1
    out["flags"] = flags
    v = np.zeros((field.size, 4), np.int16)
    dc = mode == 0
    v[dc, :3] = field["v"][dc, :3]
    for ref in range(2):
        use = ((mode >> ref) & 1 == 1) & (ug == 0)
        v[use, ref] = field["v"][use, ref]
        v[use, 2 + ref] = field["v"][use, 2 + ref]
    out["v"] = v
    return out
