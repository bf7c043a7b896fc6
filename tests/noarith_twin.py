"""The noarith (VLC) twin of the reference's own stream.  TEST INFRASTRUCTURE; reads committed files only.

tests/golden/test_stream.drc is arithmetic-coded.  For motion data the arithmetic and the VLC syntax share everything but
the entropy coder -- the nine sections, the order of units, the split, mode, vector and DC predictions; only arith[i]
against unpack[i] differs (schrodecoder.c:2525-2814) -- so the values the nine arithmetic decoders yield, written as
exp-Golomb codes and framed as schroencoder.c:2505-2515 frames them, are the motion data the reference's encoder would
have written for the same picture with is_noarith set.  Those values are recorded by oracle/dirac_stream.py
(Decoder.decode_block_data, log=), whose predictions the reference decoder's frame digests hold
(tests/golden/stream_md5.json); tests/motion_enc_ref.py and tests/motion_dec_ref.py take no part in making the twin, so
the twin pins them (tests/test_noarith_twin.py).

The transform twin is the stream's quantised planes through noarith_dec_ref.write_transform_data with the picture's own
codeblock counts, codeblock mode and sub-band quant indices, for a decoder in the compat state the stream's decoder is in
in front of the picture: a VLC decoder must read the stream's coefficients back from it.

  motion_pictures   every inter picture's motion twin without the coefficient decode (parse + block data: 5 to 9 s for all 96)
  pictures          every picture in coded order with both twins and what stream_lib.decode_stream yields (0.3 s each)
Both cache what they made, so the tests of a session share it; records are never changed.
"""
import noarith_dec_ref as dec_ref
import noarith_enc_ref as enc
import oracle_lib as O
import stream_lib as S

D = S.D
SECTIONS = 9
SPLIT, MODES = 0, 1


def motion_twin(pic, log):
    """(bytes, section_bytes (9)): per section the picture has, the recorded values as VLC codes -- uint for the splits, a
    bit per mode bit, sint for the residuals -- flushed and appended to the synchronised frame pack as
    schro_encoder_encode_superblock_split ... _dc_data do for is_noarith: sync, uint (length), sync, payload."""
    frame = enc.Pack()
    section_bytes = [0] * SECTIONS
    for s in range(SECTIONS):
        if pic.motion_buffers[s] is None:
            assert not log[s]
            continue
        pack = enc.Pack()
        write = pack.encode_uint if s == SPLIT else pack.encode_bit if s == MODES else pack.encode_sint
        for v in log[s]:
            write(int(v))
        frame.sync()
        pack.flush()
        frame.encode_uint(pack.get_offset())
        frame.sync()
        frame.append(pack.data)
        section_bytes[s] = pack.get_offset()
    return bytes(frame.data), section_bytes


def quant_indices(pic):
    """[component][index]: the quant index of the sub-band's header (0 where the stream codes the sub-band as zero)."""
    return [[q for q, _ in pic.subbands[k]] for k in range(3)]


def transform_twin(pic, quant, codeblocks, compat):
    """The transform data of the picture for a VLC decoder in state `compat`: quant -- the stream's quantised planes,
    codeblocks -- dirac_stream's records of them.  The stream codes no quant offset but 0 (every record carries its
    sub-band's index), so the writer's default offsets are the stream's."""
    qidx = quant_indices(pic)
    for k in range(3):
        for (index, x0, y0, x1, y1, zero, q) in codeblocks[k]:
            assert q == qidx[k][index], "a quant offset in the stream: component %d sub-band %d" % (k, index)
    data, _ = dec_ref.write_transform_data(quant, pic.depth, pic.horiz_cb, pic.vert_cb, pic.cb_mode, compat, qidx)
    return data


def parameters(pic, compat=None):
    """What a decoder is told about the picture."""
    P = dict(number=pic.number, num_refs=pic.num_refs, refs=list(pic.refs))
    if pic.num_refs:
        P.update(nbx=pic.x_num_blocks, nby=pic.y_num_blocks, blocks=(pic.xblen, pic.yblen, pic.xbsep, pic.ybsep),
                 mv_precision=pic.mv_precision)
    if not pic.zero_residual:
        P.update(depth=pic.depth, wavelet=pic.wavelet, horiz_cb=list(pic.horiz_cb), vert_cb=list(pic.vert_cb), cb_mode=pic.cb_mode,
                 compat=int(bool(compat)), is_intra=int(pic.num_refs == 0), iwt=list(pic.iwt))
    return P


# ---- motion only ------------------------------------------------------------------------------------------------------------

_parsed = []            # [Picture] of the inter pictures in coded order, parsed once
_motion = {}            # picture number -> record


def _decoder():
    tables = S.load_tables()
    qf, qo12 = O.quant_tables()
    return D.Decoder(tables["arith_lut"], qf, qo12, tables["schro_table_offset_3_8"])


def _parse():
    if not _parsed:
        dec = _decoder()
        for code, payload in D.parse_units(S.load_stream()):
            if code == 0x00:
                dec.fmt = D.parse_sequence_header(payload)
            elif code & 8:
                pic = dec.parse_picture(code, payload)
                if pic.num_refs:
                    _parsed.append(pic)
    return _parsed


def motion_numbers():
    """The numbers of the inter pictures in coded order."""
    return [pic.number for pic in _parse()]


def motion_pictures(numbers=None, limit=None):
    """Per inter picture in coded order (those of `numbers`, `limit` at most) a dict: number, num_refs, refs, nbx, nby,
    blocks, mv_precision, mv (the stream's field), log (the recorded values), motion (the twin's bytes), section_bytes.
    Parse and block data only: no coefficient is decoded."""
    n = 0
    for pic in _parse():
        if numbers is not None and pic.number not in numbers:
            continue
        if limit is not None and n >= limit:
            return
        if pic.number not in _motion:
            log = [[] for _ in range(SECTIONS)]
            mv = _decoder().decode_block_data(pic, log)
            data, section_bytes = motion_twin(pic, log)
            _motion[pic.number] = dict(parameters(pic), mv=mv, log=log, motion=data, section_bytes=section_bytes)
        yield _motion[pic.number]
        n += 1


# ---- everything ---------------------------------------------------------------------------------------------------------------

_records = []
_source = []


def _next_record():
    if not _source:
        _source.append(S.decode_stream(S.load_stream(), S.load_tables(), quantised=True, detail=True))
    rec = next(_source[0])
    pic = rec["picture"]
    rec["twin"] = parameters(pic, rec["compat"])
    if pic.num_refs:
        rec["motion"], rec["section_bytes"] = motion_twin(pic, rec["motion_log"])
    if not pic.zero_residual:
        rec["transform"] = transform_twin(pic, rec["quant"], rec["codeblocks"], rec["compat"])
        rec["quant_indices"] = quant_indices(pic)
    return rec


def pictures(limit=None):
    """Per picture in coded order what stream_lib.decode_stream yields (number, refs, mv, params, quant, codeblocks, coeffs,
    out, md5 ...) and: twin -- `parameters`; motion, section_bytes -- the motion twin (inter pictures); transform -- the
    transform twin's bytes; quant_indices.  Stops after `limit` pictures; what was decoded stays for the next caller."""
    n = 0
    while limit is None or n < limit:
        if n == len(_records):
            try:
                _records.append(_next_record())
            except StopIteration:
                return
        yield _records[n]
        n += 1


# ---- the pictures the GPU tests take, by number; tests/test_noarith_twin.py asserts that they are what they are named for ------

# the first one-reference and the first two-reference picture; the most mode-2 blocks, the most mode-3 blocks, the largest
# |v|; the longest and the shortest motion twin; the last picture -- each the first in coded order that holds the extreme
# and is not yet in the list
MOTION_EIGHT = [3, 1, 41, 2, 4, 30, 7, 98]
# the first 12 pictures in coded order: one intra picture, three one-reference pictures, eight two-reference pictures
FIRST_TWELVE = [0, 3, 1, 2, 7, 4, 5, 6, 11, 8, 9, 10]
