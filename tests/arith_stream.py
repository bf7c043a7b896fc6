"""The transform data of the reference stream's pictures as the bytes a decoder is handed.  TEST INFRASTRUCTURE; reads
committed files only.

oracle/dirac_stream.py parses a picture into Picture.subbands -- per component and sub-band (quant index, payload).  The
transform data is put together again from them as schro_decoder_parse_transform_data reads it: per sub-band sync, uint
(length), uint (quant index) when the length is not 0, sync (ZERO padding bits), the payload; one sync at the end.
tests/test_arith_dec_ref.py asserts that for every picture these bytes are exactly the tail of the parse unit's payload, so
what the device tests feed is the stream's own bytes and not a reconstruction."""
import noarith_enc_ref as enc
import noarith_twin as T
import stream_lib as S

D = S.D


def serialise(pic):
    """The transform data of a parsed dirac_stream.Picture."""
    pack = enc.Pack()
    for component in range(3):
        for q, payload in pic.subbands[component]:
            pack.sync()
            pack.encode_uint(len(payload))
            if len(payload):
                pack.encode_uint(q)
                pack.sync()
                pack.append(payload)
    pack.sync()
    return bytes(pack.data)


def units():
    """(parsed Picture, parse unit payload) of every picture with a residual, in coded order; no coefficient is decoded."""
    dec = T._decoder()
    for code, payload in D.parse_units(S.load_stream()):
        if code == 0x00:
            dec.fmt = D.parse_sequence_header(payload)
        elif code & 8:
            pic = dec.parse_picture(code, payload)
            if not pic.zero_residual:
                yield pic, payload


_records = {}


def pictures(limit=None):
    """A copy of each of noarith_twin.pictures' records (coded order, cached, never changed) with "arith": the picture's
    transform data as the stream holds it."""
    for rec in T.pictures(limit):
        n = rec["number"]
        if n not in _records:
            _records[n] = dict(rec, arith=None if rec["zero_residual"] else serialise(rec["picture"]))
        yield _records[n]


def entry(rec, data, nbytes, coeffs, quant, result, on_device=None, compat=None):
    """The twelve entries of schroedinger_amd.arith_decode_pictures for a record."""
    P = rec["twin"]
    return (data, nbytes, on_device, coeffs, quant, P["depth"], P["horiz_cb"], P["vert_cb"], P["cb_mode"], P["is_intra"],
            P["compat"] if compat is None else compat, result)
