"""Without a device: the host-only half of the arithmetic transform-data decoder's interface -- the refusals of
schro_hip_arith_decode_check (those of the VLC call), the scratch it asks for, the result block's layout."""
import ctypes as C

import numpy as np
import pytest

import schroedinger_amd as sa
from schroedinger_amd import _lib


class Plane:
    """An address with a geometry: the host-only calls dereference nothing."""

    def __init__(self, ptr, w, h, b, stride=None):
        self.ptr, self.width, self.height, self.stride = ptr, w, h, w * b if stride is None else stride


def entry(b=2, depth=2, w=32, h=16, data=1 << 20, nbytes=500, result=1 << 21, quant=False, hc=(1, 2, 3), vc=(1, 1, 2), mode=1, word=None):
    planes = [Plane((k + 4) << 22, w >> (k > 0), h >> (k > 0), b) for k in range(3)]
    qu = [Plane((k + 8) << 22, w >> (k > 0), h >> (k > 0), b) for k in range(3)] if quant else None
    return [data, nbytes, word, planes, qu, depth, list(hc), list(vc), mode, 0, 0, result]


def refused(pictures, b, match):
    with pytest.raises(sa.SchroHipError, match=match):
        sa.arith_decode_check([tuple(p) for p in pictures], b)


def test_accepted_and_scratch():
    a, c = entry(), entry(b=2, depth=0, hc=(1,), vc=(1,), data=3 << 20, result=(3 << 20) + 4096)
    for k in range(3):
        c[3][k].ptr += 1 << 26
    sa.arith_decode_check([tuple(a)], 2)
    sa.arith_decode_check([tuple(a), tuple(c)], 2)
    sa.arith_decode_check([tuple(entry(b=4, quant=True))], 4)
    # eight words per sub-band: 3 x 7 at depth 2, 3 x 1 at depth 0
    assert sa.arith_decode_scratch_words([tuple(a)], 2) == 8 * 21
    assert sa.arith_decode_scratch_words([tuple(a), tuple(c)], 2) == 8 * 24


def test_refusals_are_those_of_the_vlc_call():
    refused([entry()], 3, "bytes_per_sample must be 2 or 4")
    refused([entry(depth=7)], 2, "picture 0: transform_depth 7")
    refused([entry(w=30)], 2, "picture 0, component 0: 30 x 16 must be positive multiples of 4")
    refused([entry(hc=(1, 0, 3))], 2, "picture 0: 0 x 1 codeblocks at level 1")
    refused([entry(mode=2)], 2, "codeblock_mode_index 2")
    refused([entry(nbytes=1 << 29)], 2, "below 2\\^29")
    refused([entry(result=(1 << 21) + 2)], 2, "result is NULL or unaligned")
    refused([entry(word=(1 << 23) + 1)], 2, "bytes_on_device is unaligned")
    refused([entry(data=(4 << 22) + 8)], 2, "picture 0: data overlaps coeffs\\[0\\]")
    refused([entry(result=(5 << 22) + 8)], 2, "picture 0: result overlaps coeffs\\[1\\]")
    # the arithmetic result is 4 bytes longer than the VLC one: a plane that starts at its last word overlaps it
    size = C.sizeof(_lib.ArithDecodeResult)
    assert size == C.sizeof(_lib.NoarithDecodeResult) + 4
    refused([entry(result=(4 << 22) - size + 4)], 2, "result overlaps coeffs\\[0\\]")
    sa.arith_decode_check([tuple(entry(result=(4 << 22) - size))], 2)
    bad = entry()
    bad[3][1].stride = 30
    refused([bad], 2, "stride\\[1\\] 30 for 16 samples")
    second = entry(data=3 << 20, result=3 << 21)
    refused([entry(), second], 2, "picture 1: its coeffs overlaps the coeffs of picture 0")
    with pytest.raises(sa.SchroHipError):
        sa.arith_decode_scratch_words([tuple(entry(depth=9))], 2)


def test_result_block():
    r = _lib.ArithDecodeResult()
    r.bytes_read, r.error, r.first_error, r.compat_quant_offset, r.clamped_quant, r.bins = 7, 1, 40, 1, 3, 0xffffffff
    r.subband_length[2][18], r.subband_quant_index[1][4] = 1234, 60
    d = sa.arith_decode_result(r)
    assert (d["bytes_read"], d["error"], d["first_error"], d["compat_quant_offset"], d["clamped_quant"], d["bins"]) == (7, 1, 40, 1, 3, 0xffffffff)
    assert d["subband_length"][2, 18] == 1234 and d["subband_quant_index"][1, 4] == 60
    words = np.frombuffer(bytes(r), np.uint32)
    assert words.size == 82 and sa.arith_decode_result(words)["bins"] == 0xffffffff
    assert C.sizeof(_lib.ArithDecodePicture) == C.sizeof(_lib.NoarithDecodePicture) == 216
