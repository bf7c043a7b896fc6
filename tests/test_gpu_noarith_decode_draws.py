"""GPU: schro_hip_noarith_decode_batch on the drawn geometries, their damaged twins and the scan's scale cases of
tests/noarith_dec_draws.py, against tests/noarith_dec_ref.py bit for bit -- coefficient planes, quant planes, the whole
result block -- between guard blocks, as tests/test_gpu_noarith_decode.py runs the named cases (run_guarded is its).  What
the lists contain -- depths to 6 with both sample sizes, codeblocks of no size, the compat test firing, clamped indices,
every counter raised by some damage, scans of one, two and three steps that find and that run out -- is asserted on the
CPU by tests/test_noarith_dec_draws.py."""
import numpy as np
import pytest

import noarith_dec_cases as DC
import noarith_dec_draws as DD
import test_gpu_noarith_decode as T

pytestmark = pytest.mark.gpu

DAMAGED = [c for kind in DD.KINDS for c in DD.DAMAGED[kind]]


def with_quant(n):
    """a sixth of the cases, by index, run without quant planes"""
    return n % 6 != 5


@pytest.mark.parametrize("name", [c.name for c in DD.DRAWS])
def test_draws_are_the_reference_bit_for_bit(ctx, name):
    n = DD.DRAWS.index(DD.BY_NAME[name])
    T.run_guarded(ctx, [DD.DRAWS[n]], [n % 4], pad=n % 3, with_quant=with_quant(n))


@pytest.mark.parametrize("name", [c.name for c in DAMAGED])
def test_damaged_draws_are_defined(ctx, name):
    n = DAMAGED.index(DD.BY_NAME[name])
    T.run_guarded(ctx, [DAMAGED[n]], [(n + 1) % 4], pad=(n + 1) % 3, with_quant=with_quant(n))


@pytest.mark.parametrize("name", [c.name for c in DD.SCALE])
def test_scan_steps_on_damaged_payloads(ctx, name):
    n = DD.SCALE.index(DD.BY_NAME[name])
    T.run_guarded(ctx, [DD.SCALE[n]], [(n + 2) % 4], pad=(n + 2) % 3, with_quant=with_quant(n))


# ---- eight unlike pictures in one call ----------------------------------------------------------------------------------------

def batch_of(bpp, which):
    """Eight pictures of one sample size: an error picture -- first (which 0) or last (which 1) --, intact draws of depths 0,
    6 and 3, three damaged draws that decode, one scale stream."""
    mine = lambda cases: [c for c in cases if c.dtype.itemsize == bpp]
    error = lambda c: c.expected()[2]["error"]
    intact = mine(DD.DRAWS)
    at = lambda depth: [c for c in intact if c.depth == depth][which]
    bad = [c for c in mine(DD.DAMAGED["flip-anywhere"]) if error(c)][which]
    hurt = [[c for c in mine(DD.DAMAGED[kind]) if not error(c)][3 * which + j] for j, kind in enumerate(("flip-payload", "cut", "pattern"))]
    scale = [c for c in mine(DD.SCALE) if c.name.endswith(("-00", "-cut-in-codeblock-1"))][-which]
    cases = [bad, at(0), hurt[0], at(6), hurt[1], scale, hurt[2], at(3)]
    return cases[::-1] if which else cases


@pytest.mark.parametrize("which", [0, 1], ids=["error-first", "error-last"])
@pytest.mark.parametrize("bpp", [2, 4])
def test_eight_unlike_pictures_in_one_call(ctx, bpp, which):
    """lane_x and fill_x are maxima over the call's pictures and chunk_first accumulates over them: pictures of 1 and of 57
    sub-bands, of a few chunks and of more than a thousand, and one the header walk refuses, in one call."""
    cases = batch_of(bpp, which)
    errors = [c.expected()[2]["error"] for c in cases]
    assert sum(errors) == 1 and errors[-1 if which else 0] == 1
    assert len({c.name for c in cases}) == 8 and len({(tuple(c.sizes), c.depth) for c in cases}) >= 6
    assert {0, 6} <= {c.depth for c in cases}
    T.run_guarded(ctx, cases, [(n + which) % 4 for n in range(8)], pad=1 + which)


# ---- the length on the device -------------------------------------------------------------------------------------------------

def word_case(bpp):
    """an intact draw of middling size"""
    mine = sorted((c for c in DD.DRAWS if c.dtype.itemsize == bpp), key=lambda c: len(c.data))
    return mine[len(mine) // 2]


def length_words(case):
    bands = DC.split(case.data, 3 * case.nsub)
    big = max(range(len(bands)), key=lambda j: bands[j][0])
    length, qi, payload = bands[big]
    header = len(DC.join(bands[:big]))                          # the first byte of the longest payload's header
    first = len(DC.join(bands[:big] + [(length, qi, b"")]))      # ... and of the payload
    assert length >= 128 and first - header >= 3                 # (the length alone takes two bytes)
    n = len(case.data)
    return {"len-1": n - 1, "in-payload": first + length // 2, "in-header": header + 1, "zero": 0, "len": n, "len+1000": n + 1000}


@pytest.mark.parametrize("word", ["len-1", "in-payload", "in-header", "zero", "len", "len+1000"])
@pytest.mark.parametrize("bpp", [2, 4])
def test_length_word_on_the_device(ctx, bpp, word):
    """bytes_on_device: the call reads min(word, data_bytes) bytes -- a word that cuts the last byte, a payload, a header,
    everything; the whole input; and a word beyond data_bytes, for which data_bytes holds.  The word lies in the guarded
    block without a footprint: it keeps its value."""
    case = word_case(bpp)
    value = length_words(case)[word]
    want = T.expected_with_word(case, value)[2]
    assert want["error"] == 0
    if word in ("len", "len+1000"):
        assert all(np.array_equal(want[k], case.expected()[2][k]) for k in want)
    elif word == "zero":
        assert not want["subband_length"].any() and want["bytes_read"] == 3 * case.nsub      # every header reads guard bits
    else:
        assert want["truncated"] == 1
    T.run_guarded(ctx, [case], [bpp], pad=1, words=[value])


# ---- quantise -> encode -> decode at depths 4, 5 and 6 -------------------------------------------------------------------------

def round_trip_pictures():
    """(sizes, depth, hc, vc, mode) of the first draw of each depth 4 .. 6 with one codeblock in sub-band 0: with compat on,
    the encoder's and the decoder's rules agree there."""
    out = []
    for depth in (4, 5, 6):
        c = next(c for c in DD.DRAWS if c.depth == depth and c.counts(0) == (1, 1))
        out.append((c.sizes, c.depth, c.hc, c.vc, c.mode))
    return out


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_deep_chain_quantise_encode_decode_without_a_host_wait(ctx, dtype):
    """The three geometries in one call each of quantise_batch, noarith_encode_batch and noarith_decode_batch on one queue:
    the decoder's quant planes are the quantiser's, its coefficients the quantiser's reconstruction, its bytes_read the
    encoder's bytes."""
    T.chain_round_trip(ctx, dtype, round_trip_pictures(), seed=78)
