"""CPU: the walk of tests/noarith_dec_draws.py -- what the draws, their damaged twins and the scale cases must contain to be
worth running on a device, asserted so that no later change can hollow the lists out.  Every figure is the restatement's
(tests/noarith_dec_ref.py)."""
import numpy as np
import pytest

import noarith_dec_cases as DC
import noarith_dec_draws as DD
import noarith_dec_ref as ref
import noarith_enc_ref as enc

COUNTERS = ("truncated", "not_consumed", "overran", "long_codes", "clamped_quant")


def fires(case):
    return case.compat == 0 and case.expected()[2]["compat_quant_offset"] == 1


def test_the_draws_cover_depths_sizes_and_syntax():
    assert len(DD.DRAWS) == DD.NDRAWS >= 48
    assert {(c.depth, c.dtype.itemsize) for c in DD.DRAWS} == {(d, b) for d in range(7) for b in (2, 4)}
    assert all(c.depth == n % 7 for n, c in enumerate(DD.DRAWS))
    assert {c.mode for c in DD.DRAWS} == {0, 1} and {c.compat for c in DD.DRAWS} == {0, 1} and {c.is_intra for c in DD.DRAWS} == {0, 1}
    # both the syntax the encoder writes too (one codeblock in sub-band 0) and the decoder's own
    one = [c for c in DD.DRAWS if c.counts(0) == (1, 1)]
    assert len(DD.DRAWS) // 4 <= len(one) <= 3 * len(DD.DRAWS) // 4
    # sizes that the transform rounds up, and sizes it does not
    assert sum(1 for c in DD.DRAWS if c.depth and int(c.name.split("-")[5].split("x")[0]) % (1 << c.depth)) >= 20
    assert all(c.expected()[2]["error"] == 0 for c in DD.DRAWS)
    # no picture is larger than the named cases' largest
    assert max(len(c.data) for c in DD.DRAWS) < 100000


@pytest.mark.parametrize("depth", [4, 5, 6])
def test_deep_draws_code_every_component(depth):
    """At least one sub-band of every component is coded in at least one draw of the depth (in fact in most), for both
    sample sizes, and the 57 headers of depth 6 are all walked."""
    for b in (2, 4):
        cases = [c for c in DD.DRAWS if c.depth == depth and c.dtype.itemsize == b]
        assert cases
        assert any(all(c.expected()[2]["subband_length"][k].any() for k in range(3)) for c in cases), (depth, b)
    for c in DD.DRAWS:
        if c.depth == depth:
            assert c.nsub == 1 + 3 * depth and c.expected()[2]["bytes_read"] == len(c.data)
            # LL bands of a few samples
            assert enc.subband(c.planes[1], depth, 0).size <= 6 * 4


def test_witnesses_of_the_draws():
    empty = 0
    for c in DD.DRAWS:
        shapes = [enc.get_codeblock(enc.subband(c.planes[k], c.depth, i), x, y, *c.counts(i)).shape
                  for k in range(3) for i in range(c.nsub) for y in range(c.counts(i)[1]) for x in range(c.counts(i)[0])]
        empty += any(h == 0 or w == 0 for h, w in shapes)
    assert empty >= 8, empty
    fired = [c for c in DD.DRAWS if fires(c)]
    assert len(fired) >= 1
    assert sum(1 for c in DD.DRAWS if c.expected()[2]["clamped_quant"]) >= 5
    for c in DD.DRAWS:
        same = all(np.array_equal(a, b) for a, b in zip(c.expected()[1], c.planes))
        if fires(c):
            # the decoder reads the offset as the first value: its planes are not the writer's
            assert c.mode == 1 and c.counts(0) == (1, 1) and not same, c.name
        else:
            assert same, c.name
    # the counters a well-formed stream leaves alone
    for c in DD.DRAWS:
        r = c.expected()[2]
        assert r["truncated"] == 0 and r["long_codes"] == 0 and (fires(c) or r["overran"] == 0), c.name


def test_witnesses_of_the_damage():
    assert set(DD.DAMAGED) == set(DD.KINDS)
    seen = dict.fromkeys(COUNTERS, 0)
    for kind in DD.KINDS:
        cases = DD.DAMAGED[kind]
        assert len(cases) >= 40 and len({c.name for c in cases}) == len(cases)
        errors = sum(c.expected()[2]["error"] for c in cases)
        assert 4 * errors <= len(cases), (kind, errors, len(cases))
        for c in cases:
            for key in COUNTERS:
                seen[key] += int(c.expected()[2][key] > 0)
    assert all(seen.values()), seen
    for c in DD.DAMAGED["flip-payload"] + DD.DAMAGED["pattern"]:
        # headers intact: the lengths and the indices are the draw's
        base = DD.DRAWS[int(c.name[5:7])]
        for key in ("subband_length", "subband_quant_index", "bytes_read"):
            assert np.array_equal(c.expected()[2][key], base.expected()[2][key]), (c.name, key)
    assert all(0 <= c.data_bytes < len(c.data) for c in DD.DAMAGED["cut"])
    assert len({c.name.split("-")[-1] for c in DD.DAMAGED["pattern"]}) == len(DD.PATTERNS)


def test_scale_cases_are_what_their_names_say():
    chunks = {c.name: DD.band_chunks(c) for c in DD.SCALE}
    T = DC.CHAIN_THREADS
    for base, full in (("s16-chain-two-steps", None), ("s32-chain-codeblocks", None)):
        full = DD.band_chunks(DC.BY_NAME[base])[0]
        assert T < full - 1 <= 2 * T                    # two steps
        for tail in ("00", "ff", "aa", "55", "flip-chunk-0", "flip-chunk-1023", "flip-chunk-1024", "flip-last-chunk"):
            assert chunks["%s-%s" % (base, tail)][0] == full, (base, tail)
        for n in (1024, 1025, 1026):
            for form in ("cut", "ends"):
                assert chunks["%s-%s-%d" % (base, form, n)][0] == n, (base, form, n)
            r = DD.BY_NAME["%s-ends-%d" % (base, n)].expected()[2]
            assert r["truncated"] == 1 and r["subband_length"][0, 1] == DC.BY_NAME[base].expected()[2]["subband_length"][0, 1]
            assert DD.BY_NAME["%s-cut-%d" % (base, n)].expected()[2]["subband_length"][0, 1] == n * DD.CHUNK_BYTES
        # the scan sees one chunk less than the band has: 1023, then 1024 (one full step), then 1025 (a second step of one)
        assert 1024 - 1 < T and 1025 - 1 == T and 1026 - 1 == T + 1
        # a flip changes where codes end, in the chunk the name says
        old = DD.band_chunks(DC.BY_NAME[base])[1]
        for what, chunk in (("chunk-0", 0), ("chunk-1023", 1023), ("chunk-1024", 1024), ("last-chunk", full - 1)):
            new = chunks["%s-flip-%s" % (base, what)][1]
            diff = [n for n, (a, b) in enumerate(zip(old, new)) if a != b]
            assert len(new) == len(old) and len(diff) == 1 and diff[0] // DD.CHUNK_BYTES == chunk and bin(old[diff[0]] ^ new[diff[0]]).count("1") == 1
            assert DD.completions(new) != DD.completions(old)
    # the zero twins: the scan must run out, not find -- fewer codes complete than the first codeblock needs
    for name, need in (("s16-chain-two-steps-00", 128 * 64), ("s32-chain-codeblocks-00", 64 * 32), ("s16-chain-three-steps-00", 256 * 64)):
        count, payload = chunks[name]
        assert not any(payload) and DD.completions(payload) == 0 < need
        assert DD.BY_NAME[name].expected()[2]["long_codes"] == 1
    # 64 codes per chunk: the codeblock completes early, the rest is left over
    for base, need in (("s16-chain-two-steps", 128 * 64), ("s32-chain-codeblocks", 128 * 64)):
        count, payload = chunks[base + "-ff"]
        assert DD.completions(payload) == 8 * len(payload) > need + 8 and DD.BY_NAME[base + "-ff"].expected()[2]["not_consumed"] == 1
    # three steps
    assert chunks["s16-chain-three-steps"][0] > 2 * T + 1 and chunks["s16-chain-three-steps-00"][0] == chunks["s16-chain-three-steps"][0]
    three = DD.BY_NAME["s16-chain-three-steps"]
    assert all(np.array_equal(a, b) for a, b in zip(three.expected()[1], three.planes))
    # the cut inside the second codeblock: the first is whole, the second is not, the last two read guard bits only
    cut = DD.BY_NAME["s32-chain-codeblocks-cut-in-codeblock-1"]
    whole = DC.BY_NAME["s32-chain-codeblocks"]
    got, want = (enc.subband(c.expected()[1][0], 1, 1) for c in (cut, whole))
    block = lambda a, x, y: enc.get_codeblock(a, x, y, 2, 2)
    assert np.array_equal(block(got, 0, 0), block(want, 0, 0)) and block(got, 0, 0).any()
    assert not np.array_equal(block(got, 1, 0), block(want, 1, 0)) and block(got, 1, 0).any() and not block(got, 1, 0)[-1].any()
    assert not block(got, 0, 1).any() and not block(got, 1, 1).any()
    assert cut.expected()[2]["overran"] == 1


def test_what_the_batch_and_round_trip_tests_pick_from():
    """tests/test_gpu_noarith_decode_draws.py takes, per sample size, two error streams (one first in a call, one last), two
    intact draws each of depths 0, 3 and 6 and a `00` scale stream; and per depth 4 .. 6 a draw with one codeblock in sub-band
    0, where the encoder's and the decoder's rules agree."""
    for b in (2, 4):
        mine = lambda cases: [c for c in cases if c.dtype.itemsize == b]
        assert sum(c.expected()[2]["error"] for c in mine(DD.DAMAGED["flip-anywhere"])) >= 2
        for depth in (0, 3, 6):
            assert sum(1 for c in mine(DD.DRAWS) if c.depth == depth) >= 2
        assert any(c.name.endswith("-00") for c in mine(DD.SCALE))
        # a draw of middling size with a payload of at least 128 bytes: a length word can end inside its header
        assert sorted(len(c.data) for c in mine(DD.DRAWS))[len(mine(DD.DRAWS)) // 2] > 1000
    for depth in (4, 5, 6):
        assert any(c.depth == depth and c.counts(0) == (1, 1) for c in DD.DRAWS)


def test_names_are_unique_and_sizes_small():
    assert len(DD.BY_NAME) == len(DD.ALL)
    assert len(DD.SCALE) == 2 * (4 + 4 + 6) + 1 + 2
    assert max(len(c.data) for c in DD.SCALE) < 20000
