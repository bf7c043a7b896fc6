"""The streams the arithmetic motion-data decoder is tested on (tests/test_motion_arith_dec_ref.py on the CPU,
tests/test_gpu_motion_arith_decode.py on the device).

A case is (name, data, x_num_blocks, y_num_blocks, num_refs, have_global_motion, form): form says which restatement gives
the expectation -- "serial" (motion_arith_dec_ref.decode) or, for the two large limits, "phased" (decode_phased, held equal
to the serial one on everything small).

INTACT   the field of every case of motion_dec_cases.intact () -- every encoder case, both reference counts, global motion
         -- written with the arithmetic writer.
LIMITS   72 x 68 and 260 x 260 blocks of random payload bytes: a diagonal longer than a wave and longer than the walks'
         workgroups, and chains that run off their payloads; splits written with 32 and 31 data bins (long_codes; the first
         is 2^32, which the decoder keeps mod 2^32: the split is (pred + 0) % 3, not (pred + 2^32) % 3); a DC residual of
         exactly 30 data bins (the loop stops there: the next bin is the sign, and the residual behind it decodes); a
         section whose payload ends in the middle of a code; a section of length 0 among non-empty ones.
HOSTILE  each intact stream of at most 600 blocks, damaged four ways (see hostile ()).
"""
import numpy as np

import motion_arith_dec_ref as A
import motion_dec_cases as DC
from motion_enc_ref import SECTIONS

SMALL = DC.SMALL                # blocks: the serial restatement is quick below
FILL_MAX = 256                  # bytes of a filled payload: a 00 byte costs about 1277 bins

_EXPECTED = {}


def expected(case):
    """(field, result) of a case, computed once."""
    if case[0] not in _EXPECTED:
        f = A.decode if case[6] == "serial" else A.decode_phased
        _EXPECTED[case[0]] = f(*case[1:6])
    return _EXPECTED[case[0]]


_INTACT = []


def intact():
    if not _INTACT:
        for c in DC.intact():
            field = DC.expected(c)[0]
            _INTACT.append((c[0], A.write_field(field, *c[2:6]), c[2], c[3], c[4], c[5], "serial" if c[2] * c[3] <= 5000 else "phased"))
    return _INTACT


def field_of(case):
    """The field an intact case was written from."""
    return DC.expected(next(c for c in DC.intact() if c[0] == case[0]))[0]


def limits():
    out = []
    rng = np.random.default_rng(401)
    for nbx, nby, num_refs in ((72, 68, 2), (260, 260, 2)):
        blocks = nbx * nby
        sizes = [blocks // 16 // 4, blocks // 4] + [blocks // 8] * 7
        data = A.frame([rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes], num_refs)
        out.append(("%dx%d random bytes" % (nbx, nby), data, nbx, nby, num_refs, 0, "phased"))
    # 8 x 8: four superblocks; the other sections are empty and read 0xff: every value 0
    splits = A.write_section(0, [1 << 32, (1 << 31) + 1, 1, 0])
    out.append(("splits of 32 and 31 data bins", A.frame([splits] + [b""] * 8, 2), 8, 8, 2, 0, "serial"))
    # every block a DC: the first Y residual is -(2^30 + 5) -- 30 data bins, then the sign -- and the second one 3
    base = intact_by_name("all DC")
    p = A.payloads_of(base[1], 2)
    units = expected(base)[1]["section_units"][6]
    p[6] = A.write_section(6, [-(1 << 30) - 5, 3] + [0] * (units - 2))
    out.append(("a DC residual of 30 data bins", A.frame(p, 2), base[2], base[3], 2, 0, "serial"))
    # the longest payload of a stream without its last third
    base = intact_by_name("12x12 mixed refs 2")
    p = A.payloads_of(base[1], 2)
    s = max(range(SECTIONS), key=lambda k: len(p[k]))
    p[s] = p[s][:2 * len(p[s]) // 3]
    out.append(("a payload that ends inside a code", A.frame(p, 2), 12, 12, 2, 0, "serial"))
    p = A.payloads_of(base[1], 2)
    p[2] = b""
    out.append(("a section of length 0 among others", A.frame(p, 2), 12, 12, 2, 0, "serial"))
    return out


def intact_by_name(name):
    return next(c for c in intact() if c[0] == name)


def hostile():
    """Per intact stream of at most SMALL blocks: a flipped bit per 32 bytes inside payloads (headers intact), the input cut
    to 0 .. len - 1 bytes, the last section's stated length reaching past the input, the longest section (FILL_MAX bytes of
    it at most) replaced by 00, ff, aa or 55."""
    out, kinds = [], {}
    for n, c in enumerate(x for x in intact() if x[2] * x[3] <= SMALL):
        name, data, nbx, nby, num_refs, hg, _ = c
        rng = np.random.default_rng(6000 + n)
        sections = A.parse(data, num_refs)[0]
        inside = np.concatenate([np.arange(sec[0], sec[0] + sec[1]) for sec in sections if sec is not None and sec[1]])
        picks = [int(rng.choice(inside[(inside >= lo) & (inside < lo + 32)])) * 8 + int(rng.integers(0, 8))
                 for lo in range(0, len(data), 32) if ((inside >= lo) & (inside < lo + 32)).any()]

        def add(kind, d):
            out.append(("%s, %s" % (name, kind), d, nbx, nby, num_refs, hg, "serial"))
            kinds.setdefault(kind.split(":")[0], []).append(out[-1])
        add("payload bits", DC.flip(data, picks))
        cut = 0 if n == 0 else len(data) - 1 if n == 1 else int(rng.integers(0, len(data)))
        add("cut: %d of %d bytes" % (cut, len(data)), data[:cut])
        p = A.payloads_of(data, num_refs)
        lengths = [len(x) for x in p]
        lengths[8] += 1 + n
        add("length past the input: %d for %d bytes" % (lengths[8], len(p[8])), A.frame(p, num_refs, lengths))
        longest = max((s for s in range(SECTIONS) if sections[s] is not None), key=lambda s: sections[s][1])
        byte = (0x00, 0xff, 0xaa, 0x55)[n % 4]
        p[longest] = bytes([byte]) * min(len(p[longest]), FILL_MAX)
        add("filled: section %d with %02x" % (longest, byte), A.frame(p, num_refs))
    # the witnesses, from the restatement
    results = [expected(c)[1] for c in out + limits()]
    witness = {k: sum(bool(r[k]) for r in results) for k in ("truncated", "overran", "not_consumed", "long_codes", "unverified")}
    assert all(witness.values()), witness
    by_name = {c[0]: c for c in intact()}
    seen = sum(expected(c)[0].tobytes() != expected(by_name[c[0].rsplit(", ", 1)[0]])[0].tobytes() for c in kinds["payload bits"])
    assert seen, (seen, len(kinds["payload bits"]))
    witness.update(streams=len(out), payload_damage_seen=seen, payload_damaged=len(kinds["payload bits"]))
    return out, witness


_ALL = None


def all_cases():
    """(intact, limits, hostile, witness counts), made once and shared."""
    global _ALL
    if _ALL is None:
        h, w = hostile()
        _ALL = (intact(), limits_once(), h, w)
        names = [c[0] for part in _ALL[:3] for c in part]
        assert len(set(names)) == len(names)
    return _ALL


_LIMITS = []


def limits_once():
    if not _LIMITS:
        _LIMITS.extend(limits())
    return _LIMITS


def describe():
    """The witness counts, as DESIGN 4.25 quotes them."""
    w = all_cases()[3]
    return ("%(streams)d hostile streams: truncated %(truncated)d, overran %(overran)d, not_consumed %(not_consumed)d, long_codes "
            "%(long_codes)d, unverified %(unverified)d (limits included); %(payload_damage_seen)d of %(payload_damaged)d "
            "payload-damaged streams decode to another field" % w)


# ---- the refusals: motion_dec_cases' descriptions (the same words), with this call's result size -----------------------------

RESULT_BYTES = 172
describe_picture = DC.describe
REFUSALS = [r for r in DC.REFUSALS if r[0] != "the result over the length word"] + [
    ("the result over the length word", DC._set(word=DC.RESULT + RESULT_BYTES - 4), "picture 0: bytes_on_device overlaps the result of picture 0"),
]
ACCEPTED = [a for a in DC.ACCEPTED if a[0] != "the length word behind the result"] + [
    ("the length word behind the result", DC._set(word=DC.RESULT + RESULT_BYTES)),
]


def scratch_words(pictures):
    """schro_hip_motion_arith_decode_scratch_words by hand: per picture 9 sections of 4 words; a split residual, a split
    and a first unit per superblock, padded to an even count; per block a word of mode bins, seven residuals, the flags and
    two code indices."""
    total = 0
    for p in pictures:
        blocks = p["nbx"] * p["nby"]
        total += 9 * 4 + (3 * (blocks // 16) + 1) // 2 * 2 + 11 * blocks
    return total
