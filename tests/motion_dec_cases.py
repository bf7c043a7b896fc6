"""The streams the motion-data decoder is tested on (tests/test_motion_dec_ref.py on the CPU, tests/test_gpu_motion_decode.py
and the sanitized walk over the same geometries).

A case is (name, data, x_num_blocks, y_num_blocks, num_refs, have_global_motion, form): form says which restatement gives
the expectation -- "serial" (motion_dec_ref.decode) or, where that would take more than a few seconds, "wavefront"
(decode_wavefront, held equal to the serial one on everything small).

INTACT   every case of motion_enc_cases.all_cases () through its encoded bytes.
LIMITS   a picture on either side of each limit motion_dec.hip introduces (its constants are restated below):
  - 4 x 4, 8 x 4, 4 x 8: one superblock, two side by side, two on top of each other -- they are intact cases;
  - a code that ends one bit before, on and up to three bits behind a chunk's end (the next chunk is entered in state A,
    A, D, F, S), in a section of 12 x 12 DC blocks: the smallest drawn field with more than 64 codes in a section;
  - 64 codes in a chunk: that section all ff;
  - the scan composes SCAN_THREADS = 256 runs of chunks: a section of 255, 256 and 257 chunks (the run goes from one
    chunk to two), of 66-bit codes so that the 256 codes of a 16 x 16 picture reach over all of them, and the same
    lengths of random bytes in the unsigned section 0;
  - the walks stride over a diagonal: 72 x 68 random bytes have diagonals of 68 blocks, longer than a wave and shorter than
    the walks' workgroup of 256; 260 x 260 is the smallest square with a diagonal of more than 256 blocks, and its 65
    superblocks per diagonal are more than the split walk's workgroup of 64, which is one wave.
DAMAGED  each intact stream of at most 600 blocks, damaged four ways (see damaged ()).
"""
import numpy as np

import motion_dec_ref as D
import motion_enc_cases as MC
import motion_enc_ref as R

CHUNK_BYTES = 8
SCAN_THREADS = 256              # kMdScanThreads
WALK_THREADS = 256              # kMdWalkThreads
SPLIT_THREADS = 64              # kMdSplitThreads
SMALL = 600                     # blocks: the serial restatement is quick below

_EXPECTED = {}


def expected(case):
    """(field, result) of a case, computed once."""
    if case[0] not in _EXPECTED:
        f = D.decode if case[6] == "serial" else D.decode_wavefront
        _EXPECTED[case[0]] = f(*case[1:6])
    return _EXPECTED[case[0]]


def uint_code(value):
    """The bits of schro_pack_encode_uint."""
    v = value + 1
    n = v.bit_length() - 1
    return "".join("0" + str((v >> i) & 1) for i in range(n - 1, -1, -1)) + "1"


def to_bytes(bits, fill="1"):
    bits += fill * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def assemble(payloads, num_refs):
    """A stream of the given payloads: per section the length code on a byte of its own, then the payload."""
    out = b""
    for s in range(R.SECTIONS):
        if not D.absent(num_refs, s):
            out += to_bytes(uint_code(len(payloads[s])), "0") + bytes(payloads[s])
    return out


def payloads_of(data, num_refs):
    sections = D.parse(data, num_refs)[0]
    return [b"" if sec is None else bytes(data[sec[0]:sec[0] + sec[1]]) for sec in sections]


def replace(data, num_refs, s, payload):
    p = payloads_of(data, num_refs)
    p[s] = payload
    return assemble(p, num_refs)


_INTACT = []


def intact():
    if not _INTACT:
        _INTACT.extend((c[0], R.encode(*c[1:6])[0], c[2], c[3], c[4], c[5], "serial" if c[2] * c[3] <= 5000 else "wavefront")
                       for c in MC.all_cases())
    return _INTACT


def limits():
    out = []
    geometries = {c[2:4] for c in MC.all_cases()}
    assert {(4, 4), (8, 4), (4, 8)} <= geometries
    dc = R.encode(MC.draw(300, 12, 12, 2, 0, splits=(2,), modes=(0,)), 12, 12, 2, 0)[0]
    for pad in (59, 60, 61, 62, 63):
        # `pad` codes of one bit, then 0 0 1 s: the sign is bit pad + 3 of the payload
        bits = "1" * pad + "0011" + "1" * (140 - pad) + "0010" * 3
        out.append(("a four-bit code behind %d bits" % pad, replace(dc, 2, 6, to_bytes(bits)), 12, 12, 2, 0, "serial"))
    out.append(("64 codes in a chunk", replace(dc, 2, 6, b"\xff" * 24), 12, 12, 2, 0, "serial"))
    rng = np.random.default_rng(301)
    base = R.encode(MC.draw(302, 16, 16, 2, 0, splits=(2,), modes=(0,)), 16, 16, 2, 0)[0]
    long_bits = "".join("".join("0" + str(b) for b in rng.integers(0, 2, 32)) + "1" + str(int(rng.integers(0, 2))) for _ in range(256))
    assert len(long_bits) >= 8 * CHUNK_BYTES * (SCAN_THREADS + 1)
    for nchunks in (SCAN_THREADS - 1, SCAN_THREADS, SCAN_THREADS + 1):
        n = CHUNK_BYTES * nchunks
        out.append(("%d chunks of 66-bit codes" % nchunks, replace(base, 2, 7, to_bytes(long_bits)[:n]), 16, 16, 2, 0, "serial"))
        out.append(("%d chunks of random splits" % nchunks, replace(base, 2, 0, rng.integers(0, 256, n, dtype=np.uint8).tobytes()),
                    16, 16, 2, 0, "serial"))
    for nbx, nby, num_refs in ((72, 68, 2), (260, 260, 2)):
        assert min(nbx, nby) > 64 and (min(nbx, nby) > WALK_THREADS) == (nbx == 260)
        blocks = nbx * nby
        sizes = [blocks // 16 // 2, blocks // 2] + [blocks // 4] * 7
        data = assemble([rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes], num_refs)
        out.append(("%dx%d random bytes" % (nbx, nby), data, nbx, nby, num_refs, 0, "wavefront"))
    assert 260 // 4 > SPLIT_THREADS and 256 // 4 <= SPLIT_THREADS
    return out


def flip(data, positions):
    b = bytearray(data)
    for p in positions:
        b[p >> 3] ^= 0x80 >> (p & 7)
    return bytes(b)


def damaged():
    """Per intact stream of at most SMALL blocks: a flipped bit per 32 bytes inside payloads (headers intact), a flipped
    bit per 64 bytes anywhere, the input cut to 0 .. len - 1 bytes, the longest section replaced by 00, ff, aa or 55."""
    out, kinds = [], {}
    for n, c in enumerate(x for x in intact() if x[2] * x[3] <= SMALL):
        name, data, nbx, nby, num_refs, hg, _ = c
        rng = np.random.default_rng(5000 + n)
        sections = D.parse(data, num_refs)[0]
        inside = np.concatenate([np.arange(sec[0], sec[0] + sec[1]) for sec in sections if sec is not None and sec[1]])
        picks = [int(rng.choice(inside[(inside >= lo) & (inside < lo + 32)])) * 8 + int(rng.integers(0, 8))
                 for lo in range(0, len(data), 32) if ((inside >= lo) & (inside < lo + 32)).any()]
        add = lambda kind, d: (out.append(("%s, %s" % (name, kind), d, nbx, nby, num_refs, hg, "serial")), kinds.setdefault(kind.split(":")[0], []).append(out[-1]))
        add("payload bits", flip(data, picks))
        add("any bits", flip(data, [int(rng.integers(8 * lo, 8 * min(lo + 64, len(data)))) for lo in range(0, len(data), 64)]))
        cut = 0 if n == 0 else len(data) - 1 if n == 1 else int(rng.integers(0, len(data)))
        add("cut: %d of %d bytes" % (cut, len(data)), data[:cut])
        longest = max((s for s in range(R.SECTIONS) if sections[s] is not None), key=lambda s: sections[s][1])
        byte = (0x00, 0xff, 0xaa, 0x55)[n % 4]
        add("filled: section %d with %02x" % (longest, byte), replace(data, num_refs, longest, bytes([byte]) * sections[longest][1]))
    # the witnesses, from the restatement
    results = [expected(c)[1] for c in out]
    witness = {k: sum(bool(r[k]) for r in results) for k in ("truncated", "overran", "not_consumed", "long_codes", "unverified")}
    assert all(witness[k] for k in ("truncated", "overran", "not_consumed", "long_codes")), witness
    # a 00 section is one code that never ends: it is long and reads to the payload's end and past it
    never = [c for c in kinds["filled"] if " with 00" in c[0] and expected(c)[1]["long_codes"] and expected(c)[1]["overran"]]
    assert never
    by_name = {c[0]: c for c in intact()}
    seen = sum(expected(c)[0].tobytes() != expected(by_name[c[0].rsplit(", ", 1)[0]])[0].tobytes() for c in kinds["payload bits"])
    assert 2 * seen >= len(kinds["payload bits"]), (seen, len(kinds["payload bits"]))
    witness.update(streams=len(out), never_ending=len(never), payload_damage_seen=seen, payload_damaged=len(kinds["payload bits"]))
    return out, witness


_ALL = None


def all_cases():
    """(intact, limits, damaged, witness counts), made once and shared."""
    global _ALL
    if _ALL is None:
        d, w = damaged()
        _ALL = (intact(), limits(), d, w)
        names = [c[0] for part in _ALL[:3] for c in part]
        assert len(set(names)) == len(names)
    return _ALL


def every():
    a = all_cases()
    return a[0] + a[1] + a[2]


# ---- the refusals of schro_hip_motion_decode_check: descriptions with addresses only (nothing is dereferenced) ---------

MAX_BLOCKS = 1 << 14
MAX_BYTES = 1 << 29
DATA, WORD, FIELD, RESULT = 0x1000000, 0x1800000, 0x2000000, 0x3000000
FIELD_BYTES = 8 * 8 * 20
RESULT_BYTES = 136


def describe():
    """One 8 x 8 picture with two references: the data, the length word, the field and the result far apart."""
    return [dict(data=DATA, data_bytes=100, word=None, nbx=8, nby=8, num_refs=2, hg=0, motion=FIELD, result=RESULT)]


def _set(**kw):
    def change(d):
        d[0].update(kw)
    return change


def _second(**kw):
    """A second picture, far from the first, with `kw` relative to the first one's addresses."""
    def change(d):
        p = dict(d[0], data=0x100 * DATA, motion=0x100 * FIELD, result=0x100 * RESULT)
        p.update({k: (v(d[0]) if callable(v) else v) for k, v in kw.items()})
        d.append(p)
    return change


REFUSALS = [
    ("no columns", _set(nbx=0), "picture 0: 0 x 8 blocks must be positive multiples of 4"),
    ("negative rows", _set(nby=-4), "picture 0: 8 x -4 blocks must be positive multiples of 4"),
    ("columns no multiple of 4", _set(nbx=6), "picture 0: 6 x 8 blocks must be positive multiples of 4"),
    ("rows no multiple of 4", _set(nby=10), "picture 0: 8 x 10 blocks must be positive multiples of 4"),
    ("too many columns", _set(nbx=MAX_BLOCKS + 4, nby=4), "picture 0: 16388 x 4 blocks"),
    ("too many rows", _set(nbx=4, nby=MAX_BLOCKS + 4), "picture 0: 4 x 16388 blocks"),
    ("no reference", _set(num_refs=0), "picture 0: num_refs 0 (1 or 2)"),
    ("three references", _set(num_refs=3), "picture 0: num_refs 3 (1 or 2)"),
    ("no data", _set(data=0), "picture 0: data is NULL"),
    ("no field", _set(motion=0), "picture 0: motion is NULL or not 4-byte aligned"),
    ("a misaligned field", _set(motion=FIELD + 2), "picture 0: motion is NULL or not 4-byte aligned"),
    ("no result", _set(result=0), "picture 0: result is NULL or not 4-byte aligned"),
    ("a misaligned result", _set(result=RESULT + 1), "picture 0: result is NULL or not 4-byte aligned"),
    ("a misaligned length word", _set(word=WORD + 2), "picture 0: bytes_on_device is not 4-byte aligned"),
    ("2^29 bytes", _set(data_bytes=MAX_BYTES), "picture 0: data_bytes %d" % MAX_BYTES),
    ("the field over the data", _set(motion=DATA + 96), "picture 0: the field overlaps data of picture 0"),
    ("the data ends inside the field", _set(data=FIELD + FIELD_BYTES - 4), "picture 0: data overlaps the field of picture 0"),
    ("the result over the data", _set(result=DATA + 4), "picture 0: the result overlaps data of picture 0"),
    ("the result inside the field", _set(result=FIELD + FIELD_BYTES - 4), "picture 0: the result overlaps the field of picture 0"),
    ("the field over the length word", _set(word=FIELD + 40), "picture 0: bytes_on_device overlaps the field of picture 0"),
    ("the result over the length word", _set(word=RESULT + RESULT_BYTES - 4), "picture 0: bytes_on_device overlaps the result of picture 0"),
    ("a second picture's field over the first one's data", _second(motion=lambda p: p["data"] - FIELD_BYTES + 4),
     "picture 0: data overlaps the field of picture 1"),
    ("a second picture's result over the first one's field", _second(result=lambda p: p["motion"] + 40),
     "picture 1: the result overlaps the field of picture 0"),
    ("two pictures into one field", _second(motion=lambda p: p["motion"]), "overlaps the field of picture"),
    ("a second picture's length word in the first one's result", _second(word=lambda p: p["result"]),
     "overlaps the result of picture"),
    ("the second picture's geometry", _second(nby=2), "picture 1: 8 x 2 blocks must be positive multiples of 4"),
]

ACCEPTED = [
    ("one superblock", _set(nbx=4, nby=4)),
    ("as many columns as there can be", _set(nbx=MAX_BLOCKS, nby=4)),
    ("as many rows as there can be", _set(nbx=4, nby=MAX_BLOCKS)),
    ("one reference", _set(num_refs=1)),
    ("global motion", _set(hg=1)),
    ("no bytes", _set(data_bytes=0)),
    ("no bytes at the field's address", _set(data=FIELD, data_bytes=0)),
    ("the last size below 2^29", _set(data=0x100 * DATA, data_bytes=MAX_BYTES - 1)),
    ("data at an odd address", _set(data=DATA + 3)),
    ("a length word", _set(word=WORD)),
    ("a field aligned to 4 bytes only", _set(motion=FIELD + 4)),
    ("the data up to the field's first byte", _set(data=FIELD - 100)),
    ("the data behind the field's last byte", _set(data=FIELD + FIELD_BYTES)),
    ("the result behind the field", _set(result=FIELD + FIELD_BYTES)),
    ("the length word behind the result", _set(word=RESULT + RESULT_BYTES)),
    ("two pictures of one stream and one length word", _second(data=lambda p: p["data"], word=WORD)),
]


def scratch_words(pictures):
    """schro_hip_motion_decode_scratch_words by hand: per picture 9 sections of 8 words; a summary and an entry of two
    words each per chunk slot, of which (data_bytes + 7) / 8 + 8 suffice (a section of n bytes has at most n / 8 + 1 chunks
    and eight sections have chunks); a split residual, a split and a first unit per superblock, padded to an even count;
    seven residuals, the flags and two code indices per block."""
    total = 0
    for p in pictures:
        blocks = p["nbx"] * p["nby"]
        total += 9 * 8 + 4 * ((p["data_bytes"] + 7) // 8 + 8) + (3 * (blocks // 16) + 1) // 2 * 2 + 10 * blocks
    return total
