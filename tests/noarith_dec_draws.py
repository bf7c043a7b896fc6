"""Seeded random geometries, their damaged twins and the scan's scale cases of the noarith (VLC) transform-data decoder,
shared by the CPU walk (tests/test_noarith_dec_draws.py), the GPU test (tests/test_gpu_noarith_decode_draws.py) and the
sanitizer walk.  The named cases and the limits they sit on are tests/noarith_dec_cases.py's; this module adds what no
hand-picked case has: transform depths 4 .. 6 (57 sub-bands, LL bands of one or two samples, more codeblocks than samples at
several levels at once), sizes that round up to the transform's, codeblock counts drawn per level, and damage to streams
long enough for the chain workgroup's scan (CHAIN_THREADS chunks per step) to go on for more than one step.

  DRAWS    NDRAWS pictures through the writer of tests/noarith_dec_ref.py.  Draw n has depth n % 7; the sample size
           alternates in blocks of 7, so every depth meets both.
  DAMAGED  every draw with a payload, once per kind of KINDS, from a second generator.
  SCALE    named, deterministic streams around the scan step, from `s16-chain-two-steps`, `s32-chain-codeblocks` and one
           picture whose sub-band (0, 1) takes three steps.

What the decoder must make of each comes from the restatement, once per case (Case.expected).  The witnesses -- what the
lists must contain to be worth running -- are asserted by the CPU walk, not here, so that importing stays cheap."""
import numpy as np

import noarith_dec_cases as DC
import noarith_dec_ref as ref
import noarith_enc_ref as enc

SEED = 20261021
DAMAGE_SEED = 20261022
NDRAWS = 48
FORMATS = (420, 422, 444)
DENSITIES = (0.05, 0.3, 0.7, 1.0)
KINDS = ("flip-payload", "flip-anywhere", "cut", "pattern")
PATTERNS = (b"\x00", b"\xff", b"\xaa", b"\x55", b"\x2a\xaa")
CHUNK_BYTES = DC.CHUNK_BITS // 8


def offsets_drawn(k, i, x, y):
    """-4 .. 4"""
    return (3 * k + 5 * i + x + 2 * y) % 9 - 4


def _fill(case, rng):
    density = float(rng.choice(DENSITIES))
    top = 32767 if case.dtype == np.int16 else (1 << 31) - 1
    lim = int(rng.choice([1, 6, 300, top]))
    for p in case.planes:
        v = rng.integers(-lim, lim + 1, p.shape)
        p[...] = np.where(rng.random(p.shape) < density, v, 0)
    for k in range(3):
        for i in range(case.nsub):
            if rng.random() < 0.15:
                case.band(k, i)[...] = 0


def _draws():
    rng = np.random.default_rng(SEED)
    out = []
    for n in range(NDRAWS):
        depth = n % 7
        dtype = np.int16 if (n // 7) % 2 == 0 else np.int32
        fmt = int(rng.choice(FORMATS))
        lw, lh = int(rng.integers(1, 97)), int(rng.integers(1, 65))
        counts = [(int(rng.integers(1, 6)), int(rng.integers(1, 5))) for _ in range(depth + 1)]
        if rng.random() < 0.5:
            counts[0] = (1, 1)
        mode, compat, intra = (int(rng.integers(0, 2)) for _ in range(3))
        name = "draw-%02d-%s-d%d-%d-%dx%d-m%d-c%d" % (n, "s16" if dtype == np.int16 else "s32", depth, fmt, lw, lh, mode, compat)
        out.append(DC.written(name, dtype, lw, lh, fmt, depth, counts, mode, compat, _fill, seed=int(rng.integers(1 << 30)), is_intra=intra,
                              offsets=offsets_drawn, qbase=int(rng.integers(0, 61))))
    return out


# ---- damage -----------------------------------------------------------------------------------------------------------------

def flipped(data, bits):
    data = bytearray(data)
    for b in bits:
        data[int(b) >> 3] ^= 0x80 >> (int(b) & 7)
    return bytes(data)


def structural_bit(payload, chunk):
    """The first bit of the chunk (not its first: a head may sit there) whose flip changes how many codes complete in the
    payload: the codes behind it start elsewhere, and a codeblock ends in another chunk."""
    was = completions(payload)
    for bit in range(1, DC.CHUNK_BITS):
        if DC.CHUNK_BITS * chunk + bit < 8 * len(payload) and completions(flipped(payload, [DC.CHUNK_BITS * chunk + bit])) != was:
            return bit
    raise AssertionError("chunk %d has no such bit" % chunk)


def _like(case, name, data, data_bytes=None):
    return DC.Case(name, case.dtype, case.sizes, case.depth, case.hc, case.vc, case.mode, case.compat, case.is_intra, data, data_bytes)


def _damaged():
    rng = np.random.default_rng(DAMAGE_SEED)
    out = {kind: [] for kind in KINDS}
    for case in DRAWS:
        bands = DC.split(case.data, 3 * case.nsub)
        assert DC.join(bands) == case.data
        if not any(length for length, _, _ in bands):
            continue                    # nothing but headers
        tag = case.name[:7]             # draw-NN
        # one bit per 64 payload bytes, at least one, in every coded sub-band; the headers stay what they are
        b = [(length, qi, flipped(payload, rng.integers(0, 8 * length, max(1, length // 64))) if length else payload)
             for length, qi, payload in bands]
        out["flip-payload"].append(_like(case, tag + "-flip-payload", DC.join(b)))
        n = len(case.data)
        out["flip-anywhere"].append(_like(case, tag + "-flip-anywhere", flipped(case.data, rng.integers(0, 8 * n, max(1, n // 256)))))
        out["cut"].append(_like(case, tag + "-cut", case.data, int(rng.integers(0, n))))
        big = max(range(len(bands)), key=lambda j: bands[j][0])
        pattern = PATTERNS[int(rng.integers(0, len(PATTERNS)))]
        length, qi, _ = bands[big]
        b = list(bands)
        b[big] = (length, qi, (pattern * length)[:length])
        out["pattern"].append(_like(case, "%s-pattern-%s" % (tag, pattern.hex()), DC.join(b)))
    return out


# ---- the scan's scale -------------------------------------------------------------------------------------------------------
# Sub-band (0, 1) -- the second header of the stream -- is the one that matters: the others of these pictures are zero.

BAND = 1


def _three_steps():
    # 256 x 64 values of 8 bits are 2048 chunks; 200 ten-bit codes make it 2055: thread 0 takes the first, the scan 1024, 1024 and 6
    return DC.written("s16-chain-three-steps", np.int16, 512, 128, 444, 1, DC.COUNTS["one"], 0, 0, lambda c, r: DC.fill_eight_bit(c, r, 200), 37)


def _scale():
    out = []
    three = _three_steps()
    for base in (DC.BY_NAME["s16-chain-two-steps"], DC.BY_NAME["s32-chain-codeblocks"], three):
        bands = DC.split(base.data, 3 * base.nsub)
        length, qi, payload = bands[BAND]
        assert all(l == 0 for j, (l, _, _) in enumerate(bands) if j != BAND)
        first = len(DC.join(bands[:BAND] + [(length, qi, b"")]))       # the payload's first byte in the stream

        def with_payload(name, new, new_length=None, data_bytes=None):
            b = list(bands)
            b[BAND] = (length if new_length is None else new_length, qi, new)
            return _like(base, "%s-%s" % (base.name, name), DC.join(b), data_bytes)

        if base is three:
            out.append(base)
            # one code that never ends, through all three steps
            out.append(with_payload("00", b"\x00" * length))
            continue
        for pattern in (b"\x00", b"\xff", b"\xaa", b"\x55"):
            out.append(with_payload(pattern.hex(), pattern * length))
        last = (length - 1) // CHUNK_BYTES
        for what, chunk in (("chunk-0", 0), ("chunk-1023", 1023), ("chunk-1024", 1024), ("last-chunk", last)):
            assert chunk <= last
            out.append(with_payload("flip-" + what, flipped(payload, [DC.CHUNK_BITS * chunk + structural_bit(payload, chunk)])))
        for chunks in (1024, 1025, 1026):
            keep = CHUNK_BYTES * chunks
            assert keep < length
            # the sub-band shorter, the rest of the stream behind it ...
            out.append(with_payload("cut-%d" % chunks, payload[:keep], new_length=keep))
            # ... and the stated length kept, the input ending inside the payload
            out.append(_like(base, "%s-ends-%d" % (base.name, chunks), base.data, first + keep))
        if base.counts(BAND) == (2, 2):
            # the payload ends inside the second of the four codeblocks: the heads behind it read guard bits
            cb = enc.get_codeblock(enc.subband(base.planes[0], base.depth, BAND), 0, 0, 2, 2)
            one = sum(DC.code_bits(v) for v in cb.reshape(-1).tolist()) // 8
            keep = one + one // 2
            out.append(with_payload("cut-in-codeblock-1", payload[:keep], new_length=keep))
    return out


def band_chunks(case):
    """The chunks the decoder hands sub-band (0, 1) of a SCALE case: 64 bits each of the payload as far as the input goes."""
    bands = ref.parse_transform_data(case.data[:case.data_bytes], case.depth, ref.empty_result(0))
    (payload,) = [p for k, i, qi, length, p in bands if (k, i) == (0, BAND)]
    return -(-len(payload) // CHUNK_BYTES), payload


def completions(payload):
    """The codes that complete inside the payload from a code's start at bit 0."""
    state, n = ref.A, 0
    for byte in payload:
        for bit in range(7, -1, -1):
            state, done = ref.step(state, (byte >> bit) & 1)
            n += done
    return n


DRAWS = _draws()
DAMAGED = _damaged()
SCALE = _scale()
ALL = DRAWS + [c for kind in KINDS for c in DAMAGED[kind]] + SCALE
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL) and not set(BY_NAME) & (set(DC.BY_NAME) - {c.name for c in SCALE})
