"""Pictures, limits, hostile streams and refusals of the noarith (VLC) transform-data decoder, shared by its GPU tests, the
CPU walk of schro_hip_noarith_decode_check and the sanitizer walk (tests/c/noarith_dec_walk.cpp reads the table
tests/test_noarith_dec_host_sanitized.py writes from this module).

A case is a byte string and what the decoder is told about the picture; what the decoder must make of it comes from
tests/noarith_dec_ref.py, once per case.  The streams come from the writer of that file, which follows the DECODER's
rules (zero flags on sub-band 0, quant offsets on 1 x 1 sub-bands when not in compat mode, non-zero offsets), or are
such streams damaged on purpose.  Each case is named for what it catches; where a case exists to sit on one side of a limit
of the kernels (schroedinger_amd/csrc/noarith_dec.hip, schro_hip_internal.h), the property is asserted below:
  CHUNK_BITS     a lane's share of a payload is 64 bits: codes that end on, before and behind a chunk's end; 64 codes in a
                 chunk; a code per chunk and longer; many codeblock heads in one chunk (codeblocks of no width);
  CHAIN_THREADS  the chain workgroup composes 1024 chunk summaries per step: a codeblock that takes one step and one that
                 takes two;
  FILL_GRID_X    a sub-band's row pieces are walked in strides by at most 1024 workgroups.
The chunk-per-lane launches do not stride: their grid covers every chunk slot.
"""
import functools

import numpy as np

import noarith_dec_ref as ref
import noarith_enc_cases as NC
import noarith_enc_ref as enc

CHUNK_BITS = 64
CHAIN_THREADS = 1024
FILL_GRID_X = 1024


class Case:
    def __init__(self, name, dtype, sizes, depth, hc, vc, mode, compat, is_intra, data, data_bytes=None, planes=None):
        self.name, self.dtype, self.sizes, self.depth = name, np.dtype(dtype), list(sizes), depth
        self.hc, self.vc, self.mode, self.compat, self.is_intra = list(hc), list(vc), mode, int(compat), int(is_intra)
        self.data = bytes(data)
        self.data_bytes = len(self.data) if data_bytes is None else data_bytes
        self.nsub = 1 + 3 * depth
        self.planes = planes            # the quant planes the stream was written from (None: a damaged stream)

    def counts(self, i):
        return enc.codeblock_counts(i, self.hc, self.vc)

    @functools.lru_cache(maxsize=None)
    def expected(self):
        """(coeffs, quant, result) of the restatement over planes that held zeros: computed once, shared, never changed.
        A picture with the error leaves its planes as they were: coeffs and quant are None."""
        coeffs = [np.zeros((h, w), self.dtype) for w, h in self.sizes]
        quant = [np.zeros((h, w), self.dtype) for w, h in self.sizes]
        result = ref.decode_transform_data(self.data[:self.data_bytes], coeffs, quant, self.depth, self.hc, self.vc, self.mode,
                                           self.is_intra, self.compat)
        if result["error"]:
            return None, None, result
        return coeffs, quant, result


def offsets_small(k, i, x, y):
    return (x + 2 * y + i + k) % 7 - 3


def written(name, dtype, lw, lh, fmt, depth, counts, mode, compat, fill, seed=1, is_intra=0, offsets=offsets_small, qbase=20,
            writer_compat=None, decoder_compat=None, tweak=None):
    """A picture through the writer.  compat: the state the stream is written for and the decoder starts in;
    writer_compat: per component, where the two differ (the compat test fires); tweak (planes, qidx): a last change."""
    src = NC.Case(name, dtype, lw, lh, fmt, depth, counts, mode, fill, seed, qbase)
    if tweak:
        tweak(src)
    wc = [compat] * 3 if writer_compat is None else writer_compat
    # one writer call per component state: the stream is the concatenation (every sub-band starts on a byte)
    data = b""
    for k in range(3):
        planes = [p if j == k else np.zeros_like(p) for j, p in enumerate(src.planes)]
        full, used = ref.write_transform_data(planes, depth, src.hc, src.vc, mode, wc[k], src.qidx, offsets)
        # the component's own sub-bands: the others are one byte (0x80) each
        data += full[k * src.nsub:len(full) - (2 - k) * src.nsub]
    return Case(name, dtype, src.sizes, depth, src.hc, src.vc, mode, compat if decoder_compat is None else decoder_compat, is_intra,
                data, planes=src.planes)


# ---- fills beyond tests/noarith_enc_cases.py's --------------------------------------------------------------------------

def fill_last_one(case, rng):
    """All zeros but the last sample of every sub-band: 64 one-bit codes per chunk."""
    for k in range(3):
        for i in range(case.nsub):
            case.band(k, i)[-1, -1] = 1


def fill_zero_first_last(case, rng):
    """Zero first and last codeblocks, a zero first and a zero last sub-band."""
    NC.fill_random(case, rng, 60)
    for k in range(3):
        for i in range(case.nsub):
            b = case.band(k, i)
            hc, vc = case.counts(i)
            enc.get_codeblock(b, 0, 0, hc, vc)[...] = 0
            enc.get_codeblock(b, hc - 1, vc - 1, hc, vc)[...] = 0
    case.band(0, 0)[...] = 0
    case.band(2, case.nsub - 1)[...] = 0


def fill_boundary(case, rng):
    """depth 0, three components of one band: fifteen 4-bit codes behind 0, 3 and 1 one-bit codes, then 4-bit codes on: a
    code ends ON bit 64 in Y (15 x 4 + 4), one bit BEFORE it in U (3 + 15 x 4 = 63) and one bit BEHIND it in V (1 + 16 x 4)."""
    for p, zeros in zip(case.planes, (0, 3, 1)):
        v = np.where(np.arange(p.size) % 2, -1, 1)
        v[:zeros] = 0
        p[...] = v.reshape(p.shape)


def fill_eight_bit(case, rng, longer=0):
    """Sub-band 1 of component 0 alone: every value an 8-bit code (magnitudes 7 .. 14), `longer` of them a 10-bit one."""
    b = case.band(0, 1)
    v = rng.integers(7, 15, b.shape) * np.where(rng.random(b.shape) < 0.5, -1, 1)
    flat = v.reshape(-1)
    flat[:longer] = 17
    b[...] = flat.reshape(b.shape)


def code_bits(v):
    v = abs(int(v))
    return 2 * (v + 1).bit_length() - 1 + (v != 0)


MIXED_COUNTS = [(1, 1), (2, 1), (3, 2), (4, 3)]
COUNTS = {"one": [(1, 1)], "two": [(2, 2)], "three": [(3, 2)], "mixed": MIXED_COUNTS}


def _cases():
    out = []
    # luma 16 x 8 and 32 x 16 at depths 0 .. 3, the three chroma formats; counts, mode, compat and the sample size rotate
    # so that every value of each meets every geometry class
    n = 0
    for (lw, lh) in ((16, 8), (32, 16)):
        for depth in range(4):
            for fmt in (420, 422, 444):
                for dtype in (np.int16, np.int32):
                    cname = list(COUNTS)[(n // 2) % 4]
                    mode, compat, intra = (n // 2 + n // 8) % 2, (n // 4 + n) % 2, (n // 3) % 2
                    t = "s16" if dtype == np.int16 else "s32"
                    name = "%s-%dx%d-%d-d%d-%s-m%d-c%d" % (t, lw, lh, fmt, depth, cname, mode, compat)
                    out.append(written(name, dtype, lw, lh, fmt, depth, COUNTS[cname], mode, compat, NC.fill_sparse, 100 + n, intra))
                    n += 1
    for dtype in (np.int16, np.int32):
        t = "s16" if dtype == np.int16 else "s32"
        # every (counts, mode, compat) at one geometry
        for cname, counts in COUNTS.items():
            for mode in (0, 1):
                for compat in (0, 1):
                    out.append(written("%s-all-%s-m%d-c%d" % (t, cname, mode, compat), dtype, 32, 16, 420, 2, counts, mode, compat,
                                       NC.fill_random, 7, is_intra=compat))

        # the compat test fires in component 0: the stream has no offsets on its 1 x 1 sub-bands, the decoder starts with
        # compat off, and header index 58 + first value 5 leaves 0 .. 60
        def fire0(src):
            src.qidx[0][0] = 58
            src.band(0, 0)[0, 0] = 5
        out.append(written(t + "-compat-fires-c0", dtype, 32, 16, 420, 2, MIXED_COUNTS, 1, 1, NC.fill_random, 21, tweak=fire0,
                           decoder_compat=0))

        # ... in component 1 only: component 0 carries offsets (they keep the index in range), component 1 index 2 + (-7) < 0
        def fire1(src):
            src.qidx[1][0] = 2
            src.band(1, 0)[0, 0] = -7
        out.append(written(t + "-compat-fires-c1", dtype, 32, 16, 420, 2, MIXED_COUNTS, 1, 0, NC.fill_random, 22, tweak=fire1,
                           writer_compat=[0, 1, 1]))
        # offsets that clamp at 60 and at 0
        out.append(written(t + "-clamp-60", dtype, 32, 16, 420, 1, COUNTS["two"], 1, 0, NC.fill_random, 23, qbase=57,
                           offsets=lambda k, i, x, y: 3))
        out.append(written(t + "-clamp-0", dtype, 32, 16, 420, 1, COUNTS["two"], 1, 0, NC.fill_random, 24, qbase=1,
                           offsets=lambda k, i, x, y: -3 if (i + k) % 4 == 0 else 0))
        out.append(written(t + "-zero-first-last", dtype, 32, 16, 422, 2, COUNTS["three"], 1, 1, fill_zero_first_last, 25))
        out.append(written(t + "-all-zero", dtype, 32, 16, 420, 2, COUNTS["two"], 1, 0, NC.fill_zero, 26, is_intra=1))
        # codeblocks of no width: 127 and 128 columns of codeblocks in a 16-wide band -- many heads inside one chunk
        out.append(written(t + "-heads-127", dtype, 32, 16, 420, 1, [(1, 1), (127, 1)], 1, 1, NC.fill_random, 27))
        out.append(written(t + "-heads-128", dtype, 32, 16, 420, 1, [(1, 1), (128, 1)], 1, 0, NC.fill_random, 28))
        out.append(written(t + "-longest", dtype, 32, 16, 420, 1, COUNTS["one"], 0, 0, NC.fill_longest, 29))
        out.append(written(t + "-extremes", dtype, 32, 16, 444, 1, COUNTS["two"], 1, 1, NC.fill_extremes, 30))
        out.append(written(t + "-64-per-chunk", dtype, 64, 32, 444, 1, COUNTS["one"], 0, 0, fill_last_one, 31))
        out.append(written(t + "-boundary", dtype, 40, 4, 444, 0, COUNTS["one"], 0, 0, fill_boundary, 32))
    # CHAIN_THREADS: a 128 x 64 band of 8-bit codes is 8192 bytes, 1024 chunks: thread 0 takes the first, the scan the other
    # 1023 in one step; with 96 ten-bit codes it is 1027 chunks, two steps
    out.append(written("s16-chain-one-step", np.int16, 256, 128, 444, 1, COUNTS["one"], 0, 0, fill_eight_bit, 33))
    out.append(written("s16-chain-two-steps", np.int16, 256, 128, 444, 1, COUNTS["one"], 0, 0,
                       lambda c, r: fill_eight_bit(c, r, 96), 34))
    # the same band cut into 2 x 2 codeblocks with offsets: the chain crosses the step inside the second codeblock row
    out.append(written("s32-chain-codeblocks", np.int32, 256, 128, 444, 1, [(1, 1), (2, 2)], 1, 0, lambda c, r: fill_eight_bit(c, r, 300), 35))
    # FILL_GRID_X: 8 rows x 130 columns of codeblocks = 1040 row pieces
    out.append(written("s16-fill-1040", np.int16, 32, 16, 420, 1, [(1, 1), (130, 1)], 0, 0, NC.fill_sparse, 36))
    return out


# ---- hostile streams ------------------------------------------------------------------------------------------------------

def split(data, nsb):
    """[(stated length, quant index, payload)] of a well-formed stream."""
    un = ref.Reader(data, 64)
    out = []
    for _ in range(nsb):
        un.byte_sync()
        length = un.decode_uint()
        if length == 0:
            un.byte_sync()
            out.append((0, 0, b""))
            continue
        qi = un.decode_uint()
        un.byte_sync()
        first = un.pos >> 3
        out.append((length, qi, data[first:first + length]))
        un.pos += 8 * length
    return out


def join(bands):
    pack = enc.Pack()
    for length, qi, payload in bands:
        pack.sync()
        pack.encode_uint(length)
        if length:
            pack.encode_uint(qi)
            pack.sync()
            pack.append(payload)
    pack.sync()
    return bytes(pack.data)


def _hostile():
    out = []
    for dtype in (np.int16, np.int32):
        t = "s16" if dtype == np.int16 else "s32"
        base = written(t + "-hostile-base", dtype, 32, 16, 420, 2, COUNTS["two"], 1, 0, NC.fill_random, 41)
        bands = split(base.data, 3 * base.nsub)
        assert join(bands) == base.data
        big = max(range(len(bands)), key=lambda n: bands[n][0])         # the longest payload: a middle sub-band
        assert 0 < big < len(bands) - 1 and bands[big][0] > 8
        last = len(bands) - 1
        assert bands[last][0] > 0

        def damaged(name, change, data_bytes=None, compat=0):
            b = list(bands)
            change(b)
            nbytes = data_bytes(b) if callable(data_bytes) else data_bytes
            return Case("%s-%s" % (t, name), dtype, base.sizes, base.depth, base.hc, base.vc, base.mode, compat, 0, join(b), nbytes)

        def cut(n, keep):
            def change(b):
                length, qi, payload = b[n]
                b[n] = (keep(length), qi, payload[:keep(length)])
            return change

        def stated(n, more, junk=b""):
            def change(b):
                length, qi, payload = b[n]
                b[n] = (length + more, qi, payload + junk)
            return change

        def payload_of(n, make):
            def change(b):
                length, qi, payload = b[n]
                b[n] = (length, qi, make(length))
            return change

        def index_of(n, qi):
            def change(b):
                length, _, payload = b[n]
                if length == 0:
                    length, payload = 1, b"\xff"
                b[n] = (length, qi, payload)
            return change

        out.append(damaged("payload-cut-1", cut(big, lambda l: l - 1)))
        out.append(damaged("payload-cut-to-1", cut(big, lambda l: 1)))
        # the last sub-band's payload ends the input: its length says 1 and 1000 bytes more
        out.append(damaged("length-past-1", stated(last, 1)))
        out.append(damaged("length-past-1000", stated(last, 1000)))
        out.append(damaged("length-past-middle", stated(big, 1 << 20), data_bytes=lambda b: len(join(b[:big + 1])) - 3))
        out.append(damaged("trailing-junk", stated(big, 5, b"\x00\x5a\xff\x01\x80")))
        out.append(damaged("zeros-payload", payload_of(big, lambda l: b"\x00" * l)))
        for seed in (1, 2, 3):
            def rand(b, seed=seed):
                rng = np.random.default_rng(seed)
                for n, (length, qi, payload) in enumerate(b):
                    if length:
                        b[n] = (length, qi, rng.integers(0, 256, length, dtype=np.uint8).tobytes())
            out.append(damaged("random-payloads-%d" % seed, rand, compat=seed & 1))
        out.append(damaged("index-61-first", index_of(0, 61)))
        out.append(damaged("index-61-middle", index_of(big, 61)))
        out.append(damaged("index-61-last", index_of(last, 200)))
        out.append(damaged("index-60-last", index_of(last, 60)))
        out.append(Case(t + "-empty-input", dtype, base.sizes, base.depth, base.hc, base.vc, base.mode, 0, 0, b""))
    return out


CASES = _cases()
HOSTILE = _hostile()
BY_NAME = {c.name: c for c in CASES + HOSTILE}
assert len(BY_NAME) == len(CASES) + len(HOSTILE)
# three unlike pictures in one call, per sample size
MIXED = {2: [CASES[12].name, "s16-compat-fires-c1", "s16-heads-128"], 4: [CASES[37].name, "s32-clamp-60", "s32-extremes"]}
assert all(BY_NAME[n].dtype.itemsize == b for b, names in MIXED.items() for n in names)


# ---- the properties the cases are named for --------------------------------------------------------------------------------

def _check_properties():
    rotation = {(c.mode, c.compat, tuple(c.hc[:1])) for c in CASES[:48]}
    assert {m for m, _, _ in rotation} == {0, 1} and {c for _, c, _ in rotation} == {0, 1}
    for t in ("s16", "s32"):
        # the compat test fires where the name says
        for name, comp in ((t + "-compat-fires-c0", 0), (t + "-compat-fires-c1", 1)):
            case = BY_NAME[name]
            assert case.compat == 0 and case.expected()[2]["compat_quant_offset"] == 1, name
            assert all(np.array_equal(a, b) for a, b in zip(case.expected()[1], case.planes)), name
            # ... and not before: the components in front of it alone leave the state off
            bands = split(case.data, 3 * case.nsub)
            head = join(bands[:comp * case.nsub] + [(0, 0, b"")] * ((3 - comp) * case.nsub))
            planes = [np.zeros_like(p) for p in case.planes]
            assert ref.decode_transform_data(head, planes, None, case.depth, case.hc, case.vc, case.mode, 0, 0)["compat_quant_offset"] == 0
        assert BY_NAME[t + "-clamp-60"].expected()[2]["clamped_quant"] > 0 and BY_NAME[t + "-clamp-0"].expected()[2]["clamped_quant"] > 0
        z = BY_NAME[t + "-zero-first-last"].expected()[2]["subband_length"]
        assert z[0, 0] == 0 and z[2, BY_NAME[t + "-zero-first-last"].nsub - 1] == 0 and z[0, 1:].any()
        for name, cols in ((t + "-heads-127", 127), (t + "-heads-128", 128)):
            case = BY_NAME[name]
            assert case.counts(1) == (cols, 1) and enc.subband(case.planes[0], 1, 1).shape[1] == 16
        # a code per chunk or longer; 64 codes in a chunk
        case = BY_NAME[t + "-longest"]
        assert all(code_bits(v) in (32, 64) for v in case.planes[0].reshape(-1)[:8].tolist())
        assert code_bits(case.planes[0][0, 0]) >= (CHUNK_BITS if t == "s32" else CHUNK_BITS // 2)
        assert enc.subband(BY_NAME[t + "-64-per-chunk"].planes[0], 1, 1).size >= 4 * CHUNK_BITS
        # codes that end on, one bit before and one bit behind the first chunk's end
        ends = []
        for p in BY_NAME[t + "-boundary"].planes:
            ends.append(set(np.cumsum([code_bits(v) for v in p.reshape(-1).tolist()]).tolist()))
        assert CHUNK_BITS in ends[0] and CHUNK_BITS - 1 in ends[1] and CHUNK_BITS not in ends[1] and CHUNK_BITS + 1 in ends[2] \
            and CHUNK_BITS not in ends[2]
    chunks = lambda name: -(-int(BY_NAME[name].expected()[2]["subband_length"][0, 1]) * 8 // CHUNK_BITS)
    assert chunks("s16-chain-one-step") - 1 <= CHAIN_THREADS < chunks("s16-chain-two-steps") - 1
    assert chunks("s32-chain-codeblocks") - 1 > CHAIN_THREADS
    case = BY_NAME["s16-fill-1040"]
    assert enc.subband(case.planes[0], 1, 1).shape[0] * case.counts(1)[0] == 1040 > FILL_GRID_X
    assert enc.subband(BY_NAME["s16-heads-128"].planes[0], 1, 1).shape[0] * 128 <= FILL_GRID_X
    for t in ("s16", "s32"):
        r = lambda name: BY_NAME["%s-%s" % (t, name)].expected()[2]
        assert r("payload-cut-1")["error"] == 0 and r("payload-cut-to-1")["overran"] >= 1
        assert r("length-past-1")["truncated"] == 1 and r("length-past-1000")["truncated"] == 1
        assert r("length-past-middle")["truncated"] == 1
        assert r("trailing-junk")["not_consumed"] >= 1
        assert r("zeros-payload")["long_codes"] >= 1
        assert r("index-61-first")["error"] == 1 and r("index-61-first")["first_error"] == 0
        assert r("index-61-middle")["error"] == 1 and 0 < r("index-61-middle")["first_error"] < 2 * 19 + 6
        assert r("index-61-last")["error"] == 1 and r("index-61-last")["first_error"] == 2 * 19 + 6
        assert r("index-60-last")["error"] == 0
        assert r("empty-input")["bytes_read"] == 3 * 7 and not r("empty-input")["subband_length"].any()


_check_properties()


# ---- the refusal table: (name, change to a valid picture description, fragment of the message) ---------------------------
# A description is a dict: bpp, depth, mode, sizes [(w, h)] * 3, hc, vc, stride [3], bytes [3], coeffs [3], quant [3] (or
# None), data, data_bytes, bytes_on_device, result (addresses; nothing is dereferenced by the check).

def describe(lw=32, lh=16, fmt=420, depth=2, counts=((2, 2),), mode=1, bpp=2):
    sizes = NC.iwt_sizes(lw, lh, fmt, depth)
    counts = list(counts) + [counts[-1]] * (depth + 1 - len(counts))
    d = {"bpp": bpp, "depth": depth, "mode": mode, "sizes": sizes, "hc": [c[0] for c in counts], "vc": [c[1] for c in counts]}
    d["stride"] = [(w * bpp + 63) // 64 * 64 for w, h in sizes]
    d["bytes"] = [s * h for s, (w, h) in zip(d["stride"], sizes)]
    d["coeffs"] = [0x10000000, 0x20000000, 0x30000000]
    d["quant"] = [0x14000000, 0x24000000, 0x34000000]
    d["data"], d["data_bytes"], d["bytes_on_device"], d["result"] = 0x40000000, 1 << 20, 0, 0x50000000
    return d


_set, _size = NC._set, NC._size

REFUSALS = [
    ("bpp-1", _set("bpp", 1), "bytes_per_sample must be 2 or 4"),
    ("bpp-3", _set("bpp", 3), "bytes_per_sample must be 2 or 4"),
    ("depth-7", _set("depth", 7), "transform_depth 7"),
    ("depth-negative", _set("depth", -1), "transform_depth -1"),
    ("width-odd", _size(1, 18, 4), "picture 0, component 1"),
    ("height-zero", _size(2, 16, 0), "picture 0, component 2"),
    ("width-32768", _size(0, 32768, 16), "picture 0, component 0"),
    ("counts-zero", _set("hc", 0, 1), "codeblocks at level 1"),
    ("counts-32768", _set("vc", 32768, 0), "codeblocks at level 0"),
    ("mode-2", _set("mode", 2), "codeblock_mode_index 2"),
    ("data-null", _set("data", 0), "data is NULL"),
    ("data-2^29", _set("data_bytes", 1 << 29), "bit positions are 32-bit"),
    ("length-word-odd", _set("bytes_on_device", 0x60000002), "bytes_on_device is unaligned"),
    ("result-null", _set("result", 0), "result is NULL or unaligned"),
    ("result-odd", _set("result", 0x50000002), "result is NULL or unaligned"),
    ("coeffs-null", _set("coeffs", 0, 1), "coeffs[1] is NULL or misaligned"),
    ("coeffs-odd", _set("coeffs", 0x30000001, 2), "coeffs[2] is NULL or misaligned"),
    ("quant-one-null", _set("quant", 0, 1), "quant[1] is NULL or misaligned"),
    ("quant-odd", _set("quant", 0x34000001, 2), "quant[2] is NULL or misaligned"),
    ("stride-short", _set("stride", 62, 0), "stride[0] 62"),
    ("stride-odd", _set("stride", 65, 1), "stride[1] 65"),
    ("plane-short", _set("bytes", 64 * 15 + 32 * 2 - 1, 0), "component 0: 16 rows of 32 samples at stride 64 reach outside"),
    ("data-overlaps-coeffs", _set("data", 0x20000010 - (1 << 20) + 1), "data overlaps coeffs[1]"),
    ("data-overlaps-quant", _set("data", 0x34000000 + 7), "data overlaps quant[2]"),
    ("quant-overlaps-coeffs", _set("quant", 0x20000000 + 64, 0), "quant[0] overlaps coeffs[1]"),
    ("result-in-plane", _set("result", 0x10000000 + 64), "result overlaps coeffs[0]"),
    ("result-in-data", _set("result", 0x40000000 + (1 << 20) - 4), "result overlaps data"),
    ("result-on-length-word", lambda d: d.update(bytes_on_device=0x50000000 + 320), "result overlaps bytes_on_device"),
    ("length-word-in-plane", _set("bytes_on_device", 0x24000000 + 8), "bytes_on_device overlaps quant[1]"),
    ("coeffs-overlap", _set("coeffs", 0x10000000 + 64 * 16 - 4, 1), "coeffs[1] overlaps coeffs[0]"),
    ("quant-overlap", _set("quant", 0x14000000 + 2, 2), "quant[2] overlaps quant[0]"),
]
# the other side of limits that have one: these descriptions pass
ACCEPTED = [
    ("plain", lambda d: None),
    ("no-quant", _set("quant", None)),
    ("depth-6", lambda d: d.update(describe(64, 64, 444, 6, ((1, 1),), 0, d["bpp"]))),
    ("depth-0", lambda d: d.update(describe(10, 6, 420, 0, ((2, 2),), 1, d["bpp"]))),
    ("counts-32767", lambda d: d.update(describe(32, 16, 420, 1, ((32767, 1), (1, 1)), 0, d["bpp"]))),
    ("width-32767-ish", lambda d: d.update(describe(32766, 2, 444, 1, ((1, 1),), 0, d["bpp"]))),
    ("plane-exact", lambda d: d["bytes"].__setitem__(0, d["stride"][0] * 15 + 32 * d["bpp"])),
    ("data-below-2^29", lambda d: d.update(data_bytes=(1 << 29) - 1, result=0x70000000)),
    ("data-empty", lambda d: d.update(data=0, data_bytes=0)),
    ("data-ends-at-plane", _set("data", 0x20000000 - (1 << 20))),
    ("length-word", _set("bytes_on_device", 0x60000004)),
    ("result-behind-data", _set("result", 0x40000000 + (1 << 20))),
    ("length-word-behind-result", lambda d: d.update(bytes_on_device=0x50000000 + 324)),
    ("coeffs-touch", lambda d: d["coeffs"].__setitem__(1, 0x10000000 + d["bytes"][0])),
]


def c_picture(d, L):
    """The _lib.NoarithDecodePicture of a description."""
    a = L.NoarithDecodePicture()
    a.data, a.data_bytes, a.bytes_on_device = d["data"] or None, d["data_bytes"], d["bytes_on_device"] or None
    for k in range(3):
        a.coeffs[k], a.bytes[k], a.stride[k] = d["coeffs"][k] or None, d["bytes"][k], d["stride"][k]
        a.quant[k] = (d["quant"][k] or None) if d["quant"] is not None else None
        a.iwt_width[k], a.iwt_height[k] = d["sizes"][k]
    a.transform_depth, a.codeblock_mode_index = d["depth"], d["mode"]
    for l in range(min(len(d["hc"]), 7)):
        a.horiz_codeblocks[l], a.vert_codeblocks[l] = d["hc"][l], d["vc"][l]
    a.is_intra, a.compat_quant_offset, a.result = 0, 0, d["result"] or None
    return a
