"""The seeded cases of the quantiser choice (tests/test_gpu_quant_choose.py) and what tests/test_quant_choose_draws.py
walks without a device.  The stage's input is 104 counts per sub-band, so the counts are drawn directly: a two-sided
geometric fall-off over |v| of a drawn scale, as wavelet coefficients have, `n` sampled values per sub-band.

The encoder state the stage takes as input is made here, not copied: the error table from
quant_choose_ref.make_error_table (|dequantise (quantise (x)) - x| ** 4 with tests/quant_ref.py's arithmetic), seeded
positive doubles for the one-bits / zero-bits tables, drawn weights, ratios and scales.

Targets of the two searching engines are written relative to the picture -- ("between", la, lb): halfway between the
engine's sums at frame lambdas la and lb -- so that a case says which steps its search takes; ("abs", v) is v."""
import functools
import struct

import numpy as np

import quant_choose_ref as R

BINS, NB_MAX = R.BINS, R.MAX_BANDS
SCALES = (10.0, 0.1, 0.5)               # sub-band 0, chroma, diagonal


@functools.lru_cache(maxsize=None)
def error_table():
    return R.make_error_table(4.0, True)


@functools.lru_cache(maxsize=None)
def bit_tables():
    """(onebits, zerobits): 60 x 104 positive doubles each, seeded"""
    rng = np.random.default_rng(4242)
    return rng.uniform(0.05, 6.0, (R.INDICES, BINS)), rng.uniform(0.05, 6.0, (R.INDICES, BINS))


def fall_off(rng, n, scale):
    """104 counts of n values whose |v| falls off geometrically with `scale`"""
    first = np.array([R.iexpx(i) for i in range(BINS + 1)], np.float64)
    p = np.exp(-first[:-1] / scale) - np.exp(-first[1:] / scale)
    p[0] *= 0.5 + rng.uniform(0, 2)     # the zero bin is its own matter
    return rng.multinomial(n, p / p.sum()).astype(np.uint32)


def one_bin(i, count):
    c = np.zeros(BINS, np.uint32)
    c[i] = count
    return c


def picture(seed, depth, intra=True, noarith=True, skips=None, special=None, n_lo=200, n_hi=6000, heavy=1.0):
    """One picture's inputs.  special: {(component, sub-band): 104 counts or (104 counts, overflow)} replaces drawn
    sub-bands; skips: per sub-band, default the reference's 1 << max (0, level - 1); heavy: a factor on the drawn weights
    (lambda is divided by weight * weight: heavy weights move the whole curve towards large frame lambdas, where the
    searches that step UP three and five times find their targets)."""
    rng = np.random.default_rng(seed)
    nb = R.n_bands(depth)
    counts = np.zeros((3, nb, BINS + 1), np.uint32)
    for c in range(3):
        for i in range(nb):
            level = R.position(i) >> 2
            scale = rng.uniform(1.0, 30.0) * 2.0 ** (max(depth - level, 0) * rng.uniform(0.3, 1.0)) * (0.5 if c else 1.0)
            counts[c, i, :BINS] = fall_off(rng, int(rng.integers(n_lo, n_hi)), scale)
            counts[c, i, BINS] = rng.integers(0, 3) if rng.random() < 0.2 else 0
    for (c, i), v in (special or {}).items():
        ovf = 0
        if isinstance(v, tuple):
            v, ovf = v
        counts[c, i, :BINS], counts[c, i, BINS] = v, ovf
    if skips is None:
        skips = [1 << max(0, (R.position(i) >> 2) - 1) for i in range(nb)]
    weight = np.ones(NB_MAX)
    weight[:nb] = rng.uniform(0.4, 3.0, nb) * heavy
    ratio = np.ones((3, NB_MAX))
    ratio[:, :nb] = rng.uniform(0.7, 1.3, (3, nb))
    return dict(depth=depth, is_intra=int(intra), is_noarith=int(noarith), counts=counts, skip=[int(s) for s in skips],
                weight=weight, ratio=ratio, scales=SCALES)


FULL = 0xffffffff
PICTURES = {
    "d0": lambda: picture(1, 0),
    "d3": lambda: picture(2, 3),
    "d3_inter": lambda: picture(3, 3, intra=False),
    "d3_heavy": lambda: picture(11, 3, heavy=1e4),
    "d3_arith": lambda: picture(4, 3, noarith=False),
    "d6": lambda: picture(5, 6, intra=False),
    "d6_arith": lambda: picture(6, 6, noarith=False),
    "d2_skips": lambda: picture(7, 2, skips=[1, 2, 4, 8, 16, 32, 1]),
    # one sample in all; a bin of 2^32 - 1 counts under skip 32 (alone in its sub-band: a band has fewer than 2^32 sampled
    # values in all); every sampled value in `overflow` (the NaN row); every coefficient zero (bin[1] == 0 for all indices)
    "d1_edges": lambda: picture(8, 1, skips=[1, 32, 32, 1], special={
        (0, 0): one_bin(37, 1), (0, 1): one_bin(0, FULL), (0, 2): one_bin(103, FULL), (1, 0): one_bin(0, 1),
        (1, 1): (np.zeros(BINS, np.uint32), 77), (1, 2): one_bin(0, 5000), (2, 3): one_bin(50, FULL)}),
    "d2_nan": lambda: picture(9, 2, special={(2, 4): (np.zeros(BINS, np.uint32), 5)}),
    "d2_nan_arith": lambda: picture(10, 2, noarith=False, special={(0, 3): (np.zeros(BINS, np.uint32), 1)}),
}


@functools.lru_cache(maxsize=None)
def get(name):
    return PICTURES[name]()


def bins_of(pic):
    nb = R.n_bands(pic["depth"])
    return [[R.scaled_bins(pic["counts"][c, i], pic["skip"][i]) for i in range(nb)] for c in range(3)]


@functools.lru_cache(maxsize=None)
def estimates(name):
    """(est_entropy, est_error) of a picture by the restatement; computed once, shared, not to be written to"""
    pic = get(name)
    one, zero = bit_tables()
    ent, err = R.calc_estimates(bins_of(pic), pic["depth"], pic["is_noarith"], pic["ratio"], error_table(), one, zero)
    ent.setflags(write=False)
    err.setflags(write=False)
    return ent, err


ESTIMATE_CASES = list(PICTURES)

L, B, E = R.ENGINE_LAMBDA, R.ENGINE_BIT_ALLOCATION, R.ENGINE_CONSTANT_ERROR
ENGINE_CASES = (
    [("d3", L, ("abs", 10.0 ** e)) for e in (-10, -7, -4, -2, 0, 1, 3, 6, 10)]
    + [("d6_arith", L, ("abs", 10.0 ** e)) for e in (-10, -3, 0, 2, 10)]
    + [("d0", L, ("abs", 3.7)), ("d1_edges", L, ("abs", 0.02)), ("d2_nan", L, ("abs", 1.0)), ("d2_nan_arith", L, ("abs", 0.5))]
    # bit allocation: up by 1, 3 and 5 steps, down by 1, 2 and 5, the five steps exhausted both ways (each ends in the
    # early lo == hi return), a NaN sum (every comparison false: five steps down, seven halvings, no early return)
    + [("d3", B, ("between", 1.0, 100.0)), ("d3_heavy", B, ("between", 1e4, 1e6)), ("d3_heavy", B, ("between", 1e8, 1e10)),
       ("d3", B, ("between", 0.01, 1.0)), ("d3_arith", B, ("between", 1e-4, 1e-2)), ("d6", B, ("between", 1e-10, 1e-8)),
       ("d3", B, ("abs", 1e30)), ("d3_inter", B, ("abs", 0.0)), ("d6", B, ("abs", 1e30)), ("d0", B, ("between", 1.0, 100.0)),
       ("d2_nan", B, ("abs", 5000.0)), ("d2_nan_arith", B, ("between", 0.01, 1.0)), ("d2_skips", B, ("between", 1.0, 0.01)),
       ("d1_edges", B, ("abs", 1e6))]         # (it has a NaN sub-band: its entropy sums are NaN, a target between two is none)
    # constant error: the same branches in its mirrored sense
    + [("d3", E, ("between", 1.0, 100.0)), ("d3_heavy", E, ("between", 1e4, 1e6)), ("d3_heavy", E, ("between", 1e8, 1e10)),
       ("d3_inter", E, ("between", 0.01, 1.0)), ("d6", E, ("between", 1e-4, 1e-2)), ("d6_arith", E, ("between", 1e-10, 1e-8)),
       ("d3", E, ("abs", 0.0)), ("d3", E, ("abs", 1e300)), ("d0", E, ("between", 0.03, 0.6)), ("d2_nan", E, ("between", 1.0, 100.0)),
       ("d2_skips", E, ("between", 100.0, 1e4)), ("d1_edges", E, ("between", 0.01, 1.0))]
)


def target_of(name, engine, spec):
    if spec[0] == "abs":
        return float(spec[1])
    pic = get(name)
    ent, err = estimates(name)
    ev = R.Evaluator(ent, err, pic["depth"], pic["weight"], pic["scales"])
    f = ev.lambda_to_error if engine == E else ev.lambda_to_entropy
    return 0.5 * (f(spec[1]) + f(spec[2]))


@functools.lru_cache(maxsize=None)
def expected(k):
    """the restatement's answer to ENGINE_CASES[k] and its trace; computed once, shared"""
    name, engine, spec = ENGINE_CASES[k]
    pic = get(name)
    ent, err = estimates(name)
    trace = []
    target = target_of(name, engine, spec)
    out = R.choose(ent, err, pic["depth"], pic["weight"], pic["scales"], engine, target, trace)
    out["target"] = target
    return out, trace


# eight unlike pictures in one call (depth, form, engine mixed), as indices into ENGINE_CASES by picture name and engine
def case_index(name, engine, nth=0):
    hits = [k for k, c in enumerate(ENGINE_CASES) if c[0] == name and c[1] == engine]
    return hits[nth]


MIXED_BATCH = [("d6", B), ("d0", L), ("d3_arith", B), ("d1_edges", L), ("d6_arith", E), ("d2_nan", B), ("d3_inter", E), ("d2_skips", E)]


MARGIN = 1e-6


def bits(x):
    return struct.pack("<d", x)


def check_trace(trace, what):
    """the two margins over everything an engine's run compared (tests/test_quant_choose_draws.py says why): the runner-up
    of every argmin a relative MARGIN above the winner or equal to it as bits; the two sides of every comparison of sums
    a relative MARGIN apart, equal as bits, or one of them NaN"""
    for rec in trace:
        if rec[0] == "argmin":
            _, jmin, xs = rec
            w = xs[jmin]
            if w != w:
                assert jmin == 0
                continue
            for j, x in enumerate(xs):
                if j == jmin or x != x:
                    continue
                assert bits(x) == bits(w) or x - w >= MARGIN * abs(w), (what, "argmin", jmin, j, w, x)
                if bits(x) == bits(w):
                    assert j > jmin
        else:
            _, a, b = rec
            if a != a or b != b:
                continue
            assert bits(a) == bits(b) or abs(a - b) >= MARGIN * max(abs(a), abs(b)), (what, "compare", a, b)
