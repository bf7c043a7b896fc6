"""The checker of the quantiser choice (schro_hip_quant_choose_batch): the reference's estimate and choice code restated
in plain Python / numpy on IEEE doubles -- no fused operation, the reference's evaluation order -- from

  schrohistogram.c:24-40     iexpx, ilogx_size (ilogx: tests/hist_ref.py)
  schrohistogram.c:42-68     schro_histogram_get_range
  schrohistogram.c:70-90     schro_histogram_table_generate (only to MAKE a table: the stage applies tables, it owns none)
  schrohistogram.c:92-104    schro_histogram_apply_table
  schrohistogram.c:266-343   schro_histogram_estimate_entropy, both branches
  schroutils.c:309-327       schro_utils_probability_to_entropy, schro_utils_entropy
  schroquantiser.c:688-732   schro_encoder_calc_estimates
  schroquantiser.c:738-782   the drivers of rdo_bit_allocation, rdo_lambda, rdo_cbr
  schroquantiser.c:809-836   schro_subband_pick_quant
  schroquantiser.c:838-885   schro_encoder_lambda_to_entropy
  schroquantiser.c:887-969   schro_encoder_entropy_to_lambda
  schroquantiser.c:971-1014  schro_encoder_lambda_to_error
  schroquantiser.c:1016-1098 schro_encoder_error_to_lambda
  schroquantiser.c:1100-1119 the driver of constant_error (its target is the caller's: `error` as line 1115 passes it)

None of these files is among the sources the oracle recipe compiles, so nothing here is pinned on a compiled reference:
tests/test_quant_choose_ref.py holds it (histograms small enough to work by hand, identities of get_range, the sign of
the lambda sweep, a second formulation of the sums).

Encoder state is INPUT, not restated: encoder->intra_hist_tables (60 x 104 weights, `error_table`), the one-bits /
zero-bits tables (60 x 104 each, read only when is_noarith == 0), the sub-band weight table, the arith context ratios and
the three lambda scales.  schro_table_quant is the one table of the reference's read (tests/golden/quant_tables_encoder.json
through tests/quant_ref.py).

The reference's traps, kept:
  scaled bins          the bins are the raw counts times skip, as doubles (schro_histogram_scale); the overflow word of
                       SchroHipHistogramCounts is in no bin
  duplicate bin[0]     estimate_entropy computes bin[0] before its loop and again as the loop's i = 0: the same value
  empty sampled set    all 104 bins zero (every sampled value went to `overflow`, or the band is empty): the noarith
                       branch's bin[1] / bin[0] is 0 / 0 = NaN and the estimate is NaN for every index; NaN never
                       satisfies x < min, so pick_quant answers 0.  (The arith branch gives 0: schro_utils_entropy
                       returns 0 on total == 0.)
  first minimum wins   pick_quant: j == 0 unconditional, then strict <; a NaN at j > 0 never wins, a NaN at j = 0 is
                       never displaced
  the sub-band lambda  frame lambda, *= sub-band-0 scale (i == 0), *= chroma scale (component > 0), *= diagonal scale
                       (position & 3 == 3), then /= weight * weight -- in that order, each step rounded
  no diagonal scale    ... on the error path: lambda_to_error leaves the diagonal scale out
  stale indices        constant_error leaves the indices of its LAST bisection evaluation; it never evaluates at the
                       lambda it returns
  final evaluation     rdo_bit_allocation evaluates once more at the lambda it returns
  early return         lo == hi after the steps returns sqrt (lo * hi) at once (not_bracketed is then not looked at)
  unbracketed target   a target outside [lo, hi] is searched anyway
  evaluation counts    bit allocation: at most 1 + 5 + 7 + 1; constant error: at most 1 + 5 + 14
  get_range's end      bin 103 holds |v| 30720 .. 32767 and the range ends at 32000: 768 / 2048 of it is taken off
                       again, so get_range (0, 32000) is the bins' sum MINUS 0.375 bins[103]
"""
import math

import numpy as np

import quant_ref as Q

BINS = 104
INDICES = 60                    # quant indices an estimate is made for
MAX_BANDS = 19                  # 1 + 3 * 6
RANGE_END = 32000
N_RANGES = 12
INV_LOG_2 = 1.44269504088896338700      # schroutils.c:306

ENGINE_LAMBDA, ENGINE_BIT_ALLOCATION, ENGINE_CONSTANT_ERROR = 0, 1, 2


def ilogx(x):
    x, i = abs(int(x)), 0
    while x >= 16:
        x >>= 1
        i += 1
    return x + (i << 3)


def iexpx(x):
    if x < 8:
        return x
    return (8 | (x & 7)) << ((x >> 3) - 1)


def ilogx_size(i):
    return 1 if i < 8 else 1 << ((i >> 3) - 1)


def scaled_bins(counts, skip):
    """the 104 doubles of a SchroHistogram from raw counts (the first 104 words of SchroHipHistogramCounts)"""
    return np.asarray(counts, np.uint32)[:BINS].astype(np.float64) * float(skip)


def get_range(bins, start, end):
    """schrohistogram.c:42-68, term by term in its order"""
    if start >= end:
        return 0.0
    i = ilogx(start)
    size = ilogx_size(i)
    x = float(iexpx(i + 1) - start) / size * float(bins[i])
    i += 1
    iend = ilogx(end)
    while i <= iend:
        x += float(bins[i])
        i += 1
    size = ilogx_size(iend)
    x -= float(iexpx(iend + 1) - end) / size * float(bins[iend])
    return x


def table_generate(func):
    """schrohistogram.c:70-90: weights[i] = the mean of func over the values of bin i"""
    w = np.zeros(BINS, np.float64)
    for i in range(BINS):
        s = 0.0
        for j in range(iexpx(i), iexpx(i + 1)):
            s += func(j)
        w[i] = s / ilogx_size(i)
    return w


def make_error_table(power=4.0, is_intra=True):
    """A table of the encoder's kind, made the way schro_encoder_init_error_tables makes one -- per index the mean over a
    bin of |dequantise (quantise (x)) - x| ** power -- with tests/quant_ref.py's arithmetic.  60 x 104 doubles."""
    t = np.zeros((INDICES, BINS), np.float64)
    x = np.arange(0, iexpx(BINS), dtype=np.int64)
    for j in range(INDICES):
        _, r = Q.quantise_s32(x, j, is_intra)           # schro_quantise, then schro_dequantise, vectorised
        vals = np.abs(r.astype(np.int64) - x).astype(np.float64) ** power
        for i in range(BINS):
            # (cumsum adds in index order, as table_generate's loop does)
            t[j, i] = np.cumsum(vals[iexpx(i):iexpx(i + 1)])[-1] / ilogx_size(i)
    return t


def apply_table(bins, weights):
    """schrohistogram.c:92-104: the serial sum in index order, each product rounded before it is added"""
    s = 0.0
    for i in range(BINS):
        s += float(bins[i]) * float(weights[i])
    return s


def apply_tables(bins, table):
    """apply_table for every row of a (n, 104) table at once: the same operations per row, in the same order"""
    table = np.asarray(table, np.float64)
    s = np.zeros(table.shape[0], np.float64)
    for i in range(BINS):
        s = s + float(bins[i]) * table[:, i]
    return s


def probability_to_entropy(x):
    if x <= 0 or x >= 1.0:
        return 0.0
    return -(x * math.log(x) + (1 - x) * math.log(1 - x)) * INV_LOG_2


def utils_entropy(a, total):
    if total == 0:
        return 0.0
    return probability_to_entropy(a / total) * total


def _div(a, b):
    """a / b as C has it: 0 / 0 is NaN"""
    if b == 0:
        return float("nan") if a == 0 or a != a else math.copysign(float("inf"), a)
    return a / b


def range_start(quant_index, i):
    return (Q.quant_factor(quant_index) * ((1 << i) - 1) + 3) // 4


def estimate_entropy(bins, quant_index, noarith, onebits=None, zerobits=None):
    """schrohistogram.c:266-343.  onebits / zerobits: the 104 weights of this index (arith branch only)."""
    est = 0.0
    b = [0.0] * N_RANGES
    b[0] = get_range(bins, 0, RANGE_END)
    for i in range(N_RANGES):
        b[i] = get_range(bins, range_start(quant_index, i), RANGE_END)
    if not noarith:
        est += b[1]
        for i in range(1, 6):
            est += utils_entropy(b[i], b[i - 1])
        post5 = 0.0
        for i in range(6, N_RANGES):
            post5 += b[i]
        est += utils_entropy(post5, post5 + b[5])
        ones = apply_table(bins, onebits)
        zeros = apply_table(bins, zerobits)
        est += utils_entropy(ones, zeros + ones)
    else:
        x = _div(b[1], b[0])
        x = 1.0 - math.exp(-0.5 * 25 * x)
        est += x * b[0] + (1 - x) * b[1]
        est += b[1]
        for i in range(1, N_RANGES):
            est += 2 * b[i]
    return est


def n_bands(depth):
    return 1 + 3 * depth


def position(index):
    return 0 if index == 0 else (((index - 1) // 3) << 2) | ((index - 1) % 3 + 1)


def calc_estimates(bins, depth, noarith, ratio, error_table, onebits=None, zerobits=None):
    """schroquantiser.c:688-732.  bins[c][i]: the scaled bins of component c, sub-band i; ratio[c][i].  Returns
    (est_entropy, est_error), float64 arrays [3][1 + 3 depth][60]."""
    nb = n_bands(depth)
    ent = np.zeros((3, nb, INDICES), np.float64)
    err = np.zeros((3, nb, INDICES), np.float64)
    for c in range(3):
        for i in range(nb):
            for j in range(INDICES):
                e = estimate_entropy(bins[c][i], j, noarith, None if noarith else onebits[j], None if noarith else zerobits[j])
                e *= float(ratio[c][i])
                ent[c, i, j] = e
            err[c, i] = apply_tables(bins[c][i], error_table)
    return ent, err


def pick_quant(entropy, error, lam, trace=None):
    """schroquantiser.c:809-836 on one sub-band's 60 + 60 estimates"""
    j_min, mn = -1, 0.0
    xs = []
    for j in range(INDICES):
        x = float(entropy[j]) + lam * float(error[j])
        xs.append(x)
        if j == 0 or x < mn:
            j_min, mn = j, x
    if trace is not None:
        trace.append(("argmin", j_min, xs))
    return j_min


def subband_lambda(frame_lambda, component, i, weight, scales, diagonal):
    """schroquantiser.c:862-875 (diagonal: the entropy path) / :994-1004 (the error path, without it)"""
    lam = float(frame_lambda)
    if i == 0:
        lam *= float(scales[0])
    if component > 0:
        lam *= float(scales[1])
    if diagonal and (position(i) & 3) == 3:
        lam *= float(scales[2])
    w = float(weight[i])
    lam /= w * w
    return lam


class Evaluator:
    """lambda_to_entropy / lambda_to_error over one picture's estimates; remembers the indices of its last evaluation as
    frame->quant_indices does."""

    def __init__(self, ent, err, depth, weight, scales, trace=None):
        self.ent, self.err, self.nb = ent, err, n_bands(depth)
        self.weight, self.scales, self.trace = weight, scales, trace
        self.indices = np.zeros((3, self.nb), np.int32)
        self.evaluations = 0
        self.last_sum = 0.0

    def _run(self, frame_lambda, on_error):
        total = 0.0
        for c in range(3):
            for i in range(self.nb):
                lam = subband_lambda(frame_lambda, c, i, self.weight, self.scales, diagonal=not on_error)
                q = pick_quant(self.ent[c, i], self.err[c, i], lam, self.trace)
                total += float((self.err if on_error else self.ent)[c, i, q])
                self.indices[c, i] = q
        self.evaluations += 1
        self.last_sum = total
        return total

    def lambda_to_entropy(self, frame_lambda):
        return self._run(frame_lambda, False)

    def lambda_to_error(self, frame_lambda):
        return self._run(frame_lambda, True)


def _cmp(trace, a, b):
    if trace is not None:
        trace.append(("compare", a, b))


def entropy_to_lambda(ev, entropy):
    """schroquantiser.c:887-969.  Returns (lambda, not_bracketed, path): path names the branches taken."""
    t = ev.trace
    path = dict(direction=None, steps=0, broke=False, early=False, halvings=0)
    lambda_hi = 1.0
    entropy_hi = ev.lambda_to_entropy(lambda_hi)
    _cmp(t, entropy_hi, entropy)
    if entropy_hi < entropy:
        path["direction"] = "up"
        entropy_lo, lambda_lo = entropy_hi, lambda_hi
        for j in range(5):
            lambda_hi = lambda_lo * 100
            entropy_hi = ev.lambda_to_entropy(lambda_hi)
            path["steps"] += 1
            _cmp(t, entropy_hi, entropy)
            if entropy_hi > entropy:
                path["broke"] = True
                break
            entropy_lo, lambda_lo = entropy_hi, lambda_hi
    else:
        path["direction"] = "down"
        for j in range(5):
            lambda_lo = lambda_hi * 0.01
            entropy_lo = ev.lambda_to_entropy(lambda_lo)
            path["steps"] += 1
            _cmp(t, entropy_lo, entropy)
            if entropy_lo < entropy:
                path["broke"] = True
                break
            entropy_hi, lambda_hi = entropy_lo, lambda_lo
    if entropy_lo == entropy_hi:
        path["early"] = True
        return math.sqrt(lambda_lo * lambda_hi), 0, path
    not_bracketed = 1 if (entropy_lo > entropy or entropy_hi < entropy) else 0
    _cmp(t, entropy_lo, entropy)
    _cmp(t, entropy_hi, entropy)
    for j in range(7):
        if entropy_hi == entropy_lo:
            break
        lambda_mid = math.sqrt(lambda_lo * lambda_hi)
        entropy_mid = ev.lambda_to_entropy(lambda_mid)
        path["halvings"] += 1
        _cmp(t, entropy_mid, entropy)
        if entropy_mid > entropy:
            lambda_hi, entropy_hi = lambda_mid, entropy_mid
        else:
            lambda_lo, entropy_lo = lambda_mid, entropy_mid
    return math.sqrt(lambda_hi * lambda_lo), not_bracketed, path


def error_to_lambda(ev, error):
    """schroquantiser.c:1016-1098"""
    t = ev.trace
    path = dict(direction=None, steps=0, broke=False, early=False, halvings=0)
    lambda_lo = 1.0
    error_lo = ev.lambda_to_error(lambda_lo)
    _cmp(t, error, error_lo)
    if error < error_lo:
        path["direction"] = "up"
        error_hi, lambda_hi = error_lo, lambda_lo
        for j in range(5):
            lambda_lo = lambda_hi * 100
            error_lo = ev.lambda_to_error(lambda_lo)
            path["steps"] += 1
            _cmp(t, error, error_lo)
            if error > error_lo:
                path["broke"] = True
                break
            error_hi, lambda_hi = error_lo, lambda_lo
    else:
        path["direction"] = "down"
        for j in range(5):
            lambda_hi = lambda_lo * 0.01
            error_hi = ev.lambda_to_error(lambda_hi)
            path["steps"] += 1
            _cmp(t, error, error_hi)
            if error < error_hi:
                path["broke"] = True
                break
            error_lo, lambda_lo = error_hi, lambda_hi
    if error_lo == error_hi:
        path["early"] = True
        return math.sqrt(lambda_lo * lambda_hi), 0, path
    not_bracketed = 1 if (error_lo > error or error_hi < error) else 0
    _cmp(t, error_lo, error)
    _cmp(t, error_hi, error)
    for j in range(14):
        if error_hi == error_lo:
            break
        lambda_mid = math.sqrt(lambda_lo * lambda_hi)
        error_mid = ev.lambda_to_error(lambda_mid)
        path["halvings"] += 1
        _cmp(t, error_mid, error)
        if error_mid > error:
            lambda_hi, error_hi = lambda_mid, error_mid
        else:
            lambda_lo, error_lo = lambda_mid, error_mid
    return math.sqrt(lambda_hi * lambda_lo), not_bracketed, path


def choose(ent, err, depth, weight, scales, engine, target, trace=None):
    """One picture through one engine.  Returns a dict: quant_index [3][nb] (what the engine LEAVES), frame_lambda, sum
    (what the last evaluation made returned), chosen_entropy / chosen_error [3][nb] (the estimates at quant_index),
    evaluations, not_bracketed, path."""
    ev = Evaluator(ent, err, depth, weight, scales, trace)
    path, nbr = None, 0
    if engine == ENGINE_LAMBDA:                 # rdo_lambda, rdo_cbr: :758-782
        lam = float(target)
        ev.lambda_to_entropy(lam)
    elif engine == ENGINE_BIT_ALLOCATION:       # :738-756
        lam, nbr, path = entropy_to_lambda(ev, float(target))
        ev.lambda_to_entropy(lam)
    elif engine == ENGINE_CONSTANT_ERROR:       # :1100-1119
        lam, nbr, path = error_to_lambda(ev, float(target))
    else:
        raise ValueError("engine %r" % (engine,))
    q = ev.indices.copy()
    nb = n_bands(depth)
    ce = np.array([[ent[c, i, q[c, i]] for i in range(nb)] for c in range(3)], np.float64)
    cr = np.array([[err[c, i, q[c, i]] for i in range(nb)] for c in range(3)], np.float64)
    return dict(quant_index=q, frame_lambda=lam, sum=ev.last_sum, chosen_entropy=ce, chosen_error=cr,
                evaluations=ev.evaluations, not_bracketed=nbr, path=path)


def estimated_residual_bits(chosen_entropy):
    """schro_encoder_estimate_entropy, schroquantiser.c:785-798: `int n; n += double` -- every addition truncates"""
    n = 0
    for c in range(3):
        for v in chosen_entropy[c]:
            n = int(n + float(v))
    return n
