"""CPU: what holds the checker of the low-delay slice encoder (tests/lowdelay_enc_ref.py).

  * its vectorised quantiser and code lengths against the scalar restatements (quant_ref.schro_quantise,
    schro_pack_estimate_sint, schro_pack_encode_sint) on every index and every s16 value, the int16 wrap included;
  * its bytes against INDEPENDENT code: oracle_lib.lowdelay_decode follows the reference's decoders, and what it decodes
    from the checker's bytes is the checker's own reconstruction -- on the input classes where a decoder can return it
    (lowdelay_enc_cases.CASES names the others and why);
  * the chosen indices against the search's own rules."""
import numpy as np
import pytest

import lowdelay_enc_cases as K
import lowdelay_enc_ref as R
import oracle_lib as O
import quant_ref as Q

ALL = np.arange(-32768, 32768, dtype=np.int64)
ROUND_TRIP = [n for n, c in K.CASES.items() if c[3] is None] + ["large"]


@pytest.mark.parametrize("qi", [0, 1, 2, 3, 4, 5, 7, 8, 9, 17, 31, 32, 44, 59, 60])
def test_vector_quantiser_is_the_scalar_one_on_a_sample(qi):
    """every 97th value and both ends through the scalar code (the full sweep below compares closed forms)"""
    f, o = Q.quant_factor(qi), Q.quant_offset(qi, True)
    vals = np.concatenate([ALL[::97], [-32768, 32767, -1, 0, 1], np.arange(-65535, 65536, 1009)])
    got = R.quantise_vec(vals, f, o)
    assert got.tolist() == [Q.schro_quantise(int(v), f, o) for v in vals]
    assert R.dequantise_vec(R.w16(got), f, o).tolist() == [Q.schro_dequantise(int(R.w16(int(q))), f, o) for q in got]


def test_vector_forms_on_every_index_and_value():
    """all 61 indices x all s16 values: the quantiser by its definition (truncating division of 4 |x| - offset + factor / 2,
    the dead zone), the bit length by bit_length () of Python ints, the wrap of stored values where it can happen"""
    factor, offset = R._tables()
    lengths = np.array([R.schro_pack_estimate_sint(int(v)) for v in range(0, 32769)])
    for qi in range(61):
        f, o = int(factor[qi]), int(offset[qi])
        q = R.quantise_vec(ALL, f, o)
        x = np.abs(ALL) * 4
        want = np.where(x < o, 0, np.sign(ALL) * ((x - o + f // 2) // f))
        assert np.array_equal(q, want)
        assert np.array_equal(R.w16(q), q)              # high-band values never wrap
        assert np.array_equal(R.estimate_sint_vec(q), lengths[np.abs(q)])
    # an LL difference reaches +-65535: at index 0 the stored value wraps, and the bits are those of the wrapped value
    d = np.arange(-65535, 65536, dtype=np.int64)
    q = R.w16(R.quantise_vec(d, 4, 1))
    assert q[0] == 1 and q[-1] == -1 and q.min() == -32768
    assert np.array_equal(R.estimate_sint_vec(q), lengths[np.abs(q)])


def test_codes_are_the_scalar_writer():
    vals = np.concatenate([np.arange(-300, 301), [-32768, 32767, 16383, -16384, 255, -256]])
    code, length = R.sint_codes(vals)
    assert length.tolist() == [R.schro_pack_estimate_sint(int(v)) for v in vals]
    want = [b for v in vals for b in R.schro_pack_encode_sint(int(v))]
    assert R.bits_of(code, length).tolist() == want


@pytest.mark.parametrize("name", ROUND_TRIP)
def test_decoder_returns_the_encoders_reconstruction(name):
    P, planes, res = K.expected(name)
    assert res["count"] == 0
    out = [np.zeros_like(p) for p in planes]
    O.lowdelay_decode(res["bytes"], out, P)
    for k in range(3):
        assert np.array_equal(out[k], res["recon"][k]), "component %d" % k


def test_round_trip_boundary():
    """Where a decoder cannot return the encoder's reconstruction: full-range values with a budget large enough for index
    0 (an LL difference wrapped when stored), slices that were cut, and -- on fast-decoder geometries -- slice sizes where
    8 n_bytes and 8 (n_bytes + 1) differ in bit length: the encoder sizes slice_y_length per slice (:800), the fast decoder from
    the short slice (:579)."""
    P = K.CASES["length_field"][0]             # 31 and 32 bytes: 8 x 31 has 8 bits, 8 x 32 has 9
    assert O.lowdelay_arith(P, 2) == O.LOWDELAY_FAST16 and set(R.slice_sizes(P)) == {31, 32}
    for name in ("full_range_big_budget", "overrun", "length_field"):
        P, planes, res = K.expected(name)
        out = [np.zeros_like(p) for p in planes]
        O.lowdelay_decode(res["bytes"], out, P)
        assert not all(np.array_equal(o, r) for o, r in zip(out, res["recon"]))


@pytest.mark.parametrize("name", list(K.CASES) + ["span", "large", "turns"])
def test_chosen_index_follows_the_search(name):
    P, planes, res = K.expected(name)
    for s, (slice_bytes, trace) in enumerate(zip(R.slice_sizes(P), res["traces"])):
        room, index = 8 * slice_bytes, int(res["index"][s])
        # the estimate of the final probe, trailing zeros and all, is the number of bits the writer then wrote
        assert res["used"][s] == trace[-1][1]
        if trace[0][1] <= room:
            assert index == 0 and len(trace) == 1
            continue
        assert len(trace) == 8 and 1 <= index <= 64 and trace[-1][0] == index
        accepted = [b for b, n in trace[1:7] if n >= room]
        assert index == sum(b - a for a, b in zip([0] + accepted, accepted)) + 1 == (accepted[-1] if accepted else 0) + 1
        assert bool(res["overrun"][s]) == (trace[-1][1] > room)


def test_which_cases_leave_lds():
    """lowdelay_enc_cases.leaves_lds restates the serial launch's choice between LDS and the queue's scratch: the spill
    cases are beyond it (with unlike indices, unequal rectangles and no over-run: they join the round trip), the cases
    meant for LDS are not -- neither can change sides unnoticed"""
    for name in ("spill_2x2", "spill_3x5_420", K.SPILL_BATCH[0], "one_slice", "one_slice_444_d1"):
        assert K.leaves_lds(K.CASES[name][0]), name
    for name in ["turns", "large"] + [n for n in K.CASES if n.startswith("64x32_")]:
        assert not K.leaves_lds(K.expected(name)[0]), name
    assert K.per_thread_samples(K.CASES["spill_2x2"][0]) == 3 * (32 * 32 + 33 + 32) + 32
    assert K.per_thread_samples(K.expected("turns")[0]) == 200          # (turns_case's own count)
    for name in ("spill_2x2", "spill_3x5_420"):
        P, _, res = K.expected(name)
        assert len(set(res["index"].tolist())) > 1 and res["count"] == 0 and name in ROUND_TRIP
    P = K.CASES["spill_2x2"][0]
    assert min(P["n_horiz_slices"], P["n_vert_slices"]) == 2           # a diagonal of two threads
    P = K.CASES["spill_3x5_420"][0]
    assert P["iwt_chroma_width"] < P["iwt_luma_width"] and P["iwt_chroma_height"] < P["iwt_luma_height"]
    for size, n in ((P["iwt_luma_width"] >> 2, 3), (P["iwt_luma_height"] >> 2, 5), (P["iwt_chroma_width"] >> 2, 3), (P["iwt_chroma_height"] >> 2, 5)):
        assert len(set(R.codeblock(size, 1, k, 0, n, 1)[1] - R.codeblock(size, 1, k, 0, n, 1)[0] for k in range(n))) >= 2


def test_span_and_exact_fits():
    _, _, res = K.expected("span")
    assert res["index"].min() == 0 and res["index"].max() == 64 and len(set(res["index"].tolist())) >= 40
    P, _, res = K.exact_fit(0)
    assert res["traces"][0] == [(0, 8 * P["slice_bytes_num"])] and res["index"][0] == 0       # <=: stays
    P, _, res = K.exact_fit(32)
    assert res["traces"][0][1] == (32, 8 * P["slice_bytes_num"]) and res["index"][0] >= 33    # >=: moves up
    _, _, res = K.expected("below_zero")
    assert res["index"].min() < 50          # base - quant_matrix[i] is below 0 for several sub-bands
    _, _, res = K.expected("zero")
    assert not res["index"].any() and (res["bytes"].reshape(16, 16)[:, 2:] == 255).all()
    _, _, res = K.expected("overrun")
    assert res["count"] == 16
