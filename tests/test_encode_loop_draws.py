"""CPU: the draws of tests/encode_loop_draws.py are what tests/test_gpu_encode_loop.py says they are -- every draw of
scale 1 walked, nothing skipped or filtered.  Range: every forward coefficient lies within +-4095, where DESIGN 4.9's
round trip holds (the decoder's dequantisation equals the encoder's reconstruction for every index and form).
Agreement: on the checkers alone the encoder-side u8 reconstruction equals the decoder-side one for every picture, so a
mismatch on the device is the device's.  Coverage summed over the draws, and drift: picture 2 predicted from the ORIGINAL
pictures differs from picture 2 predicted from their reconstructions."""
import os

import numpy as np
import pytest

import encode_loop_draws as E

# (a campaign of tests/test_gpu_encode_loop.py walks its own draws here first, with the same two variables)
SCALE = int(os.environ.get("SCHRO_FUZZ_SCALE", "1"))
SEED = int(os.environ.get("SCHRO_FUZZ_SEED", "0"))
NAMES = E.names(SCALE, SEED)


@pytest.fixture(scope="module")
def groups():
    return {name: E.expected(name) for name in NAMES}


def test_there_are_eight_named_and_eight_seeded_draws():
    assert len(E.NAMED) == 8 and len(NAMES) == 8 + 8 * SCALE == len(set(NAMES))
    assert all(n in E.NAMED for n in E.COMBINE_FORM + (E.FRAME_LAYER,))
    pad = [any(E.padded(E.get(n))) for n in E.COMBINE_FORM]
    assert len(E.COMBINE_FORM) == 2 and any(pad) and not all(pad)
    d = E.get(E.FRAME_LAYER)
    (lh, lw), (ch, cw) = E.iwt_dims(d)[:2]
    assert d["fmt"] == 420 and (lh, lw) == (2 * ch, 2 * cw)       # a frame's chroma components are its luma's halved


def test_range(groups):
    for name, group in groups.items():
        for n, (comps, _) in enumerate(group):
            for k, c in enumerate(comps):
                top = int(np.abs(c["coeffs"].astype(np.int32)).max())
                assert top <= 4095, (name, "picture", n, "component", k, top)


def test_agreement_on_the_cpu(groups):
    for name, group in groups.items():
        for n, (comps, _) in enumerate(group):
            for k, c in enumerate(comps):
                assert np.array_equal(c["enc_u8"], c["dec_u8"]), (name, "picture", n, "component", k, int((c["enc_u8"] != c["dec_u8"]).sum()))
                assert np.array_equal(c["recon"], c["dec_coeffs"]), (name, "picture", n, "component", k, "reconstructed coefficients")


def test_coverage(groups):
    draws = [E.get(n) for n in NAMES]
    assert {d["filt"] for d in draws} == set(range(7))
    assert {d["depth"] for d in draws} == {1, 2, 3}
    assert {d["fmt"] for d in draws} == {420, 422, 444}
    assert {d["prec"] for d in draws} == {0, 1, 2, 3}
    u = [1 << d["depth"] for d in draws]
    assert any(d["w"] % m and d["h"] % m for d, m in zip(draws, u)), "no size with padding in both directions"
    assert any(not any(E.padded(d)) for d in draws), "no size without padding"
    forms = set()
    for d in draws:
        for q in d["qi"]:
            for i in q[1:]:
                forms.add("0" if i == 0 else "3" if i == 3 else "x4" if i % 4 == 0 else "<=8" if i <= 8 else ">8")
    assert forms == {"0", "3", "x4", "<=8", ">8"}, forms
    zero = nonzero = 0
    saturating = []
    for name, group in groups.items():
        both = []
        for n, (comps, _) in enumerate(group):
            for k, c in enumerate(comps):
                zero += int((c["summaries"][:, 0] == 0).sum())
                nonzero += int((c["summaries"][:, 0] != 0).sum())
                h, w = E.dims(E.get(name))[k]
                # (the encoder's sum; the decoder's conversion saturates at the same samples: its u8 picture equals this one's,
                # test_agreement_on_the_cpu)
                s = c["enc_sum"][:h, :w]
                both.append(bool((s < -128).any() and (s > 127).any()))
            if n:
                assert any(c["quant"].any() for c in comps), (name, "picture", n, "the residual quantises to nothing")
        if any(both):
            saturating.append(name)
    assert zero > 0 and nonzero > 0, (zero, nonzero)
    assert saturating, "no draw whose sum leaves 0 .. 255 on both sides"


def test_the_search_draw_hands_over_a_valid_single_reference_field(groups):
    d = E.get("vectors_from_the_search")
    assert (d["prec"], d["blk"]) == (0, (8, 8))
    mv = groups["vectors_from_the_search"][1][1]
    P = E.motion_params(d)
    nbx, nby = P["x_num_blocks"], P["y_num_blocks"]
    assert mv.size == nbx * nby
    assert (mv["flags"] == 1).all()                 # prediction mode 1, no global motion, split 0: all of it a legal record
    assert not mv["v"][:, 1].any() and not mv["v"][:, 3].any()
    off = np.ones((nby, nbx), bool)
    off[::2, ::2] = False
    assert not mv["v"].reshape(nby, nbx, 4)[off].any() and not mv["metric"].reshape(nby, nbx)[off].any()
    assert mv["v"].reshape(nby, nbx, 4)[~off].any(), "the search found no motion at all"


DRIFT_DRAW = "dd97_420_depth3_padded"


def test_drift_is_real(groups):
    comps, _ = E.code_group(DRIFT_DRAW, refs_of=lambda pics, recons, n: pics[:n])[2]
    want = groups[DRIFT_DRAW][2][0]
    assert any(not np.array_equal(a["enc_u8"], b["enc_u8"]) for a, b in zip(comps, want)), \
        "picture 2 does not depend on which reference planes it reads"
