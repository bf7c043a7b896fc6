"""CPU: the walk of tests/encoder_pipeline_cases.py -- the order of the scratch needs that makes a sequence grow and then
reuse the block, the witness that no two calls which may meet in one table buffer expect the same outputs, and the witness
that the inter chain is a chain in the data."""
import numpy as np
import pytest

import encoder_pipeline_cases as P


@pytest.mark.parametrize("stage", P.SCRATCH_STAGES)
def test_scratch_needs_are_small_large_smaller(stage):
    (a, fa), (b, fb), (c, fc) = P.needs(stage)
    assert fa >= a and fb >= b and fc >= c
    if not (a or b or c):                               # the plane-layer call takes no scratch: the frame-layer runs do
        a, b, c = fa, fb, fc
    assert a > 0 and b >= 4 * a, (a, b)                 # B reallocates the block behind A's launches
    assert c < b and c != a, (a, b, c)                  # C's tables lie on B's leftovers, and are not A's again
    # the frame-layer run of A sizes the block itself, for less than B's own run would
    assert fa < fb, (fa, fb)
    assert len(set(P.stage(stage)["sequence"])) == 3


def test_the_new_stages_are_in_both_lists():
    for stage in ("noarith_dec", "motion_enc"):
        assert stage in P.SCRATCH_STAGES and stage in P.NINE_CALL_STAGES and stage in P.STAGES


def test_decoder_scratch_by_hand_is_the_librarys():
    """The by-hand formula of the decoder's scratch against schro_hip_noarith_decode_scratch_words, for A, B and C and for
    the three in one call; B is the picture of 1027 chunks."""
    import schroedinger_amd as sa
    from schroedinger_amd import _lib
    from test_noarith_decode_api import fake_picture
    lib = _lib.load()
    s = P.stage("noarith_dec")
    cases = [s["cases"][n] for n in s["sequence"]]
    for case in cases:
        assert case.dtype.itemsize == 2
        assert 4 * lib.schro_hip_noarith_decode_scratch_words(sa.noarith_decode_pictures([fake_picture(case)]), 1, 2) == s["batch_need"](case), case.name
    arr = sa.noarith_decode_pictures([fake_picture(c, n) for n, c in enumerate(cases)])
    assert 4 * lib.schro_hip_noarith_decode_scratch_words(arr, 3, 2) == sum(s["batch_need"](c) for c in cases)
    a, b, c = cases
    assert a.sizes[0] == (16, 8) and c.sizes[0] == (32, 16) and c.depth == 3
    assert -(-int(b.expected()[2]["subband_length"][0, 1]) // 8) == 1027
    # A goes through the frame layer as an inter picture of a 4:2:0 frame
    assert a.is_intra == 0 and a.sizes[1] == (8, 4) and all(x.expected()[2]["error"] == 0 for x in cases)
    words = P.noarith_dec_result_words(a.expected()[2])
    assert words.size * 4 == __import__("ctypes").sizeof(_lib.NoarithDecodeResult)
    back = sa.noarith_decode_result(words)
    assert all(np.array_equal(np.asarray(back[k]), np.asarray(v)) for k, v in a.expected()[2].items())


def test_motion_encoder_scratch_constants_are_the_headers():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "schroedinger_amd", "csrc", "schro_hip_internal.h")).read()
    assert "kMeSbWords = %d" % P.ME_SB_WORDS in text and "kMeSections = SCHRO_HIP_MOTION_SECTIONS" in text
    from schroedinger_amd import _lib
    assert _lib.MOTION_SECTIONS == P.ME_SECTIONS
    a, b, c = (P.case("motion_enc", n) for n in P.stage("motion_enc")["sequence"])
    assert (a[2], a[3]) == (4, 4) and (b[2], b[3]) == (132, 68) and (c[2], c[3]) == (12, 12)


@pytest.mark.parametrize("both_queues", [False, True])
@pytest.mark.parametrize("stage", P.SCRATCH_STAGES)
def test_scratch_sequence_order(stage, both_queues):
    seq = P.scratch_sequence(stage, both_queues)
    a, b, c = P.stage(stage)["sequence"]
    for q in ((0, 1) if both_queues else (1,)):
        mine = [(name, layer) for qq, name, layer in seq if qq == q]
        assert mine == [(a, "plane"), (b, "plane"), (c, "plane"), (a, P.FRAME), (b, "plane")]


@pytest.mark.parametrize("stage", P.NINE_CALL_STAGES)
def test_nine_calls_carry_unlike_tables(stage):
    """More calls than two turns of a queue's table buffers, and whichever two cases follow one another in the cycle --
    so also call k and the call that takes its buffer, four or two calls later -- expect different outputs: a launch
    that read another call's table cannot leave its own."""
    assert P.NINE > 2 * P.BIG_TABLES
    seq = P.stage(stage)["sequence"]
    for one, queues in ((False, (0,)), (True, (0, 1))):
        calls = P.nine_calls(stage, one)
        assert len(calls) == P.NINE and {q for q, _ in calls} == set(queues)
        for q in queues:
            mine = [name for qq, name in calls if qq == q]
            assert len(mine) >= P.BIG_TABLES
            for d in (1, 2, 4):                         # (a stage sends one, two or four tables per call)
                assert all(mine[k] != mine[k + d] for k in range(len(mine) - d)), (q, d, mine)
    for k in range(3):
        x, y = P.outputs(stage, seq[k]), P.outputs(stage, seq[(k + 1) % 3])
        assert x.keys() == y.keys()
        for key in x:
            assert not P.same_bytes(x[key], y[key]), (stage, seq[k], seq[(k + 1) % 3], key)
            # (not by their sizes alone: the common prefix differs too)
            n = min(x[key].nbytes, y[key].nbytes)
            assert x[key].tobytes()[:n] != y[key].tobytes()[:n], (stage, key)


# ---- the inter chain ----------------------------------------------------------------------------------------------------

def test_chain_pictures_are_unlike():
    a, b = (P.chain_geometry(n) for n in P.CHAIN_PAIR)
    for key in ("fmt", "xbsep", "prec", "dims", "hc", "mode"):
        assert a[key] != b[key], key
    assert P.records(a) != P.records(b)
    # three deep: the middle picture has the larger grid -- both queues' scratch grows mid-pipeline --, the third a smaller one
    grids = [P.records(P.chain_geometry(n)) for n in P.CHAIN_PIPELINE]
    assert grids[1] > grids[0] and grids[2] < grids[1]
    assert len(set(P.CHAIN_PIPELINE)) == 3 and P.flatten(P.chain_inputs(P.CHAIN_PIPELINE[0])) != P.flatten(P.chain_inputs(P.CHAIN_PIPELINE[2]))
    for name in P.CHAIN_PICTURES:
        g = P.chain_geometry(name)
        assert g["ext"] == max(g["blocks"]["xbsep_luma"], g["blocks"]["ybsep_luma"])       # the smallest the stages take


@pytest.mark.parametrize("name", sorted(P.CHAIN_PICTURES))
def test_chain_is_a_chain_in_the_data(name):
    """Every stage's expected output changes when its predecessor's output is replaced by the fill pattern or the field-set
    record: a stage on the device that read something else than what the stage before it left cannot pass."""
    deps = P.chain_dependencies(name)
    assert [d[:2] for d in deps] == [("pyramid", "hbm"), ("hbm level 0", "subpel"), ("hbm level 1", "mode table"), ("hbm level 2", "mode table"),
                                          ("subpel", "mode"), ("mode", "prediction"), ("prediction", "residual"), ("residual", "coefficients"),
                                          ("coefficients", "quantise"), ("quantise", "bytes")]
    for producer, consumer, want, got in deps:
        assert P.flatten(want) != P.flatten(got), (name, producer, consumer)
    e = P.chain_expected(name)
    # something of every kind is there to be compared: vectors that moved, both references used, values that survive the quantiser
    assert any(e["subpel"][r]["v"].any() for r in (0, 1)) and len(set((e["mode"][0]["flags"] & 3).tolist())) > 1
    assert all(q.any() for q, _, _ in e["quantise"]) and len(e["bytes"][0]) > 3 * (1 + 3 * P.CHAIN_DEPTH)


@pytest.mark.parametrize("name", sorted(P.CHAIN_PICTURES))
def test_chain_bytes_decode_to_the_reconstruction(name):
    e = P.chain_expected(name)
    quant, recon, used = P.chain_decoded(e["geometry"], e["bytes"][0])
    assert used == len(e["bytes"][0])
    for k in range(3):
        assert np.array_equal(quant[k], e["quantise"][k][0]) and np.array_equal(recon[k], e["quantise"][k][1]), k
