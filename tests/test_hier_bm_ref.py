"""CPU: tests/hier_bm_ref.py, the restatement of schro_hierarchical_bm_scan_hint / schro_hbm_scan, against what the C text
implies -- the order of the blocks does not matter beyond left / above / above-left, each named case of
tests/hier_bm_cases.py meets what it is named for, blocks off the grid or off the plane keep the field-set record."""
import numpy as np
import pytest

import hier_bm_cases as K
import hier_bm_ref as R
import oracle_lib as O


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_raster_and_diagonal_order_give_the_same_field(name):
    c = K.CASES[name]
    field, stats = K.expected(name)
    again, stats2 = K.reference(c, *K.inputs(name), order="diagonal")
    assert again.tobytes() == field.tobytes()
    assert stats2 == stats


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_named_cases_meet_what_they_are_named_for(name):
    c = K.CASES[name]
    field, stats = K.expected(name)            # (asserts stats[key] > 0 for every key the case wants)
    assert stats["blocks"] > 0 and stats["cand"] >= stats["blocks"]
    if name.startswith("padded_grid"):
        assert stats["skipped"] > 0 and c["nbx"] % 4 == 0 and c["nby"] % 4 == 0
        assert c["w"] % c["xb"] and c["h"] % c["yb"]            # partial right and bottom blocks
    if name == "tall_4x4":
        assert K.max_diagonal(c["nbx"], c["nby"], c["shift"]) > K.ROUGH_WAVES
    if name == "flat_ties":
        assert stats["order_ties"] > 0 and not field["metric"][field["metric"] != 0].size
    if name == "still":
        assert stats["all_duplicates"] == stats["blocks"] and not field["v"].any() and not field["metric"].any()
    if name == "moved_far":
        assert 2 * c["h_range"] + 1 > c["w"] and stats["clamped"] > 0
        assert (K.inputs(name)[2]["v"] < 0).any()
    if c["hint"] is None:
        assert K.inputs(name)[2] is None


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_records_off_the_grid_or_off_the_plane_keep_the_field_set_record(name):
    c = K.CASES[name]
    field, _ = K.expected(name)
    skip, nbx = 1 << c["shift"], c["nbx"]
    split = R.split_of(c["shift"])
    blank = R.field_set(1, split, c["ref_index"] + 1)[0]
    assert int(blank["flags"]) == (c["ref_index"] + 1) | (split << 3)
    visited = 0
    for j in range(c["nby"]):
        for i in range(nbx):
            on_grid = i % skip == 0 and j % skip == 0
            on_plane = (i * c["xb"]) >> c["shift"] < c["w"] and (j * c["yb"]) >> c["shift"] < c["h"]
            rec = field[j * nbx + i]
            if on_grid and on_plane:
                visited += 1
                assert rec["flags"] == blank["flags"] and rec["chroma_metric"] == 0
                assert rec["v"][1 - c["ref_index"]] == 0 and rec["v"][3 - c["ref_index"]] == 0
                assert rec["v"][c["ref_index"]] % skip == 0 and rec["v"][2 + c["ref_index"]] % skip == 0
            else:
                assert rec.tobytes() == blank.tobytes(), (i, j)
    assert visited == K.expected(name)[1]["blocks"]


def test_split_follows_the_level():
    assert [R.split_of(s) for s in (0, 1, 2, 3, 8)] == [2, 1, 0, 0, 0]


def test_duplicates_keep_the_last_occurrence():
    a, b, z = (4, 4), (-6, 4), (0, 0)
    assert R.remove_duplicates([z, a, z, z, b, b]) == [a, z, b]
    assert R.first_occurrences([z, a, z, z, b, b]) == [z, a, b]
    assert R.remove_duplicates([z]) == [z] and R.remove_duplicates([z, z, z]) == [z]
    assert R.remove_duplicates([a, b, z]) == [a, b, z]


def test_the_metric_runs_over_the_three_components_clipped_to_the_frame():
    rng = np.random.default_rng(5)
    frame = (rng.integers(0, 256, (11, 13), dtype=np.uint8), rng.integers(0, 256, (6, 7), dtype=np.uint8), rng.integers(0, 256, (6, 7), dtype=np.uint8))
    ref = tuple(np.zeros_like(p) for p in frame)
    # the block at (8, 8) of a 13 x 11 picture: 5 x 3 of luma, 3 x 2 of each chroma plane (the rounded-up planes)
    want = int(frame[0][8:, 8:].sum()) + int(frame[1][4:, 4:].sum()) + int(frame[2][4:, 4:].sum())
    assert R.block_sad(frame, ref, 8, 8, 0, 0, 8, 8, 1, 1, 8) == want
    # literal validity checks: outside the apron the metric is INT_MAX
    assert R.block_sad(frame, ref, 8, 8, 0, 0, 8, 8, 1, 1, 2) == R.INT_MAX
    assert R.block_sad(frame, ref, 0, 0, -9, 0, 8, 8, 1, 1, 8) == R.INT_MAX
    # the reference block reads the apron: clamped coordinates, negative chroma coordinates through >>
    ref2 = tuple(np.full_like(p, 9) for p in frame)
    m = R.block_sad(frame, ref2, 0, 0, -3, -8, 8, 8, 1, 1, 8)
    assert m == sum(int(np.abs(p[:hh, :ww].astype(int) - 9).sum()) for p, (ww, hh) in zip(frame, ((8, 8), (4, 4), (4, 4))))


def test_chain_ranges_are_those_of_schro_hbm_scan():
    assert R.chain_ranges(1) == {1: 20, 0: 3}
    assert R.chain_ranges(5) == {5: 20, 4: 10, 3: 5, 2: 3, 1: 3, 0: 3}


@pytest.mark.parametrize("size", K.CHAIN_SIZES)
def test_chain_levels_do_not_depend_on_level_0_and_diagonal_order(size):
    w, h = size
    fields, stats = K.chain_reference(w, h, 3, 0)
    frame, ref = K.chain_pictures(w, h)
    without = R.hbm_scan(R.pyramid3(frame, 3), R.pyramid3(ref, 3), K.chain_params(w, h), 3, 0, 1, 1, K.CHAIN_EXT, with_level0=False,
                         order="diagonal")
    assert without[0] is None
    for k in (1, 2, 3):
        assert without[k].tobytes() == fields[k].tobytes()
        assert ((fields[k]["flags"] >> 3) & 3 == R.split_of(k)).all()
    assert ((fields[0]["flags"] >> 3) & 3 == 2).all()
    if w == 101:
        assert stats["skipped"] > 0
    # the search finds the motion of the pictures: most level-0 blocks off the border carry (5, -3) or a neighbour of it
    P = K.chain_params(w, h)
    f0 = fields[0].reshape(P["y_num_blocks"], P["x_num_blocks"])[2:-4, 2:-4]
    assert (np.abs(f0["v"][..., 0] - 5) <= 1).mean() > 0.8 and (np.abs(f0["v"][..., 2] + 3) <= 1).mean() > 0.8


@pytest.mark.parametrize("n", range(K.N_DRAWS))
def test_draws_have_a_reference(n):
    c, frame, ref, hint, field = K.draw(n)
    assert field.dtype == O.MV_DTYPE and field.size == c["nbx"] * c["nby"]
    assert frame[1].shape == K.chroma_size(c["w"], c["h"], c["fmt"])[::-1]
