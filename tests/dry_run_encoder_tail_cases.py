"""The draws of the encoder tail's random-geometry tests (tests/encoder_tail_draws.py) walked on the CPU, without a device,
at SCHRO_FUZZ_SCALE 1 and SCHRO_FUZZ_SEED 0: each function runs the Python checkers over the draws of one GPU test, asserts
that the draws are what that test's docstring promises and returns the seconds spent in the checkers, which
tests/test_encoder_tail_draws.py prints.  The draw counts are sized so that no test spends more than about 15 s there.

Measured on one CPU core (MEASURED below, from `python tests/dry_run_encoder_tail_cases.py` with the repository and tests/
on the path): the slice encoder's 40 draws, 75 pictures of 3123 slices in all, 8.2 s; the quantiser's 40 draws, 149 planes,
1.2 s; the histograms' 60 draws, 243 planes, 0.4 s; the chain's 12 draws, 1.0 s.

Not collected by a plain `pytest tests/` (the name); tests/test_encoder_tail_draws.py runs it."""
import time

import numpy as np

import encoder_tail_draws as D
import hist_cases as HC
import lowdelay_enc_cases as K
import lowdelay_enc_ref as R
import oracle_lib as O
import quant_cases as QC

# seconds in the checkers per GPU test, as measured when the draw counts were set
MEASURED = {"test_lowdelay_encode_random_pictures": 8.2, "test_quantise_random_codeblocks": 1.2,
            "test_histogram_random_bands": 0.4, "test_chain_on_the_plane_layer": 1.0}


def walk_lowdelay():
    """B: both sides of the LDS / spill predicate; chosen indices from 0 to at least 60; empty LL rectangles; over-runs; every
    chroma format, depth, picture kind, matrix kind and denominator; fractional slice sizes"""
    spent = 0.0
    sides, indices, formats, depths, kinds, matrices, denoms = set(), set(), set(), set(), set(), set(), set()
    empty = overruns = pictures = slices = 0
    for draw in D.lowdelay_draws():
        P = draw["P"]
        assert not D.refused_for_chroma_ll(P), draw["tag"]
        nslices = P["n_horiz_slices"] * P["n_vert_slices"]
        assert 1 <= nslices <= D.MAX_SLICES and P["slice_bytes_num"] >= P["slice_bytes_denom"], draw["tag"]
        assert P["slice_bytes_denom"] == 1 or P["slice_bytes_num"] % P["slice_bytes_denom"], draw["tag"]
        assert all(p % 2 == 0 and 0 <= p <= 64 for p in draw["pads"]) and 0 <= draw["skew"] <= 3
        assert K.leaves_lds(P) or draw["tag"][1] % 8 != 7, draw["tag"]
        sides.add((K.leaves_lds(P), nslices > 1))
        formats.add(draw["fmt"])
        depths.add(P["transform_depth"])
        denoms.add(P["slice_bytes_denom"])
        matrices.add(draw["tag"][10])
        empty += D.empty_ll_rectangles(P)
        for (kind, _), planes in zip(draw["kinds"], D.lowdelay_pictures(draw)):
            t = time.perf_counter()
            res = R.encode(planes, P)
            spent += time.perf_counter() - t
            indices.update(res["index"].tolist())
            overruns += res["count"] > 0
            kinds.add(kind)
            pictures += 1
            slices += nslices
    assert {(False, True), (True, True)} <= sides, sides          # off LDS with more than one slice, too
    assert min(indices) == 0 and max(indices) >= 60 and len(indices) >= 50, sorted(indices)
    assert empty >= 1 and overruns >= 1, (empty, overruns)
    assert formats == set(D.FORMATS) and depths == {1, 2, 3, 4} and kinds == set(D.KINDS), (formats, depths, kinds)
    assert matrices == {"default", "WIDE", "DEEP", "random"} and denoms == set(range(1, 8)), (matrices, denoms)
    return spent, dict(pictures=pictures, slices=slices, empty_ll_draws=empty, overrun_pictures=overruns, indices=len(indices))


def walk_quantise():
    """C, the quantiser: every index 0 .. 60 in intra and in inter planes; both sample types; depths 1 .. 4; odd pitches; DC
    bands whose shorter side is 1, and larger ones"""
    spent = 0.0
    seen = {0: set(), 1: set()}
    types, depths, thin, wide, planes = set(), set(), 0, 0, 0
    for draw in D.quantise_draws():
        assert 1 <= len(draw["specs"]) <= 6, draw["tag"]
        for spec, shape in zip(draw["specs"], draw["tag"][3]):
            assert spec["buf"].shape[1] % 2 == 1, draw["tag"]
            seen[spec["intra"]].update(r[4] for r in spec["records"])
            types.add(spec["buf"].dtype.name)
            depths.add(shape[3])
            if spec["intra"]:
                thin += min(spec["dc"][1:]) == 1
                wide += min(spec["dc"][1:]) > 4
            t = time.perf_counter()
            QC.expected(spec)
            spent += time.perf_counter() - t
            planes += 1
    assert seen[0] == seen[1] == set(range(61)), (sorted(set(range(61)) - seen[0]), sorted(set(range(61)) - seen[1]))
    assert types == {"int16", "int32"} and depths == {1, 2, 3, 4} and thin >= 2 and wide >= 2, (types, depths, thin, wide)
    return spent, dict(planes=planes, thin_dc_bands=thin)


def walk_histogram():
    """C, the histograms: both sample types; both forms of sub-band 0; bands 1 wide and 1 high; skips 1, 2 and 4; planes of
    equal samples that land in a register bin, in an LDS bin and in the overflow count"""
    spent = 0.0
    types, forms, skips, bins = set(), set(), set(), set()
    one_wide = one_high = planes = 0
    for draw in D.histogram_draws():
        assert 1 <= len(draw["specs"]) <= 8, draw["tag"]
        for spec in draw["specs"]:
            assert spec["buf"].shape[1] % 2 == 1, draw["tag"]
            types.add(spec["buf"].dtype.name)
            forms.add(spec["bands"][0][5])
            skips.update(bd[4] for bd in spec["bands"])
            one_wide += any(bd[2] == 1 for bd in spec["bands"])
            one_high += any(bd[3] == 1 for bd in spec["bands"])
            t = time.perf_counter()
            want = HC.expected(spec)
            spent += time.perf_counter() - t
            planes += 1
            if draw["equal"]:
                for bd, row in zip(spec["bands"], want):
                    if not bd[5]:
                        assert np.count_nonzero(row) == 1, draw["tag"]       # one bin takes every sample
                        bins.add(int(np.flatnonzero(row)[0]))
    assert types == {"int16", "int32"} and forms == {0, 1} and {1, 2, 4} <= skips, (types, forms, skips)
    assert one_wide >= 1 and one_high >= 1, (one_wide, one_high)
    assert bins & {0, 1, 2, 3} and bins & set(range(4, 104)) and 104 in bins, sorted(bins)
    return spent, dict(planes=planes, equal_bins=sorted(bins))


def walk_chain(pixel_range):
    """D: every filter, depth 1 .. 3 and chroma format; both sides of the LDS / spill predicate; and the cap -- at most one
    draw in five leaves the decode half out (length_field class or over-run slices).  Where the decode half stays, the
    oracle's decoder returns the checker's reconstruction: the expected pictures are what the encoder meant."""
    spent = 0.0
    filters, depths, formats, sides = set(), set(), set(), set()
    draws = skipped = 0
    for draw in D.chain_draws():
        pictures = D.chain_pictures(draw, pixel_range)
        t = time.perf_counter()
        coeffs, res, planes, back = D.chain_expected(draw, pictures)
        spent += time.perf_counter() - t
        draws += 1
        filters.add(draw["filt"])
        depths.add(draw["depth"])
        formats.add(draw["fmt"])
        sides.add(K.leaves_lds(draw["P"]))
        if planes is None:
            skipped += 1
            continue
        for k in range(3):
            assert np.array_equal(planes[k], res["recon"][k]), draw["tag"] + ("component", k)
            assert back[k].shape == pictures[k].shape
    assert filters == set(D.FILTERS) and depths == {1, 2, 3} and formats == set(D.FORMATS), (filters, depths, formats)
    assert sides == {False, True}
    assert skipped * D.CHAIN_SKIP_CAP <= draws, (skipped, draws)
    return spent, dict(draws=draws, without_decode=skipped)


def main():
    from test_gpu_iwt_forward import pixel_range
    for name, walk in (("test_lowdelay_encode_random_pictures", walk_lowdelay), ("test_quantise_random_codeblocks", walk_quantise),
                       ("test_histogram_random_bands", walk_histogram),
                       ("test_chain_on_the_plane_layer", lambda: walk_chain(pixel_range))):
        spent, facts = walk()
        print("%-40s %6.2f s in the checkers  %s" % (name, spent, facts))


if __name__ == "__main__":
    main()
