"""GPU parity: OBMC calls whose planes are of unlike pictures.

schro_hip_obmc_batch (plane_obmc.cpp) does more per call than one launch per plane: it gives every plane a launch key
(precision, general-kernel variant, row form with its weights, prediction-only, s16 output) and sends each key's
planes out together; it merges the adjacent U and V planes of a picture into one job (pair images, full-pel planes,
and -- where the whole batch's chroma tiles make it pay -- the planes of half-pel images); it dedupes the weight tables
of a launch's block geometries and splits a launch whose tables overflow a slot; it caches tile orders under a hash
of the launch.  So which other planes share a call, and in what order, decides which kernel renders a plane.

The property under test: a plane's result does not depend on its batch-mates or on its position in the call.  Every
plane is checked against the oracle's render of that plane alone (np.array_equal)."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import schroedinger_amd as sa
import synth
from schroedinger_amd import _lib
from test_gpu_obmc import Ref, check_case, comp_size, make_case

pytestmark = pytest.mark.gpu

# Pictures that each land on a launch key or merge path of their own (make_case's arguments after ctx).  Sizes vary so
# that a launch's jobs differ in tile counts; the seed comes from the caller.
KINDS = {
    "fullpel_420": dict(w=96, h=64, xblen=12, xbsep=8, prec=0, weights=(1, 1, 1), chroma=(1, 1), mv_range=24),
    "halfpel_pair": dict(w=96, h=64, xblen=12, xbsep=8, prec=1, weights=(1, 1, 1), chroma=(1, 1), mv_range=48, pair=True),
    "qpel_fade_pair": dict(w=136, h=72, xblen=12, xbsep=8, prec=2, weights=(3, 5, 3), chroma=(1, 1), mv_range=96, pair=True),
    "eighth": dict(w=96, h=64, xblen=12, xbsep=8, prec=3, weights=(1, 1, 1), chroma=(1, 1), mv_range=192),
    "halfpel_plain": dict(w=96, h=64, xblen=12, xbsep=8, prec=1, weights=(1, 1, 1), chroma=(1, 1), mv_range=48),
    "blk32_16": dict(w=136, h=72, xblen=32, xbsep=16, prec=2, weights=(1, 1, 1), chroma=(1, 1), mv_range=80, pair=True),
    "blk20_12": dict(w=104, h=64, xblen=20, xbsep=12, prec=1, weights=(1, 1, 1), chroma=(1, 1), mv_range=40),
    "rect": dict(w=96, h=80, xblen=12, xbsep=8, yblen=16, ybsep=12, prec=2, weights=(1, 1, 1), chroma=(1, 1), mv_range=80,
                 pair=True),
    "gain": dict(w=96, h=64, xblen=12, xbsep=8, prec=2, weights=(2, 3, 1), chroma=(1, 1), mv_range=80, pair=True),
    "blk64": dict(w=136, h=72, xblen=64, xbsep=32, prec=1, weights=(1, 1, 1), chroma=(1, 1), mv_range=40),
    "pred_only": dict(w=96, h=64, xblen=12, xbsep=8, prec=2, weights=(1, 1, 1), chroma=(1, 1), mv_range=80, pair=True,
                      prediction_only=1),
    "pred_s16": dict(w=96, h=64, xblen=12, xbsep=8, prec=2, weights=(5, 3, 2), chroma=(1, 1), mv_range=80, prediction_only=2),
    "s32_residual": dict(w=96, h=64, xblen=12, xbsep=8, prec=2, weights=(1, 1, 1), chroma=(1, 1), mv_range=80, pair=True,
                         res_dtype=np.int32),
    "zero_residual": dict(w=96, h=64, xblen=12, xbsep=8, prec=1, weights=(1, 1, 1), chroma=(1, 1), mv_range=40, residual=False),
    "one_ref": dict(w=96, h=64, xblen=12, xbsep=8, prec=2, weights=(1, 1, 1), chroma=(1, 1), mv_range=80, pair=True, one_ref=True),
    "444": dict(w=96, h=64, xblen=12, xbsep=8, prec=2, weights=(1, 1, 1), chroma=(0, 0), mv_range=80),
    "422": dict(w=96, h=64, xblen=16, xbsep=12, prec=0, weights=(1, 1, 1), chroma=(1, 0), mv_range=24),
}


def case_of(ctx, kind, seed, **over):
    a = dict(KINDS[kind], **over)
    return make_case(ctx, a.pop("w"), a.pop("h"), a.pop("xblen"), a.pop("xbsep"), a.pop("prec"), a.pop("weights"),
                     a.pop("chroma"), a.pop("mv_range"), seed, **a)


def render(ctx, cases, order=None):
    """One call for the planes of all `cases` (in `order`, a permutation of the planes, if given); every plane checked."""
    jobs = [j for c in cases for j in c[0]]
    if order is not None:
        jobs = [jobs[i] for i in order]
    ctx.obmc_batch(jobs)
    for _, want, keep in cases:
        check_case(want, keep)


@pytest.mark.parametrize("first", sorted(KINDS))
def test_pairs_of_kinds(ctx, first):
    """Every ordered pair of kinds in one call -- a kind with itself too, with other contents."""
    for n, second in enumerate(sorted(KINDS)):
        a = case_of(ctx, first, 1000 + 7 * n)
        b = case_of(ctx, second, 2000 + 11 * n)
        try:
            render(ctx, [a, b])
        except AssertionError as e:
            raise AssertionError("%s then %s: %s" % (first, second, e)) from e


def test_plane_order(ctx):
    """Batches of 3 - 5 unlike pictures with their planes shuffled: V in front of U, planes of other pictures between a
    picture's U and V, and U and V planes of DIFFERENT pictures next to each other that share their geometry -- and, in
    the last batches, their vectors too, which the U / V merges look at."""
    rng = np.random.default_rng(4242)
    names = sorted(KINDS)
    for rnd in range(24):
        kinds = [names[int(i)] for i in rng.choice(len(names), int(rng.integers(3, 6)), replace=False)]
        cases = [case_of(ctx, k, 3000 + 17 * rnd + n) for n, k in enumerate(kinds)]
        order = rng.permutation(sum(len(c[0]) for c in cases))
        render(ctx, cases, order)
    # hand-made orders: V before U; U of one picture next to V of another of the same geometry
    for kind in ("fullpel_420", "halfpel_plain", "halfpel_pair", "pred_only", "zero_residual", "422"):
        y = [0, 3, 6]
        u, v = [1, 4, 7], [2, 5, 8]
        for order in ([2, 1, 0, 5, 4, 3, 8, 7, 6],                    # every picture V, U, Y
                      [1, 5, 4, 8, 7, 2] + y,                          # U0 V1 | U1 V2 | U2 V0
                      [u[0], v[1], u[1], v[0], u[2], v[2]] + y):       # U0 V1 U1 V0, then a picture's own pair
            render(ctx, [case_of(ctx, kind, 4100 + n + 10 * order[0]) for n in range(3)], order)
    # pictures that share vectors and geometry (the merges compare the vectors' address): a U / V job may take the U
    # plane of one and the V plane of the other
    for kind in ("fullpel_420", "halfpel_plain", "halfpel_pair", "pred_only", "blk20_12"):
        a = KINDS[kind]
        P = synth.motion_params(a["w"], a["h"], a["xblen"], a["xbsep"], a["prec"], a["weights"], a["chroma"])
        mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], a["mv_range"], 77)
        d_mv = ctx.upload_bytes(mv)
        for order in ([0, 1, 5, 3, 4, 2], [1, 5, 4, 2, 0, 3], None):
            cases = [case_of(ctx, kind, 4200 + n, mv=(mv, d_mv)) for n in range(2)]
            render(ctx, cases, order)
        d_mv.free()
    # ... and of other picture weights (default, a gain below one that differs in its bits alone, a fade, a gain): the U
    # plane of each next to the V plane of the next -- full-pel planes and half-pel one-component images
    for prec in (0, 1):
        P = synth.motion_params(96, 64, 12, 8, prec, (1, 1, 1), (1, 1))
        mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], 24 << prec, 78)
        d_mv = ctx.upload_bytes(mv)
        cases = [make_case(ctx, 96, 64, 12, 8, prec, wt, (1, 1), 24 << prec, 4300 + n, mv=(mv, d_mv))
                 for n, wt in enumerate(((1, 1, 1), (1, 1, 2), (1, 3, 2), (2, 3, 1)))]
        render(ctx, cases, [0, 3, 6, 9, 1, 5, 4, 8, 7, 11, 10, 2])
        d_mv.free()


def device_cus():
    """The device's compute units, as the library reads them (hipDeviceProp_t::multiProcessorCount), in a child process."""
    p = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return int(p.stdout.split()[-1])


def test_across_the_pairs_pay_threshold(ctx):
    """Two 3840 x 2160 4:2:0 pictures with half-pel chroma in one-component images carry more chroma tiles than the
    device has workgroup slots (six per CU): the call then merges U + V of such planes into two-plane jobs -- for every
    picture of the call, the small ones of other kinds beside them too.  The same small pictures alone stay below the
    threshold.  Both calls exact."""
    cus = device_cus()
    tiles = lambda w, h: ((w + 127) // 128) * ((h + 31) // 32)
    big = [make_case(ctx, 3840, 2160, 12, 8, 1, (1, 1, 1), (1, 1), 32, 50 + n) for n in range(2)]
    small_kinds = ("halfpel_plain", "blk20_12", "zero_residual", "fullpel_420", "pred_only", "qpel_fade_pair", "gain", "422")

    def small_cases(seed):
        out = [case_of(ctx, k, seed + n) for n, k in enumerate(small_kinds)]
        # plain half-pel chroma as well in the forms with two-plane kernels: prediction-only, s32 residual, 32 / 16 blocks
        out.append(case_of(ctx, "pred_only", seed + 20, pair=False))
        out.append(case_of(ctx, "s32_residual", seed + 21, pair=False))
        out.append(case_of(ctx, "blk32_16", seed + 22, pair=False))
        return out
    # (an upper bound of the small pictures' chroma tiles: every chroma plane counted, row kernel or not)
    small_tiles = sum(tiles(*comp_size(KINDS[k]["w"], KINDS[k]["h"], 1, KINDS[k]["chroma"])) * 2 for k in small_kinds)
    small_tiles += 4 * tiles(48, 32) + 2 * tiles(68, 36)
    big_tiles = 2 * 2 * tiles(1920, 1080)
    assert big_tiles > 6 * cus, (big_tiles, cus)
    assert small_tiles <= 6 * cus, (small_tiles, cus)
    mixed = small_cases(5000)
    render(ctx, mixed[:4] + big[:1] + mixed[4:8] + big[1:] + mixed[8:])
    render(ctx, small_cases(5100))
    print("device compute units: %d (pair tiles: big batch %d, small batch at most %d, threshold %d)" % (
        cus, big_tiles + small_tiles, small_tiles, 6 * cus))


def test_shared_references(ctx):
    """Pictures of different block sets, weights and precision classes that share ref1 and / or ref2 (the tile order
    groups a launch's tiles by their first reference), mixed with pictures that share nothing."""
    w, h = 136, 72
    ups = [Ref(ctx, w, h, (1, 1), True, True, 6000 + 10 * r) for r in range(3)]             # half-pel, chroma pair images
    plain_ups = [Ref(ctx, w, h, (1, 1), True, False, 6100 + 10 * r) for r in range(2)]     # half-pel, one-component images
    full = [Ref(ctx, w, h, (1, 1), False, False, 6200 + 10 * r) for r in range(2)]          # full pel
    A, B, C_ = ups
    pics = [
        dict(xblen=12, xbsep=8, prec=2, weights=(1, 1, 1), refs=[A, B]),
        dict(xblen=32, xbsep=16, prec=1, weights=(3, 5, 3), refs=[B, A]),
        dict(xblen=12, xbsep=8, prec=3, weights=(2, 3, 1), refs=[A, B]),
        dict(xblen=20, xbsep=12, prec=2, weights=(1, 1, 1), refs=[A, None], one_ref=True, prediction_only=1),
        dict(xblen=16, xbsep=12, prec=2, weights=(1, 1, 1), refs=[B, B], prediction_only=2),
        dict(xblen=12, xbsep=8, prec=1, weights=(1, 1, 1), refs=[C_, A], yblen=16, ybsep=12, residual=False),
        dict(xblen=64, xbsep=32, prec=2, weights=(1, 1, 1), refs=[A, C_]),
        dict(xblen=12, xbsep=8, prec=1, weights=(1, 1, 1), refs=plain_ups),
        dict(xblen=24, xbsep=16, prec=2, weights=(1, 3, 2), refs=plain_ups[::-1], res_dtype=np.int32),
        dict(xblen=12, xbsep=8, prec=1, weights=(1, 1, 1), refs=plain_ups, prediction_only=1),
        dict(xblen=12, xbsep=8, prec=0, weights=(1, 1, 1), refs=full),
        dict(xblen=16, xbsep=8, prec=0, weights=(3, 5, 3), refs=full[::-1]),
        dict(xblen=12, xbsep=8, prec=0, weights=(1, 1, 1), refs=[full[0], None], one_ref=True, prediction_only=1),
    ]
    rng = np.random.default_rng(61)
    for rnd in range(4):
        cases = []
        for n, p in enumerate(pics):
            p = dict(p)
            prec = p.pop("prec")
            cases.append(make_case(ctx, w, h, p.pop("xblen"), p.pop("xbsep"), prec, p.pop("weights"), (1, 1), 40 << prec,
                                   6300 + 31 * rnd + n, **p))
        # pictures with references of their own
        cases += [case_of(ctx, k, 6400 + 5 * rnd + n) for n, k in enumerate(("halfpel_pair", "fullpel_420", "qpel_fade_pair"))]
        order = None if rnd == 0 else rng.permutation(sum(len(c[0]) for c in cases))
        render(ctx, cases, order)
    for r in ups + plain_ups + full:
        r.free()


def test_weight_table_split_among_other_groups(ctx):
    """test_more_block_geometries_in_a_call_than_a_table_slot_holds's 48 luma planes of 48 geometries (one launch group
    whose weight tables overflow a slot: several launches, tiles rebased) with planes of other launch keys between
    them -- and pictures of the same key (the 16-pixel row kernel, half-pel) among them."""
    w, h, prec = 72, 56, 2
    geos = [(16, xbsep, yblen, ybsep) for xbsep in (8, 12, 16) for ybsep in (4, 8, 12, 16, 20, 24, 28, 32)
            for yblen in range(ybsep, min(2 * ybsep, 32) + 1, 4)][:48]
    ref = [Ref(ctx, w, h, (1, 1), True, False, 7000 + 10 * r) for r in range(2)]
    geo_cases = [make_case(ctx, w, h, xblen, xbsep, prec, (1, 1, 1), (1, 1), 24, 7100 + n, yblen=yblen, ybsep=ybsep,
                           refs=ref, only=(0,)) for n, (xblen, xbsep, yblen, ybsep) in enumerate(geos)]
    others = [case_of(ctx, k, 7200 + n) for n, k in enumerate(("halfpel_pair", "pred_only", "gain", "qpel_fade_pair", "fullpel_420",
                                                                "pred_s16", "blk32_16", "eighth", "halfpel_plain", "zero_residual"))]
    # (and a picture whose luma plane takes the same key as the 48: 16-pixel rows, quarter pel, default weights)
    others.append(case_of(ctx, "rect", 7300, xblen=16, xbsep=12))
    jobs, n_other = [], 0
    for n, c in enumerate(geo_cases):
        jobs += c[0]
        if n % 5 == 4 and n_other < len(others):
            jobs += others[n_other][0]
            n_other += 1
    for c in others[n_other:]:
        jobs += c[0]
    assert len(jobs) <= 128, len(jobs)
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.obmc_batch(jobs)
    ctx.synchronize()
    launches = ctx.profile_read()["obmc"][1]
    ctx.profile_enable(False)
    assert launches >= 3, launches
    for c in geo_cases + others:
        check_case(c[1], c[2])
    for r in ref:
        r.free()


def test_prediction_outside_8_bits_in_a_mixed_call(ctx):
    """One prediction-only picture whose LUMA DC values do not fit 8 bits, beside pictures with residuals and other
    prediction-only pictures in one call: the call answers SCHRO_HIP_ENEEDS_RESIDUAL once and names its own number; every
    other plane -- the same picture's chroma planes included (their DC values are in range) -- is exact.  (What lands in
    the overflowing plane itself is for the residual order to replace.)"""
    def widen(mv, P):
        dc = np.flatnonzero((mv["flags"] & 3) == 0)
        mv["v"][dc[::3], 0] = np.array([300, -400, 1000], np.int16)[np.arange(len(dc[::3])) % 3]
    wide = make_case(ctx, 160, 96, 12, 8, 2, (1, 1, 1), (1, 1), 40, 8000, modes=(0.3, 0.3, 0.1, 0.3), edit_mv=widen, pair=True,
                     prediction_only=1)
    others = [case_of(ctx, k, 8100 + n) for n, k in enumerate(("halfpel_pair", "pred_only", "fullpel_420", "pred_s16", "gain"))]
    others.append(case_of(ctx, "pred_only", 8110, pair=False))
    others.append(case_of(ctx, "fullpel_420", 8111, prediction_only=1))
    ctx.synchronize()
    before = ctx.lib.schro_hip_obmc_prediction_epoch(ctx.h)
    jobs = others[0][0] + others[1][0][:2] + wide[0] + others[1][0][2:] + [j for c in others[2:] for j in c[0]]
    with pytest.raises(sa.SchroHipError, match="does not fit") as ei:
        ctx.obmc_batch(jobs)
        ctx.synchronize()
    assert ei.value.code == _lib.ENEEDS_RESIDUAL
    epoch = ctx.lib.schro_hip_obmc_prediction_epoch(ctx.h)
    assert epoch == before + 1 and ("batch(es) %d " % epoch) in str(ei.value)
    ctx.synchronize()                                   # (reported once)
    got = (C.c_uint * 4)()
    assert ctx.lib.schro_hip_obmc_overflowed(ctx.h, got, 4) == 1 and got[0] == epoch
    assert ctx.lib.schro_hip_obmc_overflowed(ctx.h, got, 4) == 0
    check_case([x for x in wide[1] if x[2] != 0], wide[2])
    for c in others:
        check_case(c[1], c[2])
