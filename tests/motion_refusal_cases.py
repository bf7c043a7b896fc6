"""The refusal cases of the five motion stages (rough search, block matching, sub-pel, split 2, mode decision) as the
api tests have them, each answered through the stage's *_check entry point at made-up addresses: {case id: thunk}, the
thunk giving [return code, schro_hip_last_error () in full].  tests/golden/make_motion_refusals.py records the answers,
tests/test_motion_refusals.py replays them."""
import mode_cases as K
import schroedinger_amd as sa
import test_hier_bm_api as H
import test_mode_api as M
import test_rough_hint_api as R
import test_split2_api as S
import test_subpel_api as P
from schroedinger_amd import _lib
from test_rough_hint_api import Mem


def answer(check, *args):
    try:
        check(*args)
    except sa.SchroHipError as e:
        return [e.code, _lib.load().schro_hip_last_error().decode()]
    return [0, ""]


def _rough_chains():
    """test_rough_hint_api.test_chain_refusals_name_the_chain_and_the_level, case by case"""
    chain, good = R.chain, R.chain(slot=2)
    out = {"distance_nohint_0": ([chain()], 0, 4), "distance_nohint_21": ([chain()], 21, 4), "distance_hint_-2": ([chain()], 12, -2),
           "distance_hint_25": ([chain()], 12, 25), "blocks": ([good, chain(x_num_blocks=0)],), "block": ([good, chain(ybsep_luma=65)],),
           "reference": ([good, chain(ref_index=3)],), "levels_0": ([good, chain(0)],)}
    c = chain(8, 4000, 3000)
    c[0].append(c[0][-1])
    c[3].append(Mem(0x7000000))
    out["levels_9"] = ([good, c],)
    c = chain()
    lv = c[0][1]
    c[0][1] = (Mem(lv[0].ptr, lv[0].width - 1, lv[0].height), Mem(lv[1].ptr, lv[1].width - 1, lv[1].height), 0)
    out["half_width"] = ([good, c],)
    c = chain()
    lv = c[0][2]
    c[0][2] = (Mem(lv[0].ptr, lv[0].width, lv[0].height + 1), Mem(lv[1].ptr, lv[1].width, lv[1].height + 1), 0)
    out["half_height"] = ([good, c],)
    c = chain()
    c[3][2] = Mem(c[3][1].ptr + 20)
    out["field_over_own_field"] = ([good, c],)
    c = chain()
    c[3][0] = good[3][1]
    out["field_over_other_chain"] = ([good, c],)
    c = chain()
    c[3][1] = Mem(c[0][0][1].ptr + 4)
    out["field_over_plane"] = ([good, c],)
    c = chain()
    c[0][0] = (Mem(c[0][0][0].ptr, 51, 38, 50), c[0][0][1], 0)
    out["stride"] = ([good, c],)
    c = chain()
    c[3][1] = Mem(0)
    out["null_field"] = ([good, c],)
    return out


def _hbm_chains():
    """test_hier_bm_api.test_chain_refusals_name_the_chain_and_the_level, case by case"""
    chain, planes, good = H.chain, H.planes, H.chain(slot=2)
    out = {"blocks": ([good, chain(x_num_blocks=0)],), "block": ([good, chain(ybsep_luma=65)],), "reference": ([good, chain(ref_index=3)],),
           "levels_0": ([good, chain(0)],), "extension": ([good, chain(ext=7)],), "chroma_shifts": ([good, chain(h_shift=1, v_shift=2)],)}
    c = chain(8, 128, 100)
    c[0].append(c[0][-1])
    c[5].append(Mem(0x7000000))
    out["levels_9"] = ([good, c],)
    c = chain()
    f, r, e = c[0][2]
    c[0][2] = (planes(f[0].ptr, 25, 19), planes(r[0].ptr, 25, 19), e)
    out["half_level_2"] = ([good, c],)
    c = chain(1)
    f, r, e = c[0][1]
    c[0][1] = (planes(f[0].ptr, 51, 39), planes(r[0].ptr, 51, 39), e)
    out["half_level_1"] = ([good, c],)
    c = chain()
    c[5][2] = Mem(c[5][1].ptr + 20)
    out["field_over_own_field"] = ([good, c],)
    c = chain()
    c[5][0] = good[5][1]
    out["field_over_other_chain"] = ([good, c],)
    c = chain()
    c[5][1] = Mem(c[0][1][1][2].ptr + 4)
    out["field_over_plane"] = ([good, c],)
    c = chain()
    f, r, e = c[0][1]
    c[0][1] = ((Mem(f[0].ptr, 51, 38, 50), f[1], f[2]), r, e)
    out["stride"] = ([good, c],)
    for k in (2, 0):
        c = chain()
        c[5][k] = Mem(0)
        out["null_field_%d" % k] = ([good, c],)
    return out


def cases():
    out = {}

    def add(name, check, *args):
        assert name not in out, name
        out[name] = lambda: answer(check, *args)

    # ---- the rough search ----
    for n, (change, _) in enumerate(R.HINT_REFUSALS):
        add("rough_hint/table_%02d" % n, sa.rough_hint_check, [R.hint_picture(slot=2), R.hint_picture(**change)])
    a, b = R.hint_picture(slot=2), list(R.hint_picture())
    b[8] = a[8]
    add("rough_hint/one_field_twice", sa.rough_hint_check, [a, tuple(b)])
    b = list(R.hint_picture())
    b[7] = a[8]
    add("rough_hint/hint_is_another_field", sa.rough_hint_check, [a, tuple(b)])
    for name, args in _rough_chains().items():
        add("rough_me/" + name, sa.rough_me_check, *args)
    # ---- the block matching ----
    for n, (change, _) in enumerate(H.LEVEL_REFUSALS):
        add("hbm_level/table_%02d" % n, sa.hbm_level_check, [H.level(slot=2), H.level(**change)])
    a, b = H.level(slot=2), list(H.level())
    b[10] = a[10]
    add("hbm_level/one_field_twice", sa.hbm_level_check, [a, tuple(b)])
    b = list(H.level())
    b[9] = a[10]
    add("hbm_level/hint_is_another_field", sa.hbm_level_check, [a, tuple(b)])
    for name, args in _hbm_chains().items():
        add("hbm/" + name, sa.hbm_check, *args)
    # ---- the sub-pel refinement ----
    for n, (change, _) in enumerate(P.REFUSALS):
        add("subpel/table_%02d" % n, sa.subpel_check, [P.chain(slot=2), P.chain(**change)])
    a = P.chain(slot=2)
    add("subpel/one_field_twice", sa.subpel_check, [a, P.chain(field=a[8])])
    add("subpel/source_is_another_field", sa.subpel_check, [a, P.chain(src_field=a[8])])
    add("subpel/field_over_last_record", sa.subpel_check, [a, P.chain(field=Mem(a[8].ptr + P.FIELD_BYTES - 20))])
    # ---- the split-2 level ----
    for n, (change, _) in enumerate(S.REFUSALS):
        add("split2/table_%02d" % n, sa.split2_check, [S.picture(slot=2), S.picture(**change)])
    a = S.picture(slot=2)
    add("split2/one_motion_twice", sa.split2_check, [a, S.picture(motion=a[7])])
    add("split2/one_superblocks_twice", sa.split2_check, [a, S.picture(superblocks=a[8])])
    add("split2/field_is_another_motion", sa.split2_check, [a, S.picture(fields=[a[7], S.picture()[6][1]])])
    # ---- the mode decision ----
    for n, (index, value, _) in enumerate(K.REFUSED):
        good = [M.picture(slot=1), M.picture(slot=2)]
        bad = list(good[1])
        bad[index] = value(good)
        add("mode/table_%02d" % n, sa.mode_check, [good[0], tuple(bad)])
    add("mode/superblock_outside_width", sa.mode_check, [M.picture(w=16 * 8 - 32)])
    add("mode/superblock_outside_height", sa.mode_check, [M.picture(h=12 * 8 - 32)])
    return out
