"""Host side of tests/test_gpu_row_forms.py: the row kernels' tables as parsed, a picture for every entry, and a brute-force
proof that every block geometry obmc_row_form admits fits the tables of the kernel it picks."""
import os
import re
import subprocess

import pytest

import row_forms as R

ROOT = R.ROOT


def test_tables_parse_into_one_kernel_per_form():
    ks = R.parse()
    table = R.table_kernels()
    assert len(ks) == 96 and len(table) == 95
    assert sorted(n for n, k in ks.items() if k.experiments) == sorted(R.EXPERIMENT_SWITCHES)
    for kind in R.SOURCES:
        forms = [k.form for k in table.values() if k.form.kind == kind]
        assert len(forms) == len(set(forms)), kind
    # the fallbacks the sources pin with static_asserts
    assert R.row_find(R.Form(1, 3, 1, 2, True, True)) == "obmc_row_kernel_w_h2_3_1"
    assert R.row_find(R.Form(1, 2, 2, 1, True, False)) == "obmc_row_kernel_2_2"
    assert R.row_find(R.Form(1, 3, 2, 1, False, True)) is None
    assert R.row_find(R.Form(0, 3, 2, 1, True, False)) == "obmc_row_plain_3_2"
    assert R.row_find(R.Form(3, 2, 1, 1, True, False)) == "obmc_row_eighth_2_1"
    # the padded kernel has the form of the prediction-only 12-byte kernel it stands in for
    assert ks["obmc_row_kernel_p_3_1_pad"].form == ks["obmc_row_kernel_p_3_1"].form


def _row_kernel_symbols(lib):
    p = subprocess.run(["nm", "-C", lib], capture_output=True, text=True)
    assert p.returncode == 0, (lib, p.stderr[-2000:])
    return set(re.findall(r"\b(obmc_row_(?:kernel|plain|eighth)_\w+)\(", p.stdout))


def test_parsed_names_are_the_librarys_kernel_symbols():
    """The parsed names are exactly the row kernels of the built library (nm: their host-side launch stubs), and the
    experiments library's are those and its padded kernel.  Without a built library (a checkout before build ()) the parse
    is all there is -- test_tables_parse_into_one_kernel_per_form."""
    lib = os.path.join(ROOT, "schroedinger_amd", "libschro_hip.so")
    exp = os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so")
    if not os.path.exists(lib):
        pytest.skip("libschro_hip.so is not built")
    names = set(R.table_kernels())
    syms = _row_kernel_symbols(lib)
    assert syms == names, (sorted(syms - names), sorted(names - syms))
    if os.path.exists(exp):
        syms = _row_kernel_symbols(exp)
        assert syms == set(R.parse()), (sorted(syms - set(R.parse())), sorted(set(R.parse()) - syms))


@pytest.mark.parametrize("cus", [32, 80, 256, 304])
def test_every_entry_has_a_case(cus, tmp_path):
    """case_for gives every table entry a picture whose plane takes that form -- obmc_row_form, compiled from its source,
    admits the plane's block geometry with that row length; the planes of two-plane forms are carried over pairs_pay by the
    picture itself."""
    exe = R.admission_program(str(tmp_path))
    for name, k in R.table_kernels().items():
        for prec in ((1, 2) if k.form.kind == 1 else (None,)):
            a = R.case_for(k.form, cus, prec)
            comp = a["component"]
            hs, vs = a["chroma"] if comp else (0, 0)
            xblen = a["xblen"] >> hs
            seg = xblen * (2 if k.form.np == 3 else 1)
            ns = 2 if seg > 16 else 1
            assert (ns, max(2, (seg // ns + 3) // 4)) == (k.form.ns, k.form.nd), (name, a)
            yblen, ybsep = a.get("yblen", a["xblen"]) >> vs, a.get("ybsep", a["xbsep"]) >> vs
            geo = (xblen, yblen, a["xbsep"] >> hs, ybsep, 1 if k.form.np == 3 else 0)
            assert R.run_admission(exe, [geo]) == [(k.form.nd, k.form.ns)], (name, a)
            assert (a.get("prediction_only", 0) == 1) == k.form.nores, name
            assert (a["weights"] != (1, 1, 1)) == k.form.weighted, name
            assert {0: (0,), 1: (1, 2), 3: (3,)}[k.form.kind].count(a["prec"]), name
            if k.form.np == 3:
                assert a["pair"] == (a["prec"] > 0) and a["chroma"][0] == 1, name
            if k.form.np == 2:
                assert R.chroma_pair_tiles(a) >= R.pairs_pay_tiles(cus), (name, a)
                assert not a.get("pair"), name
            if k.form.np == 2 and k.form.kind == 0:
                # past the (U, V) jobs' tile limit, inside the plane jobs'
                cw, ch = a["w"], a["h"]
                assert ((cw + 63) // 64) * ((ch + 31) // 32) > 0xffff >= ((cw + 127) // 128) * ((ch + 31) // 32)


@pytest.fixture(scope="module")
def admission(tmp_path_factory):
    exe = R.admission_program(str(tmp_path_factory.mktemp("admission")))
    recs, caps, th = R.enumerate_geometries(exe)
    return exe, recs, caps, th


def test_capacities_come_from_the_header(admission):
    exe, _, caps, th = admission
    hdr = open(os.path.join(R.CSRC, "obmc_row_body.h")).read()
    assert "constexpr int kRTH = %d;" % th in hdr
    assert len(caps) == 12
    for (nd, ns, uv), (tw, blk, item) in caps.items():
        assert tw == (64 if uv else 128) and blk > 0 and item > 0


def test_every_admitted_geometry_fits_its_tables(admission):
    """Every geometry schro_params_verify_block_params allows, luma and every chroma subsampling, as a plane and as a (U, V)
    job: where obmc_row_form (compiled from its source) takes it, the blocks and (block, row) items that meet one tile --
    counted over every tile phase -- fit RowGeo's kBlk / kItem, a block row's segments fit 255 and the block rows fit the
    tile record's 8 bits."""
    _, recs, _, _ = admission
    admitted = [r for r in recs if r["nd"]]
    assert len(admitted) > 1000
    bad = []
    for r in admitted:
        assert r["class"] == (r["nd"], r["ns"], r["uv"]), r
        c, cap = r["counts"], r["caps"]
        if c["blk"] > cap["blk"] or c["item"] > cap["item"] or c["nbi"] > 255 or c["nbj"] > 255:
            bad.append(r)
    assert not bad, bad[:5]


def test_full_pel_two_plane_forms_need_the_pair_tile_limit(admission):
    """At full pel a picture's U and V planes become one (U, V) job wherever obmc_row_form takes them as one: no geometry
    admits a plane of one segment and refuses the (U, V) job -- so the full-pel two-plane kernels are reached through the
    (U, V) jobs' tile limit alone (row_forms.FULLPEL_TWO_PLANE)."""
    _, recs, _, _ = admission
    by = {(r["geo"], r["uv"]): r for r in recs}
    gaps = [g for (g, uv), r in by.items() if not uv and r["nd"] and r["ns"] == 1 and not by[(g, True)]["nd"]]
    assert not gaps, gaps[:5]


def test_capacity_limits_are_found_for_every_class(admission):
    """The geometries test_gpu_row_forms.py renders at the capacities: for every class the admitted ones closest to each
    table and, of the geometries whose counts exceed a table, the one with the smallest load over it."""
    _, recs, _, _ = admission
    limits = R.limit_geometries(recs)
    assert len(limits) == 10          # (2, 3, 4 dwords) x (1, 2 segments) x (plane, (U, V)), less the two-segment rows of 8 bytes
    for c, slot in limits.items():
        assert "refused" in slot and "blk" in slot and "item" in slot, c
        r = slot["refused"]
        assert not r["nd"] and (r["counts"]["blk"] > r["caps"]["blk"] or r["counts"]["item"] > r["caps"]["item"]
                                or r["counts"]["nbi"] > 255), r
    cases = R.capacity_cases(limits)
    assert {s for _, s, _ in cases} == {"admitted", "refused"}


def test_limit_cases_sit_on_both_sides():
    L = R.limit_cases()
    names = [n for n, _, _ in L]
    assert len(names) == len(set(names))
    for prec in range(4):
        m = R.origin_limit(prec)
        assert ((m + 32) << prec) <= 32767 < ((m + 33) << prec)
        assert "origin_p%d_w%d" % (prec, m) in names and "origin_p%d_h%d" % (prec, m + 1) in names
    assert R.origin_limit(3) == 4063
    t = {n: s for n, _, s in L}
    tiles = lambda s, tw: ((s["w"] + tw - 1) // tw) * ((s["h"] + 31) // 32)
    assert tiles(t["tiles_luma_65535"], 128) == 0xffff and tiles(t["tiles_luma_65536"], 128) == 0x10000
    assert tiles(t["tiles_uv_65535"], 64) == 0xffff
    a = R.FULLPEL_TWO_PLANE
    assert tiles(a, 64) == 0x10000


def test_admitted_limit_cases_fit_the_admission(tmp_path):
    """The block geometry of every rendered plane of an admitted-side limit case is one obmc_row_form takes (the sizes,
    weights and references each case is about are the GPU file's to show: test_route_witness)."""
    exe = R.admission_program(str(tmp_path))
    for name, side, s in R.limit_cases():
        if side != "admitted":
            continue
        for k in s.get("only", (0, 1, 2)):
            hs, vs = s["chroma"] if k else (0, 0)
            uv = 1 if k and (s.get("pair") or s["prec"] == 0) else 0
            geo = (s["xblen"] >> hs, s.get("yblen", s["xblen"]) >> vs, s["xbsep"] >> hs, s.get("ybsep", s["xbsep"]) >> vs, uv)
            assert R.run_admission(exe, [geo])[0][0], (name, k, geo)


def test_row_length_cases_differ_in_row_length_alone():
    """The 36-byte-row cases are refused for their rows: their blocks are no higher than 32, and their 32-byte twins are the
    same blocks but for the length."""
    t = {n: s for n, _, s in R.limit_cases()}
    for a, b in (("row_32_bytes_p0", "row_36_bytes_p0"), ("row_32_bytes_p2", "row_36_bytes_p2"),
                 ("uv_row_32_bytes", "uv_row_36_bytes")):
        hs, vs = t[b]["chroma"] if t[b]["only"] != (0,) else (0, 0)
        assert t[b].get("yblen", t[b]["xblen"]) >> vs <= 32, b
        assert t[b]["xblen"] >> hs << (1 if t[b].get("pair") else 0) == 36, b
        assert t[a]["xblen"] >> hs << (1 if t[a].get("pair") else 0) == 32, a
        assert {k: v for k, v in t[a].items() if k not in ("xblen", "xbsep", "yblen", "ybsep")} == \
            {k: v for k, v in t[b].items() if k not in ("xblen", "xbsep", "yblen", "ybsep")}
