"""GPU parity: every OBMC row kernel, and both sides of every limit of obmc_row_form (obmc_row.hip).

The row kernels are 95 instantiations picked by form (tests/row_forms.py parses them out of the three ROW_ENTRY tables) and
one more the experiments library runs under SCHRO_HIP_OBMC_PAD=1.  test_every_form renders, for each table entry, pictures
with a plane of that form (row_forms.case_for): a small one with rim blocks, vectors far outside and DC blocks and one with
whole interior tiles, with two references and with one.  The limit tests sit on the admitted side of each limit -- the row
kernels at their widest origins and fullest tables -- and on the refused side, where obmc.hip's kernels must be exact.
Every plane is compared with the oracle's with np.array_equal.

test_route_witness runs this file again in child processes under rocprofv3 and reads which kernels ran: every table entry
at least once, no general kernel in the admitted cases, no row kernel in the refused ones."""
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import row_forms as R
import schroedinger_amd as sa
from test_gpu_mixed_batches import device_cus
from test_gpu_obmc import Ref, check_case, make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = R.table_kernels()
LIMITS = R.limit_cases()


@pytest.fixture(scope="module")
def cus():
    return device_cus()


@pytest.fixture(scope="module")
def capacity_limits(tmp_path_factory):
    exe = R.admission_program(str(tmp_path_factory.mktemp("admission")))
    recs, _, _ = R.enumerate_geometries(exe)
    return R.capacity_cases(R.limit_geometries(recs))


def offset_refs(ctx, a, seed, offset, stride_pad):
    """Two full-pel references whose planes start `offset` bytes into their buffers and whose rows are a stride of
    4 k + stride_pad bytes apart (the oracle's pictures are the same)."""
    refs = []
    for r in range(2):
        ref = Ref(ctx, a["w"], a["h"], a["chroma"], False, False, seed + 10 * (r + 1))
        for k in range(3):
            pic = ref.np[k]
            ch, cw = pic.shape
            stride = (cw + offset + 3) // 4 * 4 + stride_pad
            buf = np.zeros((ch + 1, stride), np.uint8)
            buf[:ch, offset:offset + cw] = pic
            p = ctx.plane(ch + 1, stride, np.uint8, stride=stride)
            p.upload(buf)
            ref.keep.append(p)
            ref.dev[k] = types.SimpleNamespace(ptr=p.ptr + offset, stride=stride)
        refs.append(ref)
    return refs


def build(ctx, spec, seed, **over):
    """make_case for a row_forms spec (its own keys resolved here)."""
    a = dict(spec, **over)
    for key in ("component", "big"):
        a.pop(key, None)
    offset, pad = a.pop("ref_offset", 0), a.pop("ref_stride_pad", 0)
    refs = None
    if offset or pad:
        refs = a["refs"] = offset_refs(ctx, a, seed, offset, pad)
    jobs, want, keep = make_case(ctx, a.pop("w"), a.pop("h"), a.pop("xblen"), a.pop("xbsep"), a.pop("prec"), a.pop("weights"),
                                 a.pop("chroma"), a.pop("mv_range"), seed, **a)
    if refs:
        keep = keep + [p for r in refs for p in r.keep]
    return jobs, want, keep


def render(ctx, cases):
    ctx.obmc_batch([j for c in cases for j in c[0]])
    for _, want, keep in cases:
        check_case(want, keep)


@pytest.fixture(scope="module")
def fullpel_two_plane_refs(ctx):
    """The references of the full-pel two-plane pictures (16384 x 8192 4:4:4), shared by their four forms."""
    a = R.FULLPEL_TWO_PLANE
    refs = [Ref(ctx, a["w"], a["h"], a["chroma"], False, False, 900 + 10 * r) for r in range(2)]
    yield refs
    for r in refs:
        r.free()


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_every_form(ctx, cus, name, request):
    form = KERNELS[name].form
    for prec in ((1, 2) if form.kind == 1 else (None,)):
        a = R.case_for(form, cus, prec)
        p = a["prec"]
        cases = []
        if form.np == 2:
            # the picture that takes the call over pairs_pay; the smaller pictures of the same form go with it
            assert R.chroma_pair_tiles(a) >= R.pairs_pay_tiles(cus), a
            big = {}
            if form.kind == 0:
                big = dict(refs=request.getfixturevalue("fullpel_two_plane_refs"))
            cases.append(build(ctx, a, 11, **big))
        small = {k: v for k, v in a.items() if k not in ("only",)}
        small["residual"] = True
        for n, one_ref in enumerate((False, True)):
            # rim blocks, vectors far beyond the apron, DC blocks; whole interior tiles with short vectors
            cases.append(build(ctx, small, 20 + n, w=96, h=64, mv_range=96 << p, one_ref=one_ref,
                               modes=(0.2, 0.3, 0.2, 0.3)))
            cases.append(build(ctx, small, 30 + n, w=416, h=240, mv_range=3 << p, one_ref=one_ref))
        render(ctx, cases)


def _limit_ids(side):
    return [(name, spec) for name, s, spec in LIMITS if s == side]


@pytest.mark.parametrize("name,spec", _limit_ids("admitted"), ids=[n for n, _ in _limit_ids("admitted")])
def test_limit_admitted(ctx, name, spec):
    render(ctx, [build(ctx, spec, 41), build(ctx, spec, 42, one_ref=True)] if not spec.get("big") else [build(ctx, spec, 41)])


@pytest.mark.parametrize("name,spec", _limit_ids("refused"), ids=[n for n, _ in _limit_ids("refused")])
def test_limit_refused(ctx, name, spec):
    render(ctx, [build(ctx, spec, 41), build(ctx, spec, 42, one_ref=True)] if not spec.get("big") else [build(ctx, spec, 41)])


@pytest.mark.parametrize("name,spec", _limit_ids("error"), ids=[n for n, _ in _limit_ids("error")])
def test_limit_error(ctx, name, spec):
    jobs, _, keep = build(ctx, spec, 41)
    with pytest.raises(sa.SchroHipError, match="picture_weight_bits"):
        ctx.obmc_batch(jobs)
    for p in keep:
        p.free()


def test_capacity_admitted(ctx, capacity_limits):
    """For every (row length, segments, (U, V)) class: the admitted geometries that come closest to the block table, the item
    table and 255 segments per block row (tests/test_row_forms.py proves they fit)."""
    for name, side, spec in capacity_limits:
        if side == "admitted":
            try:
                render(ctx, [build(ctx, spec, 51), build(ctx, spec, 52, one_ref=True, mv_range=4)])
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e)) from e


def test_capacity_refused(ctx, capacity_limits):
    """... and the first geometry of each class that the capacities refuse: obmc.hip's kernels."""
    for name, side, spec in capacity_limits:
        if side == "refused":
            try:
                render(ctx, [build(ctx, spec, 51), build(ctx, spec, 52, one_ref=True, mv_range=4)])
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e)) from e


def test_pad_kernel_form(ctx):
    """The experiments library's obmc_row_kernel_p_3_1_pad (SCHRO_HIP_OBMC_PAD=1): prediction-only 12-pixel luma rows at
    quarter pel.  Run by test_route_witness in a child with that library and switch; with the product library this is the
    p_3_1 kernel's picture."""
    a = R.case_for(R.parse()["obmc_row_kernel_p_3_1_pad"].form)
    render(ctx, [build(ctx, a, 61, w=416, h=240), build(ctx, a, 62, w=96, h=64, mv_range=160)])


def _kernel_launches(tmp_path, tag, k, env=None):
    """{kernel name: launches} of this file's tests selected by `k`, run in a child process under rocprofv3's kernel trace."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        pytest.fail("rocprofv3 is not installed: the route witness needs its kernel trace")
    out = tmp_path / tag
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "-o", "run", "--",
           sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__), "-k", k]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=2400)
    assert p.returncode == 0, (tag, p.stdout[-4000:], p.stderr[-4000:])
    files = glob.glob(os.path.join(str(out), "**", "*kernel_stats.csv"), recursive=True)
    assert files, (tag, os.listdir(str(out)))
    counts = {}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"(obmc_\w+)", row["Name"])
                if m:
                    counts[m.group(1)] = counts.get(m.group(1), 0) + int(row["Calls"])
    return counts


@pytest.mark.timeout(6000)
def test_route_witness(tmp_path):
    """Which kernels the cases above launch, from rocprofv3's kernel statistics: the forms and the admitted limits run row
    kernels only and every table entry at least once; the refused limits run obmc.hip's kernels only; the experiments
    library runs its padded kernel under its switch."""
    general = ("obmc_kernel", "obmc_item_kernel")
    forms = _kernel_launches(tmp_path, "forms", "test_every_form")
    missing = sorted(set(KERNELS) - {n for n, c in forms.items() if c > 0})
    assert not missing, "row kernels never launched: %s" % missing
    admitted = _kernel_launches(tmp_path, "admitted", "test_limit_admitted or test_capacity_admitted")
    assert not any(admitted.get(g) for g in general), admitted
    assert any(n.startswith("obmc_row_") for n in admitted), admitted
    refused = _kernel_launches(tmp_path, "refused", "test_limit_refused or test_capacity_refused")
    assert not any(n.startswith("obmc_row_") for n in refused), refused
    assert any(refused.get(g) for g in general), refused
    pad = _kernel_launches(tmp_path, "pad", "test_pad_kernel_form",
                           dict(SCHRO_HIP_LIB=os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so"),
                                **R.EXPERIMENT_SWITCHES["obmc_row_kernel_p_3_1_pad"]))
    assert pad.get("obmc_row_kernel_p_3_1_pad", 0) > 0, pad
    print("row kernel launches (%d kernels):" % (len(KERNELS) + 1))
    for n in sorted(KERNELS):
        print("  %-32s %d" % (n, forms[n]))
    print("  %-32s %d (experiments library, SCHRO_HIP_OBMC_PAD=1)" % ("obmc_row_kernel_p_3_1_pad", pad["obmc_row_kernel_p_3_1_pad"]))
    print("admitted limits:", {n: c for n, c in sorted(admitted.items())})
    print("refused limits:", {n: c for n, c in sorted(refused.items())})
