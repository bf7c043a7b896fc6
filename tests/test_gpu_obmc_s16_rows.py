"""GPU parity: s16 planes (prediction_only 2 -- schro_motion_render_hip's mc_tmp_frame, the prediction - 128) on the OBMC
row kernels, and the route report (schro_hip_obmc_routes) that says where every plane went.

An s16 plane takes the residual-form row kernel of its form (obmc_row_body.h: row_finish_s16 / _s16_uv / _s16_plain) wherever
a u8 plane of the same geometry, weights and references would; gain and negative weights stay on obmc.hip's per-pixel
kernel.  Every plane is compared bit for bit with the oracle's accumulator through orc_rrshift6_s16_ip_2d
(oracle_lib.rrshift6_s16), and Context.obmc_routes is read after every call.  test_route_witness runs some of the cases
again under rocprofv3 and checks that the kernels that ran are the routes the context reported."""
import csv
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import row_forms as R
import schroedinger_amd as sa
import synth
from schroedinger_amd import _lib, frames
from test_gpu_mixed_batches import device_cus
from test_gpu_obmc import check_case, comp_size, make_case
from test_gpu_row_forms import build, fullpel_two_plane_refs  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = R.table_kernels()
RESIDUAL_FORMS = sorted(n for n, k in KERNELS.items() if not k.form.nores)
# (test_route_witness's children append every call's routes here)
ROUTES_LOG = os.environ.get("SCHRO_TEST_ROUTES_LOG")


@pytest.fixture(scope="module")
def cus():
    return device_cus()


def routes_of(ctx, jobs):
    """One schro_hip_obmc_batch call; the planes it handed to each route."""
    ctx.obmc_routes(reset=True)
    ctx.obmc_batch(jobs)
    got = ctx.obmc_routes(reset=True)
    if ROUTES_LOG:
        with open(ROUTES_LOG, "a") as f:
            f.write(json.dumps(got) + "\n")
    return got


def only_row(n):
    return {"row": n, "item": 0, "general": 0, "strip": 0}


def s16(spec, **over):
    """A row_forms spec as an s16 picture (make_case: prediction_only 2 needs the residual flag left on)."""
    a = dict(spec, prediction_only=2, **over)
    a["residual"] = True
    return a


@pytest.mark.parametrize("name", RESIDUAL_FORMS)
def test_every_residual_form(ctx, cus, name, request):
    """One s16 picture per residual-form table entry (every precision, plain planes and pair images, fades, one and two
    segments, plane, two-plane and (U, V) jobs): rim blocks, far vectors and DC blocks, and whole interior tiles (the fast
    finish); the form's planes all report `row`."""
    form = KERNELS[name].form
    only = (0,) if form.np == 1 else (1, 2)
    for prec in ((1, 2) if form.kind == 1 else (None,)):
        a = R.case_for(form, cus, prec)
        p = a["prec"]
        cases = []
        if form.np == 2:
            big = {}
            if form.kind == 0:
                big = dict(refs=request.getfixturevalue("fullpel_two_plane_refs"))
            cases.append(build(ctx, s16(a), 11, **big))
        small = s16({k: v for k, v in a.items() if k != "only"}, only=only)
        for n, one_ref in enumerate((False, True)):
            cases.append(build(ctx, small, 20 + n, w=96, h=64, mv_range=96 << p, one_ref=one_ref, modes=(0.2, 0.3, 0.2, 0.3)))
            cases.append(build(ctx, small, 30 + n, w=416, h=240, mv_range=3 << p, one_ref=one_ref))
        jobs = [j for c in cases for j in c[0]]
        assert routes_of(ctx, jobs) == only_row(len(jobs)), (name, prec)
        for _, want, keep in cases:
            check_case(want, keep)


def wide_dc(mv, P):
    """DC blocks with 300, -400 and 32767 in every component: on the picture's rim (the first and last block row and
    column) and scattered through the overlapped interior -- the reference's 16-bit sums wrap."""
    nby, nbx = P["y_num_blocks"], P["x_num_blocks"]
    idx = np.arange(nbx * nby)
    bx, by = idx % nbx, idx // nbx
    rim = (bx == 0) | (by == 0) | (bx == nbx - 1) | (by == nby - 1)
    sel = np.flatnonzero((rim & (idx % 2 == 0)) | (idx % 5 == 0))
    mv["flags"][sel] -= mv["flags"][sel] & 3
    vals = np.array([300, -400, 32767], np.int16)
    for n, b in enumerate(sel):
        mv["v"][b, :3] = vals[n % 3]


@pytest.mark.parametrize("prec,pair", [(0, False), (1, True), (2, True), (2, False), (3, False)])
def test_wide_dc_values_wrap_as_the_reference(ctx, prec, pair):
    """DC values of 300, -400 and 32767 in overlapped blocks and at the rim: exact, and the same routes as the u8 residual
    form of the same picture (all row kernels for the headline's 12 / 8 blocks)."""
    kw = dict(modes=(0.4, 0.2, 0.2, 0.2), edit_mv=wide_dc, pair=pair)
    for w, h in ((416, 240), (100, 52)):
        twin = make_case(ctx, w, h, 12, 8, prec, (1, 1, 1), (1, 1), 20 << prec, 71, **kw)
        want_routes = routes_of(ctx, twin[0])
        check_case(twin[1], twin[2])
        jobs, want, keep = make_case(ctx, w, h, 12, 8, prec, (1, 1, 1), (1, 1), 20 << prec, 71, prediction_only=2, **kw)
        assert routes_of(ctx, jobs) == want_routes == only_row(3), (w, h, want_routes)
        check_case(want, keep)


class Window:
    """Plane `out` of make_case inside a larger s16 plane: it starts at pixel (x0, y0) of it and has its stride."""

    def __init__(self, parent, x0, y0, w, h):
        self.parent, self.x0, self.y0 = parent, x0, y0
        self.width, self.height, self.stride = w, h, parent.stride
        self.ptr = parent.ptr + y0 * parent.stride + 2 * x0

    def download(self):
        return self.parent.download()[self.y0:self.y0 + self.height, self.x0:self.x0 + self.width]


@pytest.mark.parametrize("x0,y0,stride_pad", [(1, 3, 6), (8, 2, 0), (3, 0, 2)])
@pytest.mark.parametrize("prec,pair", [(0, False), (2, True), (2, False)])
def test_planes_inside_larger_planes(ctx, x0, y0, stride_pad, prec, pair):
    """s16 planes that start at an odd pixel or whose rows are not 16 bytes apart (the per-pixel finish), and one that is
    aligned (the fast finish), inside a larger plane whose margin stays as it was."""
    parents = []

    def alloc(role, h, w, dtype):
        assert role == "out" and dtype == np.int16
        stride = (2 * (w + x0 + 5) + 63) // 64 * 64 + stride_pad
        p = ctx.plane(h + y0 + 3, w + x0 + 5, np.int16, stride=stride).fill(0x11)
        parents.append(p)
        return Window(p, x0, y0, w, h)

    jobs, want, keep = make_case(ctx, 416, 104, 12, 8, prec, (1, 1, 1), (1, 1), 24 << prec, 81, pair=pair,
                                 modes=(0.2, 0.3, 0.2, 0.3), edit_mv=wide_dc, prediction_only=2, alloc=alloc)
    assert routes_of(ctx, jobs) == only_row(3)
    check_case(want, keep)
    for (_, out, _), p in zip(want, parents):
        full = p.download()
        inside = np.zeros(full.shape, bool)
        inside[y0:y0 + out.height, x0:x0 + out.width] = True
        assert (full[~inside] == 0x1111).all()
        p.free()


@pytest.mark.parametrize("weights", [(3, -1, 1), (5, 3, 2)])
@pytest.mark.parametrize("prec", [0, 2])
def test_gain_weights_stay_on_the_general_kernel(ctx, weights, prec):
    """A gain or a negative weight: obmc.hip's per-pixel kernel, exact (the 16-bit wrap included)."""
    jobs, want, keep = make_case(ctx, 136, 72, 12, 8, prec, weights, (1, 1), 24 << prec, 91, modes=(0.2, 0.3, 0.2, 0.3),
                                 edit_mv=wide_dc, prediction_only=2)
    assert routes_of(ctx, jobs) == {"row": 0, "item": 0, "general": 3, "strip": 0}
    check_case(want, keep)


def test_one_call_mixes_u8_and_s16_planes(ctx):
    """u8 residual, u8 prediction-only and s16 pictures of one form in one call, in both orders: every plane exact, and the
    only batch schro_hip_obmc_overflowed names is the call whose prediction-only picture has a DC value outside 8 bits --
    s16 planes with such values raise nothing."""
    def narrow_dc(mv, P):
        pass

    def call(order, pred_edit):
        cases = {
            "res": make_case(ctx, 416, 240, 12, 8, 2, (1, 1, 1), (1, 1), 40, 101, pair=True, edit_mv=wide_dc),
            "pred": make_case(ctx, 416, 240, 12, 8, 2, (1, 1, 1), (1, 1), 40, 102, pair=True, edit_mv=pred_edit,
                              prediction_only=1),
            "s16": make_case(ctx, 416, 240, 12, 8, 2, (1, 1, 1), (1, 1), 40, 103, pair=True, edit_mv=wide_dc,
                             prediction_only=2),
        }
        jobs = [j for k in order for j in cases[k][0]]
        assert routes_of(ctx, jobs) == only_row(9)
        return cases, ctx.lib.schro_hip_obmc_prediction_epoch(ctx.h)

    got = (C.c_uint * 8)()
    # the prediction-only picture fits 8 bits: nothing is named
    cases, _ = call(("res", "pred", "s16"), narrow_dc)
    ctx.synchronize()
    assert ctx.lib.schro_hip_obmc_overflowed(ctx.h, got, 8) == 0
    for k in ("res", "pred", "s16"):
        check_case(cases[k][1], cases[k][2])
    # ... it does not: that call alone is named
    cases, epoch = call(("s16", "pred", "res"), wide_dc)
    with pytest.raises(sa.SchroHipError) as ei:
        ctx.synchronize()
    assert ei.value.code == _lib.ENEEDS_RESIDUAL
    ctx.synchronize()
    assert ctx.lib.schro_hip_obmc_overflowed(ctx.h, got, 8) == 1 and got[0] == epoch
    for k in ("res", "s16"):
        check_case(cases[k][1], cases[k][2])
    for p in cases["pred"][2]:
        p.free()


def round_up(x, depth):
    return -(-x // (1 << depth)) << depth


@pytest.mark.parametrize("prec", [0, 1, 2, 3])
@pytest.mark.parametrize("hs,vs", [(1, 1), (1, 0), (0, 0)])
def test_the_have_cuda_order_runs_on_the_row_kernels(ctx, hs, vs, prec):
    """The frame layer's HAVE_CUDA order (schrodecoder.c:1742-1760, 1908-1910, 2011): schro_motion_render_hip into an S16
    mc_tmp_frame, schro_hipframe_add, schro_hipframe_convert -- exact at every step, and its planes on the routes of the CPU
    call's fused u8 form (add TRUE) of the same picture: every plane on the row kernels at 4:2:0 and 4:4:4.  (4:2:2 chroma of
    the 12 / 8 set -- 6 x 12 blocks every 4 x 8 samples -- meets more rows of a tile than the row kernels' tables hold, u8 and
    s16 alike: obmc.hip's item kernel)"""
    w, h, depth = 200, 120, 3
    pd = [comp_size(w, h, k, (hs, vs))[::-1] for k in range(3)]
    il = (round_up(h, depth + vs), round_up(w, depth + hs))
    iw = [il, (il[0] >> vs, il[1] >> hs), (il[0] >> vs, il[1] >> hs)]
    P = synth.motion_params(w, h, 12, 8, prec, (1, 1, 1), (hs, vs))
    mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], 24 << prec, seed=19, modes=(0.2, 0.3, 0.2, 0.3))
    wide_dc(mv, P)
    params = frames.make_params(
        wavelet_filter_index=0, transform_depth=depth, iwt_luma_width=iw[0][1], iwt_luma_height=iw[0][0],
        iwt_chroma_width=iw[1][1], iwt_chroma_height=iw[1][0], num_refs=2, xblen_luma=12, yblen_luma=12,
        xbsep_luma=8, ybsep_luma=8, mv_precision=prec, picture_weight_bits=1, picture_weight_1=1,
        picture_weight_2=1, x_num_blocks=P["x_num_blocks"], y_num_blocks=P["y_num_blocks"])
    fmt16, fmt8 = frames.frame_format(np.int16, hs, vs), frames.frame_format(np.uint8, hs, vs)
    resid = [synth.image_s(ih, iwd, np.int16, seed=60 + k) for k, (ih, iwd) in enumerate(iw)]
    frame = frames.DeviceFrame(ctx, fmt16, iw[0][1], iw[0][0]).upload(frames.HostFrame(resid, hs, vs))
    refs_np = [[synth.picture_u8(ph, pw, seed=70 + 10 * r + k) for k, (ph, pw) in enumerate(pd)] for r in range(2)]
    refs = []
    for r in range(2):
        d = frames.DeviceFrame(ctx, fmt8, w, h).upload(frames.HostFrame(refs_np[r], hs, vs))
        if prec > 0:
            u = frames.DeviceFrame(ctx, fmt8, w, h, upsampled=True)
            sa.check(ctx.lib.schro_upsampled_hipframe_upsample(u.ptr(), d.ptr()))
            refs.append(u)
        else:
            refs.append(d)
    mc_tmp = frames.DeviceFrame(ctx, fmt16, iw[0][1], iw[0][0])
    motion = _lib.Motion(refs[0].ptr(), refs[1].ptr(), mv.ctypes.data, C.pointer(params))
    fused = frames.DeviceFrame(ctx, fmt8, w, h)
    ctx.obmc_routes(reset=True)
    sa.check(ctx.lib.schro_motion_render_hip(C.byref(motion), None, frame.ptr(), 1, fused.ptr()))
    u8_routes = ctx.obmc_routes(reset=True)
    got_fused = fused.download()
    sa.check(ctx.lib.schro_motion_render_hip(C.byref(motion), mc_tmp.ptr(), None, 0, None))
    assert ctx.obmc_routes(reset=True) == u8_routes
    assert u8_routes == only_row(3) if (hs, vs) != (1, 0) else u8_routes["row"] == 1 and u8_routes["general"] == 0
    got_pred = mc_tmp.download()
    preds = []
    for k, (ph, pw) in enumerate(pd):
        _, acc = O.motion_render(mv, O.MotionParams(**P), k, O.UpComp(refs_np[0][k], upsample=prec > 0),
                                 O.UpComp(refs_np[1][k], upsample=prec > 0), np.zeros((ph, pw), np.int16), pw, ph, return_acc=True)
        preds.append(O.rrshift6_s16(acc))
        assert np.array_equal(got_pred[k][:ph, :pw], preds[k]), k
    sa.check(ctx.lib.schro_hipframe_add(frame.ptr(), mc_tmp.ptr()))
    got_sum = frame.download()
    out = frames.DeviceFrame(ctx, fmt8, w, h)
    sa.check(ctx.lib.schro_hipframe_convert(out.ptr(), frame.ptr()))
    got = out.download()
    for k, (ph, pw) in enumerate(pd):
        want_sum = O.frame_add(resid[k][:ph, :pw], preds[k])
        assert np.array_equal(got_sum[k][:ph, :pw], want_sum), k
        assert np.array_equal(got[k], O.convert_u8(want_sum, pw, ph)), k
        assert np.array_equal(got_fused[k], O.motion_render(mv, O.MotionParams(**P), k, O.UpComp(refs_np[0][k], upsample=prec > 0),
                                                           O.UpComp(refs_np[1][k], upsample=prec > 0), resid[k], pw, ph)), k


def _child(tmp_path, tag, k):
    """Run this file's tests selected by `k` in a child under rocprofv3's kernel trace: ({kernel: launches}, [routes of
    every call])."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        pytest.fail("rocprofv3 is not installed: the route witness needs its kernel trace")
    out, log = tmp_path / tag, tmp_path / (tag + ".routes")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "-o", "run", "--",
           sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__), "-k", k]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, SCHRO_TEST_ROUTES_LOG=str(log)), capture_output=True, text=True,
                       timeout=2400)
    assert p.returncode == 0, (tag, p.stdout[-4000:], p.stderr[-4000:])
    counts = {}
    for f in glob.glob(os.path.join(str(out), "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"(obmc_\w+)", row["Name"])
                if m:
                    counts[m.group(1)] = counts.get(m.group(1), 0) + int(row["Calls"])
    routes = [json.loads(line) for line in open(str(log))]
    return counts, routes


@pytest.mark.timeout(3000)
def test_route_witness(tmp_path):
    """The routes the context reports are the kernels rocprofv3 saw: s16 pictures of every residual form launch row
    kernels only, gain weights obmc.hip's per-pixel kernel only."""
    rows, routes = _child(tmp_path, "forms", "test_every_residual_form and not 2_2")
    assert routes and all(r["row"] > 0 and r["item"] == r["general"] == r["strip"] == 0 for r in routes), routes
    assert any(n.startswith("obmc_row_") for n in rows) and not rows.get("obmc_kernel") and not rows.get("obmc_item_kernel"), rows
    gen, routes = _child(tmp_path, "gain", "test_gain_weights")
    assert routes and all(r["general"] > 0 and r["row"] == r["item"] == r["strip"] == 0 for r in routes), routes
    assert gen.get("obmc_kernel", 0) > 0 and not any(n.startswith("obmc_row_") or n == "obmc_item_kernel" for n in gen), gen
    print("s16 forms:", {n: c for n, c in sorted(rows.items())})
    print("gain weights:", gen)
