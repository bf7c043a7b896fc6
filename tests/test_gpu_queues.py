"""Two in-order queues per context (schro_hip_context_select_queue / _queue_mark /
_queue_wait_mark): picture batch k's OBMC on queue 1 beside batch k + 1's inverse wavelet on
queue 0, with the decoder's stage dependencies as marks.  Every picture of every batch must
equal the oracle's, whatever the interleaving on the device."""
import numpy as np
import pytest

import oracle_lib as O
import schroedinger_amd as sa
import synth

pytestmark = pytest.mark.gpu


def test_pipelined_batches_equal_the_oracle(ctx):
    w, h, depth, filt, prec = 320, 256, 3, 0, 2
    P = synth.motion_params(w, h, 12, 8, prec, (1, 1, 1), (1, 1))
    op = O.MotionParams(**P)
    dims = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    refs = [[synth.picture_u8(hh, ww, seed=5 + 10 * r + k) for k, (hh, ww) in enumerate(dims)] for r in range(2)]
    ups = [[O.UpComp(p, upsample=True) for p in comps] for comps in refs]
    d_ref = [[ctx.upload(p) for p in comps] for comps in refs]
    nsets, steps = 2, 6
    sets = []
    for s in range(nsets):
        hp = [[ctx.hp_plane(hh, ww) for (hh, ww) in dims] for _ in range(2)]
        res = [ctx.plane(hh, ww, np.int16) for (hh, ww) in dims]
        out = [ctx.plane(hh, ww, np.uint8) for (hh, ww) in dims]
        sets.append(dict(hp=hp, res=res, out=out))
    # every step has its own coefficients and vectors; a set's frames are reused every nsets steps
    coeffs = [[synth.image_s(hh, ww, np.int16, seed=100 + 3 * k + c) >> 4 for c, (hh, ww) in enumerate(dims)]
              for k in range(steps)]
    mvs = [synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], 48, seed=200 + k) for k in range(steps)]
    d_co = [[ctx.upload(c) for c in cs] for cs in coeffs]
    d_mv = [ctx.upload_bytes(m) for m in mvs]
    got = []
    for k in range(steps):
        s = k % nsets
        b = sets[s]
        ctx.select_queue(0)
        ctx.queue_wait_mark(8 + s)
        ctx.upsample_batch([(d_ref[r][c], b["hp"][r][c]) for r in range(2) for c in range(3)])
        ctx.iiwt_batch([(d_co[k][c], b["res"][c]) for c in range(3)], depth, filt)
        ctx.queue_mark(s)
        ctx.select_queue(1)
        ctx.queue_wait_mark(s)
        ctx.obmc_batch([sa.obmc_plane(d_mv[k], P, c, b["hp"][0][c], b["hp"][1][c], b["res"][c], b["out"][c])
                        for c in range(3)])
        # the pictures leave on the render queue, behind their OBMC (and before the set is reused)
        got.append([b["out"][c].download() for c in range(3)])
        ctx.queue_mark(8 + s)
    ctx.select_queue(0)
    ctx.synchronize()
    for k in range(steps):
        for c, (hh, ww) in enumerate(dims):
            res = O.inverse_iwt(coeffs[k][c], depth, filt)
            want = O.motion_render(mvs[k], op, c, ups[0][c], ups[1][c], res, ww, hh)
            assert np.array_equal(got[k][c], want), "step %d component %d" % (k, c)


def test_queue_arguments_are_checked(ctx):
    with pytest.raises(sa.SchroHipError):
        ctx.select_queue(4)         # queues 0, 1 (kernels), 2, 3 (copies)
    with pytest.raises(sa.SchroHipError):
        ctx.queue_mark(16)
    ctx.queue_wait_mark(7)      # never recorded: no-op
    ctx.select_queue(0)


def test_queues_on_disjoint_compute_units():
    # schro_hip_queue_set_cu_mask: queue 0 on every fourth CU, queue 1 on the others -- the inverse wavelet on
    # one, the same on the other, both equal to the oracle's (a mask changes where a kernel runs, not what it does);
    # a context of its own: the masks stay with its queues
    ctx = sa.Context(0)
    try:
        q0 = [1 if i % 4 == 0 else 0 for i in range(256)]
        ctx.queue_set_cu_mask(0, q0)
        ctx.queue_set_cu_mask(1, [1 - b for b in q0])
        h, w, depth, filt = 144, 208, 3, 0
        coeff = synth.image_s(h, w, np.int16, seed=77) >> 3
        want = O.inverse_iwt(coeff, depth, filt)
        outs = []
        for q in (0, 1, 0):
            ctx.select_queue(q)
            src, dst = ctx.upload(coeff), ctx.plane(h, w, np.int16)
            ctx.iiwt_batch([(src, dst)], depth, filt)
            outs.append(dst)
        ctx.select_queue(0)
        ctx.synchronize()
        for n, dst in enumerate(outs):
            assert np.array_equal(dst.download(), want), n
        with pytest.raises(sa.SchroHipError):
            ctx.queue_set_cu_mask(7, q0)
    finally:
        ctx.close()


def test_encoder_calls_on_both_queues():
    """The encoder-side calls (forward wavelet, downsample, SAD scan, rough scan) on queue 1 beside an inverse and an
    in-place forward transform on queue 0, no host synchronisation between the steps: a second, larger transform grows
    queue 1's scratch behind a running one, and the synchronous rough scan keeps its results in the scratch the transform
    enqueued just before it still uses.  A context of its own: its queues' scratch starts empty.  Every result against
    its oracle at the end."""
    import ctypes as C

    import analysis_ref as A
    from schroedinger_amd import frames
    from test_gpu_iwt_forward import pixel_range
    ctx = sa.Context(0)
    try:
        filt = 0
        small = [pixel_range(240, 320, np.int16, seed=31 + k) for k in range(3)]
        big = pixel_range(1088, 1920, np.int16, seed=41)
        s_src = [ctx.upload(a) for a in small]
        s_co = [ctx.plane(240, 320, np.int16).fill(0x5a) for _ in small]
        s_back = [ctx.plane(240, 320, np.int16).fill(0xa5) for _ in small]
        s_co2 = [ctx.plane(240, 320, np.int16).fill(0x5a) for _ in small]
        b_src, b_co = ctx.upload(big), ctx.plane(1088, 1920, np.int16).fill(0x5a)
        # queue 0's in-place transform: a 4:2:0 s16 frame
        comps = [pixel_range(240, 320, np.int16, 51), pixel_range(120, 160, np.int16, 52), pixel_range(120, 160, np.int16, 53)]
        params = frames.make_params(wavelet_filter_index=1, transform_depth=3, iwt_luma_width=320, iwt_luma_height=240,
                                    iwt_chroma_width=160, iwt_chroma_height=120)
        fr = frames.DeviceFrame(ctx, frames.frame_format(np.int16, 1, 1), 320, 240).upload(frames.HostFrame(comps, 1, 1))
        # the analysis pictures: two levels with an apron of 8, scans over the second
        ext = 8
        pics = [A.picture(352, 288, 61), A.picture(352, 288, 62)]
        want_pyr = [A.pyramid(p, 2) for p in pics]
        d_pics = [ctx.upload(p) for p in pics]
        lvl1 = [ctx.plane(144 + 2 * ext, 176 + 2 * ext, np.uint8).fill(0x5a) for _ in pics]
        lvl2 = [ctx.plane(72 + 2 * ext, 88 + 2 * ext, np.uint8).fill(0x5a) for _ in pics]
        inner2 = [sa.SubPlane(p, ext, ext, 72, 88) for p in lvl2]
        rng = np.random.default_rng(71)
        scans = np.zeros(37, sa.SCAN_DTYPE)
        for s in scans:
            bw, bh = int(rng.integers(1, 17)), int(rng.integers(1, 17))
            x, y = int(rng.integers(0, 88 - bw + 1)), int(rng.integers(0, 72 - bh + 1))
            rx, ry, sw, sh = sa.metric_scan_setup(x, y, bw, bh, 88, 72, ext, 0, 0, int(rng.integers(1, 9)))
            s["x"], s["y"], s["block_width"], s["block_height"], s["ref_x"], s["ref_y"], s["scan_width"], s["scan_height"] = x, y, bw, bh, rx, ry, sw, sh
            s["gravity_x"] = s["dx"] = rx - x
            s["gravity_y"] = s["dy"] = ry - y
        P = dict(x_num_blocks=44, y_num_blocks=36, xbsep_luma=8, ybsep_luma=8)

        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 0))
        ctx.select_queue(1)
        ctx.iwt_batch(list(zip(s_src, s_co)), 3, filt)
        ctx.queue_mark(3)
        ctx.select_queue(0)
        ctx.queue_wait_mark(3)
        ctx.iiwt_batch(list(zip(s_co, s_back)), 3, filt)
        ctx.select_queue(1)
        ctx.iwt_batch([(b_src, b_co)], 4, filt)             # grows queue 1's scratch
        ctx.select_queue(0)
        sa.check(ctx.lib.schro_hipframe_iwt_transform(ctx.h, fr.ptr(), C.byref(params)))
        ctx.select_queue(1)
        ctx.downsample_batch([(s, d, ext) for s, d in zip(d_pics, lvl1)])
        ctx.downsample_batch([(sa.SubPlane(s, ext, ext, 144, 176), d, ext) for s, d in zip(lvl1, lvl2)])
        (res, met), = ctx.metric_scan_batch([(inner2[0], inner2[1], ext, scans)])
        ctx.iwt_batch(list(zip(s_src, s_co2)), 3, filt)
        mvs = ctx.rough_scan_nohint(lvl2[0], lvl2[1], P, 2, 4, 1, extension=ext)     # synchronous, queue 1
        ctx.select_queue(0)
        sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 1))
        ctx.synchronize()

        for k, a in enumerate(small):
            want = O.forward_iwt(a, 3, filt)
            assert np.array_equal(s_co[k].download(), want), ("forward on queue 1", k)
            assert np.array_equal(s_co2[k].download(), want), ("forward in front of the rough scan", k)
            assert np.array_equal(s_back[k].download(), a), ("inverse on queue 0", k)
        assert np.array_equal(b_co.download(), O.forward_iwt(big, 4, filt)), "the transform that grew the scratch"
        for k, g in enumerate(fr.download()):
            assert np.array_equal(g, O.forward_iwt(comps[k], 3, 1)), ("in place on queue 0", k)
        for n in range(2):
            assert np.array_equal(lvl1[n].download(), A.edgeextend(want_pyr[n][1], ext)), ("level 1", n)
            assert np.array_equal(lvl2[n].download(), A.edgeextend(want_pyr[n][2], ext)), ("level 2", n)
        got_r, got_m = res.download(), met.download()
        for k, s in enumerate(scans):
            m = A.do_scan(want_pyr[0][2], want_pyr[1][2], s)
            assert np.array_equal(got_m[k, :m.size], m), ("scan", k)
            assert tuple(int(v) for v in got_r[k]) == A.get_min(m, s) + (0,), ("scan", k)
        want_mv = A.rough_scan_nohint(want_pyr[0][2], want_pyr[1][2], P, 2, 4, 1, extension=ext)
        assert mvs.tobytes() == want_mv.tobytes(), "rough scan behind a forward transform"
        fr.unref()
    finally:
        ctx.close()
