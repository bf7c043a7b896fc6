#!/usr/bin/env python3
"""What an s16 render costs on each OBMC route (schro_motion_render_hip's mc_tmp_frame: prediction_only 2).

Pictures: 8 x 2160p 4:2:0 between two references -- the headline's 12 / 8 blocks at quarter pel, the encoder-default 32 / 16
set at full pel, and the headline's blocks with a fade (3, 5, bits 3).  Each is measured, in a fresh child process per figure:
  s16_row   into s16 planes, product library (the row kernels)
  s16_item  into s16 planes, experiments library with SCHRO_HIP_OBMC_KERNEL=item (obmc.hip's item / per-pixel kernel)
  u8_res    the same pictures' u8 residual-form launch, product library
and the HAVE_CUDA order per 2160p picture through the frame layer (schro_motion_render_hip into an S16 frame,
schro_hipframe_add, schro_hipframe_convert) on both routes.  The children alternate between the routes, round after round; the
table gives medians over the rounds.  OBMC times are the launches' own (per-launch events, Context.profile_read); the frame
order's is the context stream's elapsed time around the three calls.

  python scripts/s16_render_ab.py [--rounds 5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, PICTURES = 3840, 2160, 8
CASES = {"headline_12_8_qpel": (12, 8, 2, (1, 1, 1)), "encoder_32_16_fullpel": (32, 16, 0, (1, 1, 1)),
         "fade_12_8_qpel": (12, 8, 2, (3, 5, 3))}
EXP = os.path.join(ROOT, "schroedinger_amd", "libschro_hip_exp.so")
ROUTE_ENV = {"row": {}, "item": {"SCHRO_HIP_LIB": EXP, "SCHRO_HIP_OBMC_KERNEL": "item"}}


def child_obmc(case, mode, steps):
    import numpy as np
    import schroedinger_amd as sa
    import synth
    xblen, xbsep, prec, weights = CASES[case]
    ctx = sa.Context(0)
    P = synth.motion_params(W, H, xblen, xbsep, prec, weights, (1, 1))
    cw, ch = W // 2, H // 2
    refs = []
    for r in range(2):
        y, u, v = (ctx.upload(synth.picture_u8(h, w, seed=10 * r + k)) for k, (h, w) in enumerate([(H, W), (ch, cw), (ch, cw)]))
        if prec == 0:
            refs.append([y, u, v])
            continue
        gy, gc = ctx.hp_plane(H, W), ctx.hp_plane(ch, cw, pair=True)
        ctx.upsample_batch([(y, gy), ((u, v), gc)])
        refs.append([gy, gc, gc])
    jobs = []
    for n in range(PICTURES):
        mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], 24 << prec, seed=40 + n)
        d_mv = ctx.upload_bytes(mv)
        for k, (h, w) in enumerate([(H, W), (ch, cw), (ch, cw)]):
            if mode == "u8_res":
                res = ctx.upload(synth.image_s(h, w, np.int16, seed=60 + 3 * n + k))
                out = ctx.plane(h, w, np.uint8)
                jobs.append(sa.obmc_plane(d_mv, P, k, refs[0][k], refs[1][k], res, out))
            else:
                jobs.append(sa.obmc_plane(d_mv, P, k, refs[0][k], refs[1][k], None, ctx.plane(h, w, np.int16), prediction_only=2))
    for _ in range(3):
        ctx.obmc_batch(jobs)
    ctx.synchronize()
    ctx.obmc_routes(reset=True)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(steps):
        ctx.obmc_batch(jobs)
    ctx.synchronize()
    ms, launches = ctx.profile_read()["obmc"]
    return {"ms": ms / steps, "launches": launches // steps, "routes": {k: v // steps for k, v in ctx.obmc_routes().items()}}


def child_frame(steps):
    import numpy as np
    import schroedinger_amd as sa
    import synth
    from schroedinger_amd import _lib, frames
    ctx = sa.Context(0)
    depth, prec = 3, 2
    P = synth.motion_params(W, H, 12, 8, prec, (1, 1, 1), (1, 1))
    params = frames.make_params(
        wavelet_filter_index=0, transform_depth=depth, iwt_luma_width=W, iwt_luma_height=H, iwt_chroma_width=W // 2,
        iwt_chroma_height=H // 2, num_refs=2, xblen_luma=12, yblen_luma=12, xbsep_luma=8, ybsep_luma=8, mv_precision=prec,
        picture_weight_bits=1, picture_weight_1=1, picture_weight_2=1, x_num_blocks=P["x_num_blocks"], y_num_blocks=P["y_num_blocks"])
    fmt16, fmt8 = frames.frame_format(np.int16, 1, 1), frames.frame_format(np.uint8, 1, 1)
    dims = [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
    refs = []
    for r in range(2):
        d = frames.DeviceFrame(ctx, fmt8, W, H).upload(frames.HostFrame([synth.picture_u8(h, w, seed=10 * r + k)
                                                                         for k, (h, w) in enumerate(dims)], 1, 1))
        u = frames.DeviceFrame(ctx, fmt8, W, H, upsampled=True)
        sa.check(ctx.lib.schro_upsampled_hipframe_upsample(u.ptr(), d.ptr()))
        refs.append(u)
    mv = synth.motion_field(P["x_num_blocks"], P["y_num_blocks"], 24 << prec, seed=40)
    motion = _lib.Motion(refs[0].ptr(), refs[1].ptr(), mv.ctypes.data, C.pointer(params))
    frame = frames.DeviceFrame(ctx, fmt16, W, H).upload(frames.HostFrame([synth.image_s(h, w, np.int16, seed=60 + k)
                                                                         for k, (h, w) in enumerate(dims)], 1, 1))
    mc_tmp, out = frames.DeviceFrame(ctx, fmt16, W, H), frames.DeviceFrame(ctx, fmt8, W, H)

    def order():
        sa.check(ctx.lib.schro_motion_render_hip(C.byref(motion), mc_tmp.ptr(), None, 0, None))
        sa.check(ctx.lib.schro_hipframe_add(frame.ptr(), mc_tmp.ptr()))
        sa.check(ctx.lib.schro_hipframe_convert(out.ptr(), frame.ptr()))
    for _ in range(3):
        order()
    ctx.synchronize()
    ctx.obmc_routes(reset=True)
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.timer_begin()
    for _ in range(steps):
        order()
    total = ctx.timer_end()
    prof = ctx.profile_read()
    return {"ms": total / steps, "obmc_ms": prof["obmc"][0] / steps, "routes": {k: v // steps for k, v in ctx.obmc_routes().items()}}


def run_child(args, env, steps):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--child"] + args, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("child %s failed (%d): %s" % (args, p.returncode, p.stderr[-3000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        kind = a.child[0]
        print(json.dumps(child_frame(a.steps) if kind == "frame" else child_obmc(a.child[1], a.child[2], a.steps)))
        return
    runs = [(case, mode, route) for case in CASES for mode, route in (("s16", "row"), ("s16", "item"), ("u8_res", "row"))]
    runs += [("frame_have_cuda_2160p", "frame", route) for route in ("row", "item")]
    got = {r: [] for r in runs}
    for n in range(a.rounds):
        for r in (runs if n % 2 == 0 else runs[::-1]):
            case, mode, route = r
            args = ["frame"] if mode == "frame" else ["obmc", case, mode]
            got[r].append(run_child(args, ROUTE_ENV[route], a.steps))
    lines = ["# scripts/s16_render_ab.py --rounds %d --steps %d: medians over the rounds, ms (per 8 x 2160p call; frame order: "
             "per 2160p picture)" % (a.rounds, a.steps)]
    for r in runs:
        case, mode, route = r
        ms = [x["ms"] for x in got[r]]
        extra = (" obmc %.4f" % statistics.median(x["obmc_ms"] for x in got[r])) if mode == "frame" else \
            (" launches %d" % got[r][0]["launches"])
        lines.append("%-24s %-7s %-5s %.4f (min %.4f max %.4f)%s routes %s" % (
            case, mode, route, statistics.median(ms), min(ms), max(ms), extra, json.dumps(got[r][0]["routes"])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
