"""GPU: the host state around the encoder's launches -- the queues' grow-only scratch, the four table buffers and the table
slots of each queue, the two queues side by side -- which the stages' own tests, one call and one wait each on the session's
context, never move.  tests/encoder_pipeline_cases.py says which cases are enqueued in which order; every expected value
is the stages' own restatement's, every comparison bit for bit.

Every test creates contexts of its own, so that both queues' scratch, table buffers and table slots start empty.  Inputs
are uploaded and outputs laid out in guarded blocks (tests/guard_lib.py: every output holds a seeded pattern before the
calls) BEFORE the first call; from then on nothing waits on the host but what the test names -- the library's own wait where a
call grows the scratch or a table buffer comes round again, and the frame-layer entry points, which are synchronous -- until
the one synchronize in front of the comparisons.  A ballast of memsets (class Ballast) keeps the queues busy meanwhile, so
that the calls are in flight together and not one after the other."""
import ctypes as C

import numpy as np
import pytest

import analysis_ref as A
import encoder_pipeline_cases as P
import guard_lib as G
import hier_bm_cases as HK
import lowdelay_enc_cases as LC
import mode_cases as MC
import noarith_dec_cases as DC
import noarith_enc_cases as NC
import quant_cases as QC
import schroedinger_amd as sa
import split2_cases as S2
import subpel_cases as SP
import test_gpu_mode_decision as TM
import test_gpu_motion_encode as TV
import test_gpu_noarith_decode as TD
import test_gpu_noarith_encode as TN
import test_gpu_split2 as TS
import test_gpu_subpel as TP
from schroedinger_amd import _lib, frames

pytestmark = pytest.mark.gpu

MV = sa.MV_DTYPE.itemsize


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(1, -1)


def same(got, want, what):
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), what


class Ballast:
    """Work that keeps a queue busy while the test's calls are enqueued behind it, so that they pile up on the queue instead
    of running as they come: FILLS memsets of one large block (about 0.16 ms each; nine mode decision calls take about 4 ms
    to enqueue), which touch neither the scratch nor a table.  It goes BEHIND the first calls of a context: their first-use
    allocations (the scratch, the table buffers and their pinned mirrors) wait for the device and would wait the ballast out."""
    BYTES, FILLS = 1 << 30, 64

    def __init__(self, ctx):
        self.ctx, self.block = ctx, ctx.plane(1, self.BYTES, np.uint8)

    def enqueue(self, queues):
        for q in queues:
            self.ctx.select_queue(q)
            for _ in range(self.FILLS):
                self.block.fill(0x33)

    def free(self):
        self.block.free()


def upsampled_frames(ctx, refs, fmt, w, h, hs, vs, keep):
    """One upsampled device frame per reference (its planes given); the frames to unref go to `keep`."""
    ups = []
    for r in refs:
        d = frames.DeviceFrame(ctx, fmt, w, h).upload(frames.HostFrame(r, hs, vs))
        u = frames.DeviceFrame(ctx, fmt, w, h, upsampled=True)
        sa.check(ctx.lib.schro_upsampled_hipframe_upsample(u.ptr(), d.ptr()))
        keep += [u, d]
        ups.append(u)
    return ups


# ---- a stage: the entries of its plane-layer calls in guarded memory, and its frame-layer call --------------------------
#
# setup (names, frame_name) uploads everything -- it may wait --; call (k) enqueues the plane-layer call of entry k;
# frame_call () runs the frame-layer entry point on `frame_name` and keeps what it returned; check () compares all.

class Subpel:
    """schro_hip_subpel_batch (kind "subpel") or pass 1 alone: its error launch, its choice launch."""

    def __init__(self, ctx, kind="subpel"):
        self.ctx, self.kind, self.keep, self.planes = ctx, kind, [], []

    def setup(self, names, frame_name=None):
        self.names = names
        spans = []
        for name in names:
            n = TP.records(SP.CASES[name])
            spans.append({"subpel": {"start": (n * MV, False), "field": (n * MV, True)},
                          "subpel_error": {"field": (n * MV, False), "table": (n * 32, True)},
                          "subpel_choose": {"field": (n * MV, True), "table": (n * 32, False)}}[self.kind])
        self.rig = TP.Rig(self.ctx, [TP.case_entry(n) for n in names], spans, seed=len(names))
        for k, name in enumerate(names):
            if self.kind == "subpel":
                self.rig.put(k, "start", SP.inputs(name)[2])
            else:
                assert SP.CASES[name]["prec"] >= 1
                self.rig.put(k, "field", SP.fields_by_pass(name)[0])
                if self.kind == "subpel_choose":
                    self.rig.put(k, "table", SP.expected(name)[1][0])
        if frame_name:
            c = SP.CASES[frame_name]
            assert c["ref_index"] == 0          # (one reference: field 0 refines dx[0], dy[0])
            src, ref, self.start = SP.inputs(frame_name)
            self.frame_case = c
            self.d_src = self.ctx.upload(np.pad(src, c["ext"], mode="edge"))
            self.planes.append(self.d_src)
            chroma = np.zeros(((c["h"] + 1) // 2, (c["w"] + 1) // 2), np.uint8)
            self.ups = upsampled_frames(self.ctx, [[ref, chroma, chroma]], sa.FORMAT_U8_420, c["w"], c["h"], 1, 1, self.keep)
            self.frame_want = P.outputs("subpel", frame_name)

    def call(self, k):
        if self.kind == "subpel":
            self.ctx.subpel_batch([self.rig.chain(k, "start", "field")])
        elif self.kind == "subpel_error":
            self.ctx.subpel_error_batch([self.rig.chain(k, None, "field")], 1, [self.rig.span(k, "table")])
        else:
            self.ctx.subpel_choose_batch([self.rig.chain(k, None, "field")], 1, [self.rig.span(k, "table")])

    def frame_call(self):
        c = self.frame_case
        got = self.ctx.subpel_deep(self.d_src, self.ups, dict(SP.params_of(c), mv_precision=c["prec"]), c["lam"], [self.start], extension=c["ext"])
        return {"field": got[0]}

    def check(self):
        self.rig.check({(k, key): a for k, name in enumerate(self.names) for key, a in P.outputs(self.kind, name).items()})

    def free(self):
        self.rig.free()
        for p in self.planes:
            p.free()
        for f in self.keep:
            f.unref()


class ModeLike:
    """schro_hip_split2_batch and schro_hip_mode_decision_batch: the rigs of their own tests."""

    def __init__(self, ctx, kind):
        self.ctx, self.kind, self.keep, self.planes = ctx, kind, [], []
        self.K, self.T = (S2, TS) if kind == "split2" else (MC, TM)
        self.written = ("motion", "superblocks") if kind == "split2" else TM.OUTPUTS

    def setup(self, names, frame_name=None):
        self.names = names
        self.rig = self.T.Rig(self.ctx, [self.T.case_entry(n) for n in names], self.written, seed=len(names))
        for k, name in enumerate(names):
            ins = self.K.inputs(name)
            if self.kind == "split2":
                self.rig.put_fields(k, ins[2])
            else:
                self.rig.put_fields(k, *ins[2:])
        if frame_name:
            c = self.K.CASES[frame_name]
            ins = self.K.inputs(frame_name)
            hs, vs = S2.FORMATS[c["fmt"]]
            self.frame_case, self.frame_inputs, self.shifts = c, ins[2:], (hs, vs)
            self.src_planes = [self.ctx.upload(np.pad(p, c["ext"], mode="edge")) for p in ins[0]]
            self.planes += self.src_planes
            self.ups = upsampled_frames(self.ctx, ins[1], frames.frame_format(np.uint8, hs, vs), c["w"], c["h"], hs, vs, self.keep)
            self.frame_want = P.outputs(self.kind, frame_name)

    def call(self, k):
        if self.kind == "split2":
            self.ctx.split2_batch([self.rig.picture(k)])
        else:
            self.ctx.mode_decision_batch([self.rig.picture(k)])

    def frame_call(self):
        c, (hs, vs) = self.frame_case, self.shifts
        if self.kind == "split2":
            got = self.ctx.mode_decision_split2(self.src_planes, self.ups, S2.params_of(c), c["lam"], self.frame_inputs[0], extension=c["ext"],
                                                h_shift=hs, v_shift=vs)
        else:
            got = self.ctx.mode_decision(self.src_planes, self.ups, S2.params_of(c), c["lam"], *self.frame_inputs, extension=c["ext"], h_shift=hs,
                                         v_shift=vs)
        return dict(zip(self.written, got))

    def check(self):
        self.rig.check({(k, key): a for k, name in enumerate(self.names) for key, a in P.outputs(self.kind, name).items()})

    def free(self):
        self.rig.free()
        for p in self.planes:
            p.free()
        for f in self.keep:
            f.unref()


class Chain:
    """schro_hip_hbm_batch (with level 0) and schro_hip_rough_me_batch on pyramids made on the device, one per case; every
    entry has fields of its own."""

    def __init__(self, ctx, kind):
        self.ctx, self.kind, self.levels = ctx, kind, {}
        self.first = 0 if kind == "hbm" else 1

    def pyramid(self, name):
        """[level][component] of (frame, ref): planes with the apron, and the views of the pictures inside them."""
        if name not in self.levels:
            c = P.case(self.kind, name)
            ext = c["ext"]
            if self.kind == "hbm":
                pictures = HK.chain_pictures(c["w"], c["h"])
            else:
                frame, ref, _ = P.rough_chain(name)
                pictures = ([frame], [ref])
            out = []
            for planes in pictures:
                lv = [[self.ctx.upload(A.edgeextend(p, ext)) for p in planes]]
                for _ in range(P.CHAIN_LEVELS):
                    src = [sa.SubPlane(p, ext, ext, p.height - 2 * ext, p.width - 2 * ext) for p in lv[-1]]
                    dst = [self.ctx.plane((s.height + 1) // 2 + 2 * ext, (s.width + 1) // 2 + 2 * ext, np.uint8) for s in src]
                    self.ctx.downsample_batch([(s, d, ext) for s, d in zip(src, dst)])
                    lv.append(dst)
                out.append(lv)
            self.levels[name] = out
        return self.levels[name]

    @staticmethod
    def views(levels, ext):
        return [[sa.SubPlane(p, ext, ext, p.height - 2 * ext, p.width - 2 * ext) for p in lv] for lv in levels]

    def setup(self, names, frame_name=None):
        self.names = names
        lay = G.Layout()
        self.specs = []
        for k, name in enumerate(names):
            n = P.records(P.case(self.kind, name)) * MV
            self.specs.append({lv: lay.span(n, footprint=("bytes", n), name="field%d_l%d" % (k, lv), align=64, skew=4 * ((k + lv) % 3))
                               for lv in range(self.first, P.CHAIN_LEVELS + 1)})
        for name in set(names) | ({frame_name} if frame_name else set()):
            self.pyramid(name)
        self.block = G.GuardedBlock(self.ctx, lay, seed=len(names))
        self.ctx.synchronize()
        if frame_name:
            self.frame_name = frame_name
            self.frame_want = P.outputs(self.kind, frame_name)

    def call(self, k):
        name = self.names[k]
        c = P.case(self.kind, name)
        fl, rl = (self.views(lv, c["ext"]) for lv in self.pyramid(name))
        fields = [self.block[self.specs[k][lv]] for lv in range(self.first, P.CHAIN_LEVELS + 1)]
        if self.kind == "hbm":
            levels = [(fl[lv], rl[lv], c["ext"]) for lv in range(P.CHAIN_LEVELS + 1)]
            self.ctx.hbm_batch([(levels, 1, 1, c["params"], c["ref_index"], fields)], True)
        else:
            levels = [(fl[lv][0], rl[lv][0], c["ext"]) for lv in range(1, P.CHAIN_LEVELS + 1)]
            self.ctx.rough_me_batch([(levels, c["params"], c["ref_index"], fields)])

    def frame_call(self):
        c = P.case(self.kind, self.frame_name)
        fl, rl = self.pyramid(self.frame_name)
        if self.kind == "hbm":
            got = self.ctx.hbm_scan(fl, rl, c["params"], c["ref_index"], with_level0=True, extension=c["ext"], h_shift=1, v_shift=1)
        else:
            got = self.ctx.rough_scan([lv[0] for lv in fl], [lv[0] for lv in rl], c["params"], c["ref_index"], extension=c["ext"])
        return {"level%d" % lv: got[lv] for lv in range(self.first, P.CHAIN_LEVELS + 1)}

    def check(self):
        self.block.check({self.specs[k][int(key[5:])]: as_bytes(a) for k, name in enumerate(self.names)
                          for key, a in P.outputs(self.kind, name).items()})

    def free(self):
        self.block.free()
        for out in self.levels.values():
            for lv in out:
                for planes in lv:
                    for p in planes:
                        p.free()


class Noarith:
    """schro_hip_noarith_encode_batch with caller-owned buffers: the bytes and the result words of every entry in a guarded
    block, 37 bytes of room behind the bytes."""
    ROOM = 37

    def __init__(self, ctx):
        self.ctx, self.pics, self.keep = ctx, [], []

    def setup(self, names, frame_name=None):
        self.names = names
        words = C.sizeof(_lib.NoarithResult) // 4
        lay = G.Layout()
        self.specs = []
        for k, name in enumerate(names):
            n = len(NC.BY_NAME[name].expected()[0])
            self.specs.append((lay.span(n + self.ROOM, align=64, skew=k % 4, footprint=("bytes", n), name="out%d" % k),
                               lay.plane(1, words, np.uint32, footprint="rect", name="result%d" % k)))
        self.block = G.GuardedBlock(self.ctx, lay, seed=len(names))
        self.pics = [TN.picture_of(self.ctx, NC.BY_NAME[name]) for name in names]
        if frame_name:
            case = self.frame_case = NC.BY_NAME[frame_name]
            (w, h) = case.sizes[0]
            assert case.sizes[1] == ((w + 1) // 2, (h + 1) // 2)
            self.frame = frames.DeviceFrame(self.ctx, frames.frame_format(case.dtype, 1, 1), w, h).upload(frames.HostFrame(case.planes, 1, 1))
            self.keep.append(self.frame)
            self.params = frames.make_params(transform_depth=case.depth, num_refs=1, is_noarith=1, iwt_luma_width=w, iwt_luma_height=h,
                                             iwt_chroma_width=case.sizes[1][0], iwt_chroma_height=case.sizes[1][1],
                                             codeblock_mode_index=case.mode)
            for l in range(case.depth + 1):
                self.params.horiz_codeblocks[l], self.params.vert_codeblocks[l] = case.hc[l], case.vc[l]
            self.bound = sa.noarith_encode_bound(case.sizes, case.depth, case.hc, case.vc, case.dtype.itemsize)
            stats = case.expected()[2]
            self.frame_want = dict(P.outputs("noarith", frame_name), false_zero=np.array([stats["false_zero_codeblocks"], stats["false_zero_subbands"]]))
        self.ctx.synchronize()

    def call(self, k):
        out, res = self.specs[k]
        assert self.ctx.noarith_encode_batch([self.pics[k] + (self.block[out], out.extent, self.block[res])]) is None

    def frame_call(self):
        case = self.frame_case
        got, nbytes, bits, fz, status = self.ctx.encode_transform_data_noarith(self.frame, self.params, [case.record_indices(k) for k in range(3)],
                                                                               self.bound)
        assert status == 0 and nbytes == len(got)
        return {"bytes": got, "subband_bits": bits, "false_zero": np.array(fz)}

    def check(self):
        raw = self.block.raw()
        expected = {}
        for k, name in enumerate(self.names):
            data, bits, stats = NC.BY_NAME[name].expected()
            out, res = self.specs[k]
            result = sa.noarith_result(res.payload(raw))
            assert result["bytes"] == len(data) and result["overrun"] == 0, (k, name, result["bytes"], len(data))
            assert np.array_equal(result["subband_bits"], bits), (k, name)
            assert result["false_zero"] == (stats["false_zero_codeblocks"], stats["false_zero_subbands"]), (k, name)
            tail = self.block.before[out.offset + len(data):out.offset + out.extent]        # (the canary behind the bytes)
            expected[out] = np.concatenate([np.frombuffer(data, np.uint8), tail]).reshape(1, -1)
        self.block.check(expected)

    def free(self):
        self.block.free()
        for pic in self.pics:
            TN.free(pic)
        for f in self.keep:
            f.unref()


class Lowdelay:
    """schro_hip_lowdelay_encode_batch with caller-owned buffers: planes, slices, base indices and count in a guarded block."""

    def __init__(self, ctx):
        self.ctx, self.keep = ctx, []

    def setup(self, names, frame_name=None):
        self.names = names
        lay = G.Layout()
        self.specs = []
        for k, name in enumerate(names):
            Pm, planes, res = LC.expected(name)
            assert not LC.leaves_lds(Pm)
            nslices = Pm["n_horiz_slices"] * Pm["n_vert_slices"]
            nbytes = Pm["slice_bytes_num"] * nslices // Pm["slice_bytes_denom"]
            comp = [lay.plane(p.shape[0], p.shape[1], np.int16, stride=p.shape[1] * 2 + (0, 6, 64)[c], footprint=None, name="comp%d_%d" % (k, c))
                    for c, p in enumerate(planes)]
            self.specs.append(dict(comp=comp, slices=lay.span(nbytes, skew=k % 4, footprint=("bytes", nbytes), name="slices%d" % k),
                                   index=lay.span(nslices, skew=1, footprint=("bytes", nslices), name="index%d" % k),
                                   count=lay.span(4, footprint=("bytes", 4), name="count%d" % k)))
        self.block = G.GuardedBlock(self.ctx, lay, seed=len(names))
        for name, s in zip(names, self.specs):
            for c, p in enumerate(LC.expected(name)[1]):
                self.block[s["comp"][c]].upload(p)
        if frame_name:
            Pm, planes, res = LC.expected(frame_name)
            hs = int(Pm["iwt_chroma_width"] < Pm["iwt_luma_width"])
            vs = int(Pm["iwt_chroma_height"] < Pm["iwt_luma_height"])
            width = max(Pm["iwt_luma_width"], Pm["iwt_chroma_width"] << hs)
            height = max(Pm["iwt_luma_height"], Pm["iwt_chroma_height"] << vs)
            f = self.frame = frames.DeviceFrame(self.ctx, frames.frame_format(np.int16, hs, vs), width, height)
            self.keep.append(f)
            host = [np.zeros((f.c.components[k].height, f.c.components[k].width), np.int16) for k in range(3)]
            for h, p in zip(host, planes):
                h[:p.shape[0], :p.shape[1]] = p
            f.upload(frames.HostFrame(host, hs, vs))
            self.frame_params = Pm
            self.frame_want = P.outputs("lowdelay", frame_name)
        self.ctx.synchronize()

    def call(self, k):
        s, b = self.specs[k], self.block
        self.ctx.lowdelay_encode_batch([([b[c] for c in s["comp"]], b[s["slices"]], b[s["index"]], b[s["count"]])], LC.expected(self.names[k])[0])

    def frame_call(self):
        data, index, count = self.ctx.encode_lowdelay(self.frame, self.frame_params)
        return {"slices": data, "index": index, "count": np.array([count], np.uint32)}

    def check(self):
        self.block.check({self.specs[k][key]: as_bytes(a) for k, name in enumerate(self.names) for key, a in P.outputs("lowdelay", name).items()})

    def free(self):
        self.block.free()
        for f in self.keep:
            f.unref()


class NoarithDec:
    """schro_hip_noarith_decode_batch with caller-owned buffers: the input bytes, the coefficient and quant planes and the
    result words of every entry in a guarded block.  The launches behind the header walk read the records -- bands, chunk
    totals, chunk and codeblock records -- that earlier launches of the same call left in the scratch."""

    def __init__(self, ctx):
        self.ctx, self.keep = ctx, []

    def setup(self, names, frame_name=None):
        self.names = names
        self.cases = [DC.BY_NAME[name] for name in names]
        lay = G.Layout()
        self.specs = []
        for k, case in enumerate(self.cases):
            b = case.dtype.itemsize
            assert case.expected()[0] is not None
            stride = lambda w: (w * b + 63) // 64 * 64 + (k % 3) * b
            self.specs.append(dict(
                data=lay.span(max(len(case.data), 1), align=64, skew=k % 4, footprint=None, name="data%d" % k),
                coeffs=[lay.plane(h, w, case.dtype, stride=stride(w), skew=b * ((k + c) % 4), name="coeffs%d_%d" % (k, c))
                        for c, (w, h) in enumerate(case.sizes)],
                quant=[lay.plane(h, w, case.dtype, stride=stride(w), skew=b * ((k + c + 2) % 4), name="quant%d_%d" % (k, c))
                       for c, (w, h) in enumerate(case.sizes)],
                result=lay.plane(1, TD.WORDS, np.uint32, align=64, skew=4 * (k % 4), name="result%d" % k)))
        self.block = G.GuardedBlock(self.ctx, lay, seed=len(names))
        for case, s in zip(self.cases, self.specs):
            self.block[s["data"]].upload(np.frombuffer(case.data, np.uint8).reshape(1, -1))
        if frame_name:
            case = self.frame_case = DC.BY_NAME[frame_name]
            (w, h) = case.sizes[0]
            assert case.sizes[1] == ((w + 1) // 2, (h + 1) // 2) and not case.is_intra
            start = [np.full((hh, ww), 0x1234, case.dtype) for ww, hh in case.sizes]
            self.frame = frames.DeviceFrame(self.ctx, frames.frame_format(case.dtype, 1, 1), w, h).upload(frames.HostFrame(start, 1, 1))
            self.keep.append(self.frame)
            self.params = frames.make_params(transform_depth=case.depth, num_refs=1, is_noarith=1, iwt_luma_width=w, iwt_luma_height=h,
                                             iwt_chroma_width=case.sizes[1][0], iwt_chroma_height=case.sizes[1][1],
                                             codeblock_mode_index=case.mode)
            for l in range(case.depth + 1):
                self.params.horiz_codeblocks[l], self.params.vert_codeblocks[l] = case.hc[l], case.vc[l]
            want = P.outputs("noarith_dec", frame_name)
            self.frame_want = {"coeffs": want["coeffs"], "result": want["result"]}
        self.ctx.synchronize()

    def call(self, k):
        case, s, b = self.cases[k], self.specs[k], self.block
        assert self.ctx.noarith_decode_batch([(b[s["data"]], case.data_bytes, None, [b[c] for c in s["coeffs"]], [b[c] for c in s["quant"]],
                                               case.depth, case.hc, case.vc, case.mode, case.is_intra, case.compat, b[s["result"]])]) is None

    def frame_call(self):
        case = self.frame_case
        result, compat, status = self.ctx.decode_transform_data_noarith(self.frame, case.data, self.params, case.compat)
        assert status == 0 and compat == case.expected()[2]["compat_quant_offset"]
        return {"coeffs": np.concatenate([p.ravel() for p in self.frame.download()]), "result": P.noarith_dec_result_words(result)}

    def check(self):
        want = {}
        for case, s in zip(self.cases, self.specs):
            coeffs, quant, result = case.expected()
            want.update(zip(s["coeffs"], coeffs))
            want.update(zip(s["quant"], quant))
            want[s["result"]] = P.noarith_dec_result_words(result).reshape(1, -1)
        self.block.check(want)

    def free(self):
        self.block.free()
        for f in self.keep:
            f.unref()


class MotionEnc:
    """schro_hip_motion_encode_batch with caller-owned buffers: the rig of its own test -- the fields, the bytes with the
    bound's room and the result words of every entry in one guarded block."""

    def __init__(self, ctx):
        self.ctx = ctx

    def setup(self, names, frame_name=None):
        self.names = names
        cases = [P.case("motion_enc", name) for name in names]
        self.rig = TV.Rig(self.ctx, cases, [sa.motion_encode_bound(*c[2:6]) for c in cases], [k % 4 for k in range(len(cases))], seed=len(names))
        self.pictures = self.rig.pictures()
        if frame_name:
            self.frame_case = P.case("motion_enc", frame_name)
            self.frame_want = P.outputs("motion_enc", frame_name)
        self.ctx.synchronize()

    def call(self, k):
        assert self.ctx.motion_encode_batch([self.pictures[k]]) is None

    def frame_call(self):
        _, field, nbx, nby, num_refs, hg, _ = self.frame_case
        params = frames.make_params(x_num_blocks=nbx, y_num_blocks=nby, num_refs=num_refs, have_global_motion=hg, **TV.PARAMS)
        got, nbytes, sections, result, status = self.ctx.encode_motion_data_noarith(field, params, sa.motion_encode_bound(nbx, nby, num_refs, hg))
        assert status == 0 and nbytes == len(got)
        TV.same(got, result, self.frame_case)
        return {"bytes": np.frombuffer(bytes(got), np.uint8), "sections": np.array(sections, np.int64)}

    def check(self):
        self.rig.check()

    def free(self):
        self.rig.free()


class Quantise:
    """schro_hip_quantise_batch, one plane per call: coefficients, quantised values and summaries of every entry in a guarded
    block, the quant planes filled as tests/quant_cases.py fills them."""

    def __init__(self, ctx):
        self.ctx = ctx

    def setup(self, names, frame_name=None):
        assert frame_name is None
        self.names = names
        lay = G.Layout()
        self.specs = []
        for k, name in enumerate(names):
            s = P.quant_spec(name)
            buf = s["buf"]
            stride = buf.shape[1] * buf.dtype.itemsize
            self.specs.append(dict(coeffs=lay.plane(buf.shape[0], buf.shape[1], buf.dtype, stride=stride, name="coeffs%d" % k),
                                   quant=lay.plane(buf.shape[0], buf.shape[1], buf.dtype, stride=stride, name="quant%d" % k),
                                   summary=lay.plane(len(s["records"]), 2, np.uint32, stride=8, name="summary%d" % k)))
        self.block = G.GuardedBlock(self.ctx, lay, seed=len(names))
        fill = lambda buf: np.frombuffer(bytes([QC.QUANT_FILL]) * buf.nbytes, buf.dtype).reshape(buf.shape)
        for name, sp in zip(names, self.specs):
            buf = P.quant_spec(name)["buf"]
            self.block[sp["coeffs"]].upload(buf)
            self.block[sp["quant"]].upload(fill(buf))
        self.tables = [QC.table(P.quant_spec(name)["records"]) for name in names]
        self.ctx.synchronize()

    def call(self, k):
        # (the C call itself: Context.quantise_batch allocates the summaries, these lie in the guarded block)
        s, sp, tab = P.quant_spec(self.names[k]), self.specs[k], self.tables[k]
        co, qu, su = (self.block[sp[key]] for key in ("coeffs", "quant", "summary"))
        arr = (_lib.QuantPlane * 1)()
        a = arr[0]
        a.coeffs, a.quant, a.bytes = co.ptr, qu.ptr, co.stride * co.height
        a.codeblocks, a.ncodeblocks, a.is_intra = tab, len(tab), 1 if s["intra"] else 0
        a.dc_predict_first, a.dc_width, a.dc_height = s.get("dc") or (0, 0, 0)
        a.summary = su.ptr
        sa.check(self.ctx.lib.schro_hip_quantise_batch(self.ctx.h, arr, 1, co.dtype.itemsize))

    def check(self):
        want = {}
        for k, name in enumerate(self.names):
            out = P.outputs("quantise", name)
            want[self.specs[k]["coeffs"]], want[self.specs[k]["quant"]], want[self.specs[k]["summary"]] = out["recon"], out["quant"], out["summary"]
        self.block.check(want)

    def free(self):
        self.block.free()


def make_stage(ctx, stage):
    if stage.startswith("subpel"):
        return Subpel(ctx, stage)
    if stage in ("split2", "mode"):
        return ModeLike(ctx, stage)
    if stage in ("hbm", "rough"):
        return Chain(ctx, stage)
    return {"noarith": Noarith, "lowdelay": Lowdelay, "quantise": Quantise, "noarith_dec": NoarithDec, "motion_enc": MotionEnc}[stage](ctx)


# ---- 1. scratch from empty, grown behind a running call, then reused stale -----------------------------------------------

@pytest.mark.parametrize("stage", P.SCRATCH_STAGES)
def test_scratch_sequences(stage):
    """A, B, C through the plane-layer call with no wait in between -- the block allocated from empty, grown behind A, C's
    tables on B's leftovers --, then A through the frame-layer entry point, which sizes the block itself and is
    synchronous, and B through the plane layer behind it: on queue 1 alone, and on a second context every step on queue 0
    and on queue 1.  All results equal their expected values."""
    for both_queues in (False, True):
        sequence = P.scratch_sequence(stage, both_queues)
        plane = [(q, name) for q, name, layer in sequence if layer == "plane"]
        frame_name = P.stage(stage)["sequence"][0]
        ctx = sa.Context(0)
        try:
            s, ballast = make_stage(ctx, stage), Ballast(ctx)
            s.setup([name for _, name in plane], frame_name)
            try:
                ctx.synchronize()               # (the last wait in front of the sequence)
                sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 0))
                queues = sorted({q for q, _, _ in sequence})
                k, got = 0, []
                for n, (q, name, layer) in enumerate(sequence):
                    if n == len(queues):
                        ballast.enqueue(queues)         # A is enqueued on every queue: B grows the block behind work that still runs
                    ctx.select_queue(q)
                    if layer == P.FRAME:
                        assert name == frame_name
                        got.append((q, s.frame_call()))
                    else:
                        s.call(k)
                        k += 1
                ctx.select_queue(0)
                sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 1))
                ctx.synchronize()
                s.check()
                for q, out in got:
                    assert out.keys() >= s.frame_want.keys()
                    for key, want in s.frame_want.items():
                        same(out[key], want, (stage, "frame layer on queue %d" % q, key))
            finally:
                s.free()
                ballast.free()
        finally:
            ctx.close()


# ---- 2. more tables in flight than there are buffers ---------------------------------------------------------------------

@pytest.mark.parametrize("stage", P.NINE_CALL_STAGES)
def test_nine_calls_without_a_wait(stage):
    """Nine calls that cycle through three unlike cases, each with outputs of its own, and one synchronize behind them: on
    one queue, and on a second context dealt alternately to both."""
    for both_queues in (False, True):
        calls = P.nine_calls(stage, both_queues)
        ctx = sa.Context(0)
        try:
            s, ballast = make_stage(ctx, stage), Ballast(ctx)
            s.setup([name for _, name in calls])
            try:
                ctx.synchronize()               # (the last wait in front of the nine calls)
                queues = sorted({q for q, _ in calls})
                for k, (q, _) in enumerate(calls):
                    if k == min(P.BIG_TABLES * len(queues), len(calls) - 1):
                        ballast.enqueue(queues)         # every buffer has been used once: the next turn piles up behind this
                    ctx.select_queue(q)
                    s.call(k)
                ctx.select_queue(0)
                ctx.synchronize()
                s.check()
            finally:
                s.free()
                ballast.free()
        finally:
            ctx.close()


# ---- 3 and 4. the inter chain as a stream of enqueued calls ---------------------------------------------------------------

class ChainPicture:
    """Everything one chain picture has on the device, in one guarded block: the picture and its two references with their
    aprons (inputs), and every stage's output -- pyramid levels, fields, the mode decision's tables, prediction, residual
    (it holds the source before the subtraction), coefficients, reconstruction, quantised values, summaries, bytes and
    result words.  The half-pel images lie outside the block."""
    WHO = ("frame", "ref0", "ref1")

    def __init__(self, ctx, name, seed):
        self.ctx, self.name = ctx, name
        e = self.e = P.chain_expected(name)
        g = self.g = e["geometry"]
        ext, n = g["ext"], g["nbx"] * g["nby"]
        lay, s = G.Layout(), {}
        pyramids = dict(frame=e["frame_pyramid"], ref0=e["ref_pyramids"][0], ref1=e["ref_pyramids"][1])
        for who in self.WHO:
            for lv in range(P.CHAIN_PYRAMID + 1):
                for k in range(3):
                    h, w = pyramids[who][lv][k].shape
                    s[who, lv, k] = lay.plane(h + 2 * ext, w + 2 * ext, np.uint8, footprint="rect" if lv else None, name="%s level %d component %d" % (who, lv, k))

        def span(key, nbytes, skew=4):
            s[key] = lay.span(nbytes, footprint=("bytes", nbytes), name=" ".join(str(v) for v in key), align=64, skew=skew)
        for r in (0, 1):
            for lv in range(P.CHAIN_PYRAMID + 1):
                span(("hbm", r, lv), n * MV, 4 * r)
            span(("subpel", r), n * MV, 8 - 4 * r)
        span(("motion",), n * MV)
        span(("superblocks",), n // 16 * sa.SB_DTYPE.itemsize, 8)
        span(("trials",), n // 16 * 4 * sa.MODE_TRIAL_DTYPE.itemsize, 16)
        span(("stats",), 24, 8)
        words = C.sizeof(_lib.NoarithResult) // 4
        for k in range(3):
            (h, w), (ih, iw) = g["dims"][k], g["iwt"][k]
            s["prediction", k] = lay.plane(h, w, np.int16, stride=w * 2 + (2, 0, 6)[k], name="prediction %d" % k)
            s["residual", k] = lay.plane(ih, iw, np.int16, stride=iw * 2 + (0, 4, 2)[k], name="residual %d" % k)
            s["coefficients", k] = lay.plane(ih, iw, np.int16, name="coefficients %d" % k)
            s["reconstruction", k] = lay.plane(ih, iw, np.int16, stride=iw * 2 + (6, 2, 10)[k], name="reconstruction %d" % k)
            s["quantised", k] = lay.plane(ih, iw, np.int16, stride=iw * 2 + (6, 2, 10)[k], name="quantised values %d" % k)
            s["summaries", k] = lay.plane(len(P.chain_records(g, k, iw * 2)), 2, np.uint32, stride=8, name="summaries %d" % k)
        self.capacity = sa.noarith_encode_bound([(w, h) for h, w in g["iwt"]], P.CHAIN_DEPTH, g["hc"], g["vc"], 2)
        data = e["bytes"][0]
        assert self.capacity >= len(data)
        s["bytes",] = lay.span(self.capacity, align=64, skew=1, footprint=("bytes", len(data)), name="bytes")
        s["result",] = lay.plane(1, words, np.uint32, name="result")
        self.s, self.lay = s, lay
        self.blk = G.GuardedBlock(ctx, lay, seed=seed)
        for who in self.WHO:
            for k in range(3):
                self.blk[s[who, 0, k]].upload(A.edgeextend(pyramids[who][0][k], ext))
        for k in range(3):
            self.blk[s["residual", k]].upload(e["source"][k])
        self.hp = [[ctx.hp_plane(h, w) for (h, w) in g["dims"]] for _ in (0, 1)]
        self.tables = []
        for k, (ih, iw) in enumerate(g["iwt"]):
            tab = ctx.codeblock_layout(iw, ih, P.CHAIN_DEPTH, g["hc"], g["vc"], s["reconstruction", k].stride, 2)
            for t, rec in zip(tab, P.chain_records(g, k, s["reconstruction", k].stride)):
                assert (t.dst_offset, t.dst_stride, t.width, t.height) == tuple(rec[:4])
                t.quant_index = rec[4]
            self.tables.append(tab)

    def __call__(self, *key):
        return self.blk[self.s[key]]

    def view(self, who, lv, k):
        """the picture inside its apron"""
        p, ext = self(who, lv, k), self.g["ext"]
        return sa.SubPlane(p, ext, ext, p.height - 2 * ext, p.width - 2 * ext)

    # -- what the calls take ---------------------------------------------------------------------------------------------
    def downsample_jobs(self, lv):
        return [(self.view(who, lv - 1, k), self(who, lv, k), self.g["ext"]) for who in self.WHO for k in range(3)]

    def hbm_chains(self):
        g = self.g
        hs, vs = g["shifts"]
        out = []
        for r in (0, 1):
            levels = [([self.view("frame", lv, k) for k in range(3)], [self.view("ref%d" % r, lv, k) for k in range(3)], g["ext"])
                      for lv in range(P.CHAIN_PYRAMID + 1)]
            out.append((levels, hs, vs, g["blocks"], r, [self("hbm", r, lv) for lv in range(P.CHAIN_PYRAMID + 1)]))
        return out

    def upsample_pairs(self):
        return [(self.view("ref%d" % r, 0, k), self.hp[r][k]) for r in (0, 1) for k in range(3)]

    def subpel_chains(self):
        g = self.g
        return [(self.view("frame", 0, 0), self.hp[r][0], g["ext"], g["blocks"], g["prec"], r, g["lam"], self("hbm", r, 0), self("subpel", r))
                for r in (0, 1)]

    def mode_picture(self):
        g = self.g
        return ([self.view("frame", 0, k) for k in range(3)], self.hp, g["shifts"], g["ext"], g["mode_params"], g["lam"],
                [self("subpel", r) for r in (0, 1)], [self("hbm", r, 1) for r in (0, 1)], [self("hbm", r, 2) for r in (0, 1)],
                self("motion"), self("superblocks"), self("trials"), self("stats"))

    def obmc_planes(self):
        return [sa.obmc_plane(self("motion"), self.g["motion_params"], k, self.hp[0][k], self.hp[1][k], None, self("prediction", k), prediction_only=2)
                for k in range(3)]

    def quant_planes(self):
        out = []
        for k in range(3):
            co, qu = self("reconstruction", k), self("quantised", k)
            a = _lib.QuantPlane()
            a.coeffs, a.quant, a.bytes = co.ptr, qu.ptr, co.spec.extent
            a.codeblocks, a.ncodeblocks, a.is_intra, a.summary = self.tables[k], len(self.tables[k]), 0, self("summaries", k).ptr
            out.append(a)
        return out

    def noarith_picture(self):
        g = self.g
        return ([self("quantised", k) for k in range(3)], self.tables, P.CHAIN_DEPTH, g["hc"], g["vc"], g["mode"], self("bytes"), self.capacity,
                self("result"))

    # -- after the synchronize -------------------------------------------------------------------------------------------
    def check(self):
        e, g, s, ext = self.e, self.g, self.s, self.g["ext"]
        want = {}
        pyramids = dict(frame=e["frame_pyramid"], ref0=e["ref_pyramids"][0], ref1=e["ref_pyramids"][1])
        for who in self.WHO:
            for lv in range(1, P.CHAIN_PYRAMID + 1):
                for k in range(3):
                    want[s[who, lv, k]] = A.edgeextend(pyramids[who][lv][k], ext)
        for r in (0, 1):
            for lv in range(P.CHAIN_PYRAMID + 1):
                want[s["hbm", r, lv]] = as_bytes(e["hbm"][r][lv])
            want[s["subpel", r]] = as_bytes(e["subpel"][r])
        for key, a in zip(("motion", "superblocks", "trials", "stats"), e["mode"]):
            want[s[key,]] = as_bytes(a)
        for k in range(3):
            q, r, summ = e["quantise"][k]
            want[s["prediction", k]], want[s["residual", k]], want[s["coefficients", k]] = e["prediction"][k], e["residual"][k], e["coefficients"][k]
            want[s["reconstruction", k]], want[s["quantised", k]], want[s["summaries", k]] = r, q, summ
        data, bits, stats = e["bytes"]
        raw = self.blk.raw()
        out = s["bytes",]
        tail = self.blk.before[out.offset + len(data):out.offset + out.extent]          # (the canary behind the bytes)
        want[out] = np.concatenate([np.frombuffer(data, np.uint8), tail]).reshape(1, -1)
        # every stage in the order of the chain, so that the first one that differs is the first one named
        mism, strays = G.find_changes(self.lay, self.blk.before, raw, want)
        G.report(["%s: %s" % (self.name, m) for m in mism], ["%s: %s" % (self.name, m) for m in strays])
        result = sa.noarith_result(s["result",].payload(raw))
        assert result["bytes"] == len(data) and result["overrun"] == 0, (self.name, result["bytes"], len(data))
        assert np.array_equal(result["subband_bits"], bits), self.name
        assert result["false_zero"] == (stats["false_zero_codeblocks"], stats["false_zero_subbands"]), self.name
        # the bytes, decoded by the restated decoder and dequantised, give the reconstruction back
        got = out.payload(raw)[0, :len(data)]
        dec_q, dec_r, used = P.chain_decoded(g, got.tobytes())
        assert used == len(data)
        for k in range(3):
            same(dec_q[k], s["quantised", k].payload(raw), (self.name, "decoded quantised values", k))
            same(dec_r[k], s["reconstruction", k].payload(raw), (self.name, "decoded and dequantised", k))

    def free(self):
        self.blk.free()
        for r in self.hp:
            for p in r:
                p.free()


def chain_front(ctx, pics):
    """Steps 1 to 5 for the pictures of one batch: the pyramids, the block matching, the half-pel images, the sub-pel
    refinement, the mode decision -- they read original pictures only."""
    for lv in range(1, P.CHAIN_PYRAMID + 1):
        ctx.downsample_batch([job for p in pics for job in p.downsample_jobs(lv)])
    ctx.hbm_batch([c for p in pics for c in p.hbm_chains()], True)
    ctx.upsample_batch([pair for p in pics for pair in p.upsample_pairs()])
    ctx.subpel_batch([c for p in pics for c in p.subpel_chains()])
    ctx.mode_decision_batch([p.mode_picture() for p in pics])


def chain_back(ctx, pics):
    """Steps 6 to 10: the prediction of `motion`, the residual, its transform (twice: the quantiser overwrites its input
    with the reconstruction), the quantiser, the noarith bytes."""
    ctx.obmc_batch([pl for p in pics for pl in p.obmc_planes()])
    ctx.subtract_batch([(p("residual", k), p("prediction", k)) for p in pics for k in range(3)])
    ctx.iwt_batch([(p("residual", k), p(stage, k)) for p in pics for k in range(3) for stage in ("coefficients", "reconstruction")],
                  P.CHAIN_DEPTH, P.CHAIN_FILT)
    planes = [a for p in pics for a in p.quant_planes()]
    sa.check(ctx.lib.schro_hip_quantise_batch(ctx.h, (_lib.QuantPlane * len(planes))(*planes), len(planes), 2))
    assert ctx.noarith_encode_batch([p.noarith_picture() for p in pics]) is None


def run_chain(batches, pipelined):
    """The chain over `batches` of picture names on a context of its own, stage completion off, one synchronize at the end.
    Not pipelined: everything on queue 0.  Pipelined: steps 1 to 5 of batch k + 1 on queue 1 while queue 0 runs steps 6 to
    10 of batch k, mark k % 16 recorded behind step 5 and waited for in front of step 6."""
    ctx = sa.Context(0)
    try:
        pics = [[ChainPicture(ctx, name, seed=10 * b + n) for n, name in enumerate(names)] for b, names in enumerate(batches)]
        ballast = Ballast(ctx)
        try:
            ctx.synchronize()
            sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 0))
            front, back = (1, 0) if pipelined else (0, 0)

            def enqueue_front(k):
                ctx.select_queue(front)
                chain_front(ctx, pics[k])
                if pipelined:
                    ctx.queue_mark(k % 16)

            def enqueue_back(k):
                ctx.select_queue(back)
                if pipelined:
                    ctx.queue_wait_mark(k % 16)
                chain_back(ctx, pics[k])

            enqueue_front(0)
            for k in range(len(pics)):
                if k + 1 < len(pics):
                    enqueue_front(k + 1)
                enqueue_back(k)
                if k == 0:
                    ballast.enqueue(sorted({front, back}))      # (the later batches pile up behind it)
            ctx.select_queue(0)
            sa.check(ctx.lib.schro_hip_context_set_stage_completion(ctx.h, 1))
            ctx.synchronize()
            for batch in pics:
                for p in batch:
                    p.check()
        finally:
            for batch in pics:
                for p in batch:
                    p.free()
            ballast.free()
    finally:
        ctx.close()


def test_inter_chain_without_a_wait():
    """Two pictures of unlike geometry in every batch call, original pictures in and stream bytes out on one queue: every
    intermediate equals what the restatements chained give, and the bytes decode to the reconstruction."""
    run_chain([P.CHAIN_PAIR], pipelined=False)


def test_inter_chain_pipelined():
    """Three pictures deep over two queues; the middle picture has the larger grid, so both queues' scratch grows
    mid-pipeline and the third picture's tables lie on the second's leftovers."""
    grids = [P.records(P.chain_geometry(n)) for n in P.CHAIN_PIPELINE]
    assert grids[1] > grids[0] and grids[2] < grids[1]
    run_chain([(name,) for name in P.CHAIN_PIPELINE], pipelined=True)
