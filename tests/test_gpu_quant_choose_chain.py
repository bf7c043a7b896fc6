"""GPU: histograms -> quantiser choice -> quantiser -> VLC transform data as one run of enqueued calls
(schro_hip_histogram_batch, schro_hip_quant_choose_batch, schro_hip_quantise_chosen_batch,
schro_hip_noarith_encode_chosen_batch) on a context of its own, nothing waited for in between: the quant indices never
leave the device.  Bytes, quant planes, reconstruction, summaries and result words are compared with tests/hist_ref.py ->
tests/quant_choose_ref.py -> tests/quant_ref.py -> tests/noarith_enc_ref.py, and with the host-record entry points
(schro_hip_quantise_batch, schro_hip_noarith_encode_batch) fed the same indices."""
import ctypes as C
import functools

import numpy as np
import pytest

import hist_ref as H
import noarith_enc_cases as NC
import noarith_enc_ref as NR
import quant_choose_draws as D
import quant_choose_ref as R
import quant_ref as Q
import schroedinger_amd as sa
from schroedinger_amd import _lib

pytestmark = pytest.mark.gpu

QI_OFFSET = sa.QUANT_CHOICE_DTYPE.fields["quant_index"][1]
ROW = sa.QUANT_CHOICE_DTYPE.itemsize
NBMAX = R.MAX_BANDS

# name: luma size, chroma shifts (h, v), depth, dtype, intra, codeblock counts per level, engine, target
SPECS = {
    "420_d2": dict(size=(64, 48), chroma=(1, 1), depth=2, dtype=np.int16, intra=True, hc=[1, 2, 3], vc=[1, 1, 2], engine=D.B,
                   target=("between", 1.0, 100.0), seed=21),
    "444_d3_s32": dict(size=(40, 24), chroma=(0, 0), depth=3, dtype=np.int32, intra=False, hc=[1, 1, 2, 2], vc=[1, 1, 1, 2], engine=D.E,
                       target=("between", 0.01, 1.0), seed=22),
    "444_d1": dict(size=(32, 32), chroma=(0, 0), depth=1, dtype=np.int16, intra=False, hc=[2, 2], vc=[2, 2], engine=D.L,
                   target=("abs", 0.4), seed=23),
    "420_d3": dict(size=(48, 32), chroma=(1, 1), depth=3, dtype=np.int16, intra=True, hc=[1, 1, 2, 3], vc=[1, 1, 2, 2], engine=D.E,
                   target=("between", 1.0, 0.01), seed=24),
}
MODE = 1


def subband_of_records(depth, hc, vc):
    out = []
    for i in range(1 + 3 * depth):
        nh, nv = NR.codeblock_counts(i, hc, vc)
        out += [i] * (nh * nv)
    return out


@functools.lru_cache(maxsize=None)
def picture(name):
    """the coefficient planes of a drawn picture and everything the references make of them"""
    s = SPECS[name]
    rng = np.random.default_rng(s["seed"])
    depth, dtype = s["depth"], np.dtype(s["dtype"])
    w, h = s["size"]
    sizes = [(w, h), (w >> s["chroma"][0], h >> s["chroma"][1]), (w >> s["chroma"][0], h >> s["chroma"][1])]
    planes = []
    for c, (pw, ph) in enumerate(sizes):
        p = np.zeros((ph, pw), dtype)
        for i in range(1 + 3 * depth):
            level = H.position(i) >> 2
            scale = rng.uniform(2.0, 12.0) * 2.0 ** (depth - level + (2 if i == 0 else 0))
            v = NR.subband(p, depth, i)
            v[...] = np.rint(rng.laplace(0.0, scale, v.shape)).clip(-3000, 3000).astype(dtype)
        planes.append(p)
    nb = 1 + 3 * depth
    skips = [H.band_skip(i) for i in range(nb)]
    counts = [np.array([H.counts(H.band_view(p, depth, i), skips[i], dc=s["intra"] and i == 0) for i in range(nb)], np.uint32)
              for p in planes]
    prng = np.random.default_rng(s["seed"] + 100)
    weight = np.ones(NBMAX)
    weight[:nb] = prng.uniform(0.5, 2.5, nb)
    ratio = np.ones((3, NBMAX))
    ratio[:, :nb] = prng.uniform(0.8, 1.2, (3, nb))
    bins = [[R.scaled_bins(counts[c][i], skips[i]) for i in range(nb)] for c in range(3)]
    ent, err = R.calc_estimates(bins, depth, True, ratio, D.error_table())
    engine = s["engine"]
    if s["target"][0] == "abs":
        target = float(s["target"][1])
    else:
        ev = R.Evaluator(ent, err, depth, weight, D.SCALES)
        f = ev.lambda_to_error if engine == D.E else ev.lambda_to_entropy
        target = 0.5 * (f(s["target"][1]) + f(s["target"][2]))
    trace = []
    choice = R.choose(ent, err, depth, weight, D.SCALES, engine, target, trace)
    D.check_trace(trace, name)          # the draw keeps clear of ties, as every case of the stage's own tests does
    qi = choice["quant_index"]
    sub = subband_of_records(depth, s["hc"], s["vc"])
    isz = dtype.itemsize
    want = dict(quant=[], recon=[], summary=[])
    records = []
    dc = []
    for c, p in enumerate(planes):
        recs = NC.layout_records(p.shape[1], p.shape[0], depth, s["hc"], s["vc"], p.shape[1] * isz, isz)
        records.append(recs)
        ndc = s["hc"][0] * s["vc"][0] if s["intra"] else 0
        dc.append((ndc, p.shape[1] >> depth, p.shape[0] >> depth) if ndc else (0, 0, 0))
        q, r, summ = Q.quantise_plane(p, [tuple(rec[:4]) + (int(qi[c][sub[n]]),) for n, rec in enumerate(recs)], s["intra"], ndc,
                                      (p.shape[1] >> depth, p.shape[0] >> depth) if ndc else None)
        want["quant"].append(q)
        want["recon"].append(r)
        want["summary"].append(np.array(summ, np.uint32))
    data, bits, stats = NR.encode_transform_data(want["quant"], depth, s["hc"], s["vc"], MODE, qi)
    want.update(bytes=np.frombuffer(data, np.uint8), subband_bits=bits, false_zero=(stats["false_zero_codeblocks"], stats["false_zero_subbands"]))
    return dict(spec=s, planes=planes, sizes=sizes, skips=skips, counts=counts, weight=weight, ratio=ratio, target=target, choice=choice,
                records=records, sub=sub, dc=dc, want=want)


class Chain:
    """the device side of a list of pictures (one sample depth): buffers made and filled up front, then the four calls"""

    def __init__(self, ctx, names):
        self.ctx, self.names = ctx, names
        self.pics = [picture(n) for n in names]
        self.bpp = np.dtype(self.pics[0]["spec"]["dtype"]).itemsize
        self.coeffs, self.quant, self.out, self.res = [], [], [], []
        words = C.sizeof(_lib.NoarithResult) // 4
        for p in self.pics:
            dt = p["planes"][0].dtype
            self.coeffs.append([ctx.plane(a.shape[0], a.shape[1], dt, stride=a.shape[1] * dt.itemsize).upload(a) for a in p["planes"]])
            self.quant.append([ctx.plane(a.shape[0], a.shape[1], dt, stride=a.shape[1] * dt.itemsize).fill(0x5a) for a in p["planes"]])
            cap = sa.noarith_encode_bound(p["sizes"], p["spec"]["depth"], p["spec"]["hc"], p["spec"]["vc"], self.bpp)
            self.out.append((ctx.plane(1, cap, np.uint8), cap))
            self.res.append(ctx.plane(1, words, np.uint32))
        self.clamped = ctx.plane(1, 2, np.uint32).fill(0)

    def hist_jobs(self):
        jobs = []
        for p, co in zip(self.pics, self.coeffs):
            d, intra = p["spec"]["depth"], p["spec"]["intra"]
            for c, pl in enumerate(co):
                jobs.append((pl, [H.band_rect(pl.width, pl.height, d, i, pl.stride, self.bpp) + (p["skips"][i], int(intra and i == 0))
                                  for i in range(1 + 3 * d)]))
        return jobs

    def tables(self, chosen_form, indices=None):
        """per picture and component the records with quant_index = the sub-band (chosen form) or its index"""
        out = []
        for n, p in enumerate(self.pics):
            qi = indices[n] if indices is not None else p["choice"]["quant_index"]
            out.append([[tuple(rec[:6]) + (p["sub"][k] if chosen_form else int(qi[c][p["sub"][k]]),) for k, rec in enumerate(recs)]
                        for c, recs in enumerate(p["records"])])
        return out

    def quant_jobs(self, tabs):
        return [(self.coeffs[n][c], self.quant[n][c], tabs[n][c], p["spec"]["intra"], p["dc"][c])
                for n, p in enumerate(self.pics) for c in range(3)]

    def noarith_pictures(self, tabs):
        return [(self.quant[n], tabs[n], p["spec"]["depth"], p["spec"]["hc"], p["spec"]["vc"], MODE, self.out[n][0], self.out[n][1], self.res[n])
                for n, p in enumerate(self.pics)]

    def run_chained(self, chosen=None):
        """the four calls, enqueued; chosen: a device table of the caller's instead of the choice's"""
        ctx = self.ctx
        arr, counts, self.block = ctx.histogram_planes(self.hist_jobs())
        sa.check(ctx.lib.schro_hip_histogram_batch(ctx.h, arr, len(arr), self.bpp))
        specs = [dict(counts=counts[3 * n:3 * n + 3], skip=p["skips"], depth=p["spec"]["depth"], is_intra=int(p["spec"]["intra"]), is_noarith=1,
                      engine=p["spec"]["engine"], weight=p["weight"], ratio=p["ratio"], scales=D.SCALES, target=p["target"])
                 for n, p in enumerate(self.pics)]
        self.choice = ctx.quant_choose_batch(specs)
        base = [(chosen.ptr + n * 4 * 3 * NBMAX) if chosen is not None else (self.choice.ptr + n * ROW + QI_OFFSET) for n in range(len(self.pics))]
        tabs = self.tables(True)
        self.summaries = ctx.quantise_chosen_batch(self.quant_jobs(tabs), [base[n] + 4 * NBMAX * c for n in range(len(self.pics)) for c in range(3)],
                                                   self.clamped.ptr)
        assert ctx.noarith_encode_chosen_batch(self.noarith_pictures(tabs), base, self.clamped.ptr + 4) is None

    def run_host_records(self, indices=None):
        """the same pictures through the entry points that take the indices in host records"""
        for n, p in enumerate(self.pics):
            for c, a in enumerate(p["planes"]):
                self.coeffs[n][c].upload(a)
                self.quant[n][c].fill(0x5a)
        tabs = self.tables(False, indices)
        self.summaries = self.ctx.quantise_batch(self.quant_jobs(tabs))
        assert self.ctx.noarith_encode_batch(self.noarith_pictures(tabs)) is None

    def outputs(self):
        self.ctx.synchronize()
        got = []
        for n, p in enumerate(self.pics):
            r = sa.noarith_result(self.res[n].download())
            got.append(dict(quant=[q.download() for q in self.quant[n]], recon=[c.download() for c in self.coeffs[n]],
                            summary=[self.summaries[3 * n + c].download() for c in range(3)],
                            bytes=self.out[n][0].download()[0, :r["bytes"]].copy(), result=r))
        return got

    def free(self):
        for group in self.coeffs + self.quant:
            for pl in group:
                pl.free()
        for (o, _), r in zip(self.out, self.res):
            o.free()
            r.free()
        self.clamped.free()


def same(got, want):
    for c in range(3):
        assert np.array_equal(got["quant"][c], want["quant"][c]), c
        assert np.array_equal(got["recon"][c], want["recon"][c]), c
        assert np.array_equal(got["summary"][c], want["summary"][c]), c
    assert got["bytes"].tobytes() == want["bytes"].tobytes()
    if "result" in want:
        assert got["result"]["bytes"] == want["result"]["bytes"] and got["result"]["overrun"] == 0
        assert np.array_equal(got["result"]["subband_bits"], want["result"]["subband_bits"])
        assert got["result"]["false_zero"] == want["result"]["false_zero"]
    else:
        assert got["result"]["bytes"] == len(want["bytes"]) and got["result"]["overrun"] == 0
        assert np.array_equal(got["result"]["subband_bits"], want["subband_bits"])
        assert got["result"]["false_zero"] == tuple(want["false_zero"])


@pytest.fixture(scope="module")
def own():
    """a context of its own, the tables in place"""
    if sa.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    c = sa.Context(0)
    c.quant_choose_tables(D.error_table())
    yield c
    c.close()


def check_chain(ctx, names):
    ch = Chain(ctx, names)
    try:
        ch.run_chained()
        got = ch.outputs()
        rows = ch.choice.download().view(sa.QUANT_CHOICE_DTYPE).reshape(-1)
        assert ch.clamped.download().tolist() == [[0, 0]]
        for n, p in enumerate(ch.pics):
            nb = 1 + 3 * p["spec"]["depth"]
            assert np.array_equal(rows[n]["quant_index"][:, :nb], p["choice"]["quant_index"])
            assert int(rows[n]["evaluations"]) == p["choice"]["evaluations"]
            same(got[n], p["want"])
        ch.block.free()
        ch.choice.free()
        ch.run_host_records()
        again = ch.outputs()
        for n in range(len(names)):
            same(again[n], got[n])
    finally:
        ch.free()


@pytest.mark.parametrize("names", [("420_d2",), ("444_d3_s32",), ("420_d2", "444_d1", "420_d3")], ids=lambda n: "+".join(n))
def test_chain(own, names):
    check_chain(own, list(names))


def test_clamp(own):
    """a table of the caller's own with 61 and -1 in it: clamped to 60 and 0, and counted -- per record by the quantiser,
    per sub-band by the VLC encoder"""
    ch = Chain(own, ["420_d2"])
    try:
        p = ch.pics[0]
        table = np.zeros((3, NBMAX), np.int32)
        table[:, :7] = [[61, -1, 5, 9, 0, 60, 1000], [3, 3, -7, 8, 8, 2, 1], [4, 4, 4, 4, 4, 4, 4]]
        clipped = table.clip(0, 60)
        dev = own.plane(1, 3 * NBMAX, np.int32).upload(table.reshape(1, -1))
        ch.run_chained(chosen=dev)
        got = ch.outputs()
        out_of_range = (table[:, :7] != clipped[:, :7])
        per_band = [sum(1 for s in p["sub"] if s == i) for i in range(7)]
        assert ch.clamped.download().tolist() == [[int(sum(per_band[i] for c in range(3) for i in range(7) if out_of_range[c, i])),
                                                    int(out_of_range.sum())]]
        ch.block.free()
        ch.choice.free()
        ch.run_host_records([clipped])
        same(ch.outputs()[0], got[0])
        dev.free()
    finally:
        ch.free()


def test_scratch_sequence(own):
    """the queue's grow-only scratch through small, larger, small"""
    for names in (["444_d1"], ["420_d2", "444_d1", "420_d3"], ["444_d1"]):
        check_chain(own, names)


@pytest.mark.parametrize("name", ["420_d2", "444_d3_s32", "444_d1"])
def test_frame_layer(own, name):
    """schro_encoder_choose_quantisers_hip on a device frame: the record on the host, what the restatement chooses"""
    from schroedinger_amd import frames
    p = picture(name)
    s = p["spec"]
    (w, h), (hs, vs) = s["size"], s["chroma"]
    iwt = frames.DeviceFrame(own, frames.frame_format(np.dtype(s["dtype"]), hs, vs), w, h).upload(frames.HostFrame(p["planes"], hs, vs))
    try:
        params = frames.make_params(transform_depth=s["depth"], num_refs=0 if s["intra"] else 1, iwt_luma_width=w, iwt_luma_height=h,
                                    iwt_chroma_width=p["sizes"][1][0], iwt_chroma_height=p["sizes"][1][1])
        for _ in range(2):              # (the second call finds the context's table and record in place)
            got = own.choose_quantisers(iwt, params, 1, s["engine"], p["target"], p["weight"], p["ratio"], D.SCALES)
            want, nb = p["choice"], 1 + 3 * s["depth"]
            assert np.array_equal(got["quant_index"][:, :nb], want["quant_index"]) and not got["quant_index"][:, nb:].any()
            assert int(got["evaluations"]) == want["evaluations"] and int(got["not_bracketed"]) == 0
            assert np.float64(got["frame_lambda"]).tobytes() == np.float64(want["frame_lambda"]).tobytes()
            assert np.array_equal(got["chosen_error"][:, :nb], want["chosen_error"])
            assert np.allclose(got["chosen_entropy"][:, :nb], want["chosen_entropy"], rtol=1e-9, atol=0)
            assert R.estimated_residual_bits(got["chosen_entropy"][:, :nb]) >= 0
        with pytest.raises(sa.SchroHipError, match="picture 0: engine 7 is unknown"):
            own.choose_quantisers(iwt, params, 1, 7, p["target"], p["weight"], p["ratio"], D.SCALES)
    finally:
        iwt.unref()


def test_chosen_refusals(own):
    ch = Chain(own, ["444_d1"])
    try:
        tabs = ch.tables(True)
        row = own.plane(1, 3 * NBMAX, np.int32).fill(0)
        with pytest.raises(sa.SchroHipError, match="plane 1: chosen is NULL or not 4-byte aligned"):
            own.quantise_chosen_batch(ch.quant_jobs(tabs), [row.ptr, row.ptr + 2, row.ptr], ch.clamped.ptr)
        with pytest.raises(sa.SchroHipError, match="clamped is NULL or not 4-byte aligned"):
            own.quantise_chosen_batch(ch.quant_jobs(tabs), [row.ptr] * 3, None)
        bad = [[list(r) for r in t] for t in tabs[0]]
        bad[2][1][6] = 19
        with pytest.raises(sa.SchroHipError, match="plane 2 codeblock 1: quant_index 19 is no sub-band"):
            own.quantise_chosen_batch(ch.quant_jobs([bad]), [row.ptr] * 3, ch.clamped.ptr)
        bad[2][1][6] = 3
        with pytest.raises(sa.SchroHipError, match="picture 0, component 2, sub-band 0, record 1: quant_index 3 is not the sub-band"):
            sa.noarith_encode_chosen_check(ch.noarith_pictures([bad]), [row.ptr], ch.clamped.ptr, ch.bpp)
        with pytest.raises(sa.SchroHipError, match="picture 0: chosen is NULL or not 4-byte aligned"):
            sa.noarith_encode_chosen_check(ch.noarith_pictures(tabs), [row.ptr + 1], ch.clamped.ptr, ch.bpp)
        sa.noarith_encode_chosen_check(ch.noarith_pictures(tabs), [row.ptr], ch.clamped.ptr, ch.bpp)
        row.free()
    finally:
        ch.free()
