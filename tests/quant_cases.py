"""Shared by tests/test_gpu_quantise.py, tests/test_quantise_api.py, tests/dry_run_quant_cases.py and
tests/encode_loop_draws.py: codeblock layouts as records, the decoder's tight hand-over of a quant plane (tight_values),
the planes of the geometry and DC cases, the runner that compares a schro_hip_quantise_batch call with tests/quant_ref.py
bit for bit, and the refusal cases."""
import ctypes as C

import numpy as np

import quant_ref as Q
from schroedinger_amd import _lib

EINVAL = -1
QUANT_FILL = 0x5a               # what the quant planes hold before a call


def layout(width, height, depth, hc, vc, stride, itemsize):
    """schro_hip_codeblock_layout as a list of [dst_offset, dst_stride, width, height, quant_index = 0] (host only)."""
    lib = _lib.load()
    a, b = (C.c_int * (depth + 1))(*hc), (C.c_int * (depth + 1))(*vc)
    n = lib.schro_hip_codeblock_layout(width, height, depth, a, b, stride, itemsize, None, 0)
    assert n > 0, lib.schro_hip_last_error()
    tab = (_lib.Codeblock * n)()
    assert lib.schro_hip_codeblock_layout(width, height, depth, a, b, stride, itemsize, tab, n) == n
    return [[t.dst_offset, t.dst_stride, t.width, t.height, 0] for t in tab]


def table(records):
    tab = (_lib.Codeblock * len(records))()
    for t, (off, stride, w, h, qi) in zip(tab, records):
        t.dst_offset, t.dst_stride, t.width, t.height, t.src_offset, t.src_bytes, t.quant_index = off, stride, w, h, -1, 0, qi
    return tab


def values(rng, shape, dtype, small_every=3):
    """coefficients: mostly small, some over the whole range the type's contract allows (s32: within +-2^27)"""
    big = 32768 if np.dtype(dtype) == np.int16 else 1 << 27
    v = rng.integers(-big, big, shape)
    small = rng.integers(-300, 301, shape)
    return np.where(rng.integers(0, small_every, shape) == 0, v, small).astype(dtype)


def record_mask(shape, records, itemsize):
    m = np.zeros(shape[0] * shape[1], bool)
    for rec in records:
        m[Q._cells(rec, itemsize, m.size)] = True
    return m.reshape(shape)


def tight_values(quant, records, itemsize):
    """the quant plane's codeblocks as the decoder's hand-over: row-major, tight, `itemsize` bytes each"""
    flat, blobs, recs, off = quant.reshape(-1), [], [], 0
    for (o, st, w, h, qi) in records:
        v = flat[Q._cells((o, st, w, h), quant.dtype.itemsize, flat.size)].astype({2: np.int16, 4: np.int32}[itemsize])
        blobs.append(v.reshape(-1))
        recs.append((o, st, w, h, off, itemsize, qi))
        off += v.size * itemsize
    return np.concatenate(blobs).view(np.uint8), recs


def geometry_specs(dtype, seed):
    """The planes of the codeblock-geometry case for one sample type."""
    rng = np.random.default_rng(seed)
    b = np.dtype(dtype).itemsize
    specs = []
    # 3 levels, 3 x 2 codeblocks on the finest, 1 x 1 coarser: unequal widths (44 = 14 + 15 + 15), odd starts, and a pitch
    # of an odd number of samples, so that rows are not 4-byte aligned (s16)
    for (w, h, pitch) in ((88, 72, 89), (44, 40, 47)):
        recs = layout(w, h, 3, [1, 1, 1, 3], [1, 1, 1, 2], pitch * b, b)
        for n, r in enumerate(recs):
            r[4] = (7 * n + 3) % 61             # a distinct index per codeblock, every form among them
        assert len(set(r[4] for r in recs)) == len(recs)
        for intra in (0, 1):
            specs.append(dict(buf=values(rng, (h, pitch), dtype), records=recs, intra=intra))
    # one plane of one 1 x 1 codeblock
    specs.append(dict(buf=np.array([[-77]], dtype), records=[[0, b, 1, 1, 9]], intra=0))
    # a codeblock whose values all quantise to zero beside one with a single non-zero value, in its last sample
    buf = rng.integers(-3, 4, (20, 50)).astype(dtype)
    buf[19, 49] = 4000
    specs.append(dict(buf=buf, records=[[0, 50 * b, 25, 20, 30], [25 * b, 50 * b, 25, 20, 30]], intra=1))
    # the case is what it says: the checker finds nothing in the first codeblock, one value in the second, in its last sample
    q, _, summ = Q.quantise_plane(buf, specs[-1]["records"], 1)
    assert summ[0] == (0, 0) and summ[1][0] == 1 and summ[1][1] == abs(int(q[19, 49])) > 0
    return specs


def split(w, h, pitch_bytes, itemsize, indices):
    """a band cut into min (2, w) x min (2, h) codeblocks of unlike indices"""
    xs = [0, w] if w < 2 else [0, w // 2, w]
    ys = [0, h] if h < 2 else [0, (h + 1) // 2, h]
    recs = []
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            recs.append([ys[j] * pitch_bytes + xs[i] * itemsize, pitch_bytes, xs[i + 1] - xs[i], ys[j + 1] - ys[j],
                         indices[len(recs) % len(indices)]])
    return recs


def dc_specs(dtype, seed, threads):
    """The intra LL bands: 1 x 1, 1 x 9, 9 x 1, 7 x 5, 65 x 64 (diagonals longer than a wave) and one whose shorter side is
    the DC kernel's workgroup size + 1 (the strided diagonal); width x height."""
    rng = np.random.default_rng(seed)
    b = np.dtype(dtype).itemsize
    specs = []
    for n, (w, h) in enumerate(((1, 1), (1, 9), (9, 1), (7, 5), (65, 64), (threads + 9, threads + 1))):
        pitch = w + 3
        if np.dtype(dtype) == np.int16:
            # values whose reconstruction + prediction leaves 16 bits: the s16 stores truncate
            buf = np.where(rng.integers(0, 4, (h, pitch)) == 0, rng.integers(-32768, 32768, (h, pitch)),
                           rng.integers(-2000, 2001, (h, pitch))).astype(dtype)
        else:
            buf = rng.integers(-(1 << 20), 1 << 20, (h, pitch)).astype(dtype)
        recs = split(w, h, pitch * b, b, [(5 + 11 * n) % 61, (18 + 7 * n) % 61, (3 + 13 * n) % 61, (40 + 5 * n) % 61])
        specs.append(dict(buf=buf, records=recs, intra=1, dc=(len(recs), w, h)))
    return specs


def expected(spec):
    """(quant, recon, summaries) of a spec by tests/quant_ref.py; quant holds QUANT_FILL bytes outside the records"""
    buf = spec["buf"]
    dc = spec.get("dc")
    q, r, s = Q.quantise_plane(buf, spec["records"], spec["intra"], dc[0] if dc else 0, dc[1:] if dc else None)
    fill = np.frombuffer(bytes([QUANT_FILL]) * buf.dtype.itemsize, buf.dtype)[0]
    q = np.where(record_mask(buf.shape, spec["records"], buf.dtype.itemsize), q, fill)
    return q, r, np.array(s, np.uint32).reshape(-1, 2)


def run_specs(ctx, specs):
    """One schro_hip_quantise_batch call over all specs, compared with the checker: quantised values, reconstruction,
    summaries.  Returns the downloaded (quant, recon) pairs."""
    jobs, keep = [], []
    for s in specs:
        buf = s["buf"]
        co = ctx.upload(buf, stride=buf.shape[1] * buf.dtype.itemsize)
        qu = ctx.plane(buf.shape[0], buf.shape[1], buf.dtype, stride=co.stride).fill(QUANT_FILL)
        jobs.append((co, qu, table(s["records"]), s["intra"], s.get("dc")))
        keep += [co, qu]
    summaries = ctx.quantise_batch(jobs)
    out = []
    for n, (s, job, summ) in enumerate(zip(specs, jobs, summaries)):
        want_q, want_r, want_s = expected(s)
        got_q, got_r, got_s = job[1].download(), job[0].download(), summ.download()
        assert np.array_equal(got_q, want_q), ("quantised values", n, np.argwhere(got_q != want_q)[:4])
        assert np.array_equal(got_r, want_r), ("reconstruction", n, np.argwhere(got_r != want_r)[:4])
        assert np.array_equal(got_s, want_s), ("summaries", n, got_s.tolist(), want_s.tolist())
        out.append((got_q, got_r))
    for p in keep + summaries:
        p.free()
    return out


REFUSAL_PLANE = (16, 32)        # rows x samples of the s16 planes the refusal cases describe
# the subtract call's refusal over the same planes: (dst_stride, width, height), a destination stride shorter than its row
SUBTRACT_REFUSAL = (20, 16, 16)


def refusal_table(stride):
    """(good records, cases) for planes of REFUSAL_PLANE samples and `stride` bytes a row: name -> (the bad plane's records
    and members, the words its message holds).  `quant_offset`: the quant plane lies that many bytes behind the coefficients'
    first.  Read by refusal_cases below and by tests/encoder_walk_cases.py."""
    good = [[0, stride, 16, 16, 5], [32, stride, 16, 16, 6]]

    def rec(**kw):
        r = dict(off=0, stride=stride, w=16, h=16, qi=5)
        r.update(kw)
        return [good[0], [r["off"], r["stride"], r["w"], r["h"], r["qi"]]]

    cases = {
        "quant index above 60": (dict(records=rec(qi=61)), ("plane 1", "codeblock 1", "quant_index 61")),
        "bad sample size": (dict(records=good, bps=3), ("bytes_per_sample",)),
        "zero width": (dict(records=rec(w=0)), ("plane 1", "codeblock 1")),
        "negative height": (dict(records=rec(h=-4)), ("plane 1", "codeblock 1")),
        "stride shorter than a row": (dict(records=rec(stride=30)), ("plane 1", "codeblock 1", "stride")),
        "stride not a multiple of the sample": (dict(records=rec(stride=stride + 1)), ("plane 1", "codeblock 1", "stride")),
        "quant overlapping coeffs": (dict(records=good, quant_offset=64), ("plane 1", "overlaps")),
        "record past the plane": (dict(records=rec(off=stride * 8)), ("plane 1", "codeblock 1", "outside")),
        "record starting in front of the plane": (dict(records=rec(off=-2)), ("plane 1", "codeblock 1", "outside")),
        "DC records that do not tile the band": (dict(records=good, dc_predict_first=1, dc_width=32, dc_height=16),
                                                 ("plane 1", "DC band")),
        "DC record outside the band": (dict(records=good, dc_predict_first=2, dc_width=16, dc_height=16),
                                       ("plane 1", "codeblock 1", "DC band")),
        "no records": (dict(records=good, ncodeblocks=0), ("plane 1",)),
    }
    return good, cases


def refusal_cases(ctx):
    """Every refusal of schro_hip_quantise_batch: SCHRO_HIP_EINVAL, nothing launched, the message naming plane and record.
    The planes are real allocations of the context (a call that wrongly went through would only touch them)."""
    lib = ctx.lib
    co, qu = ctx.plane(*REFUSAL_PLANE, np.int16), ctx.plane(*REFUSAL_PLANE, np.int16)
    summ = ctx.plane(4, 2, np.uint32, stride=8)
    good, cases = refusal_table(co.stride)

    def call(records, bps=2, plane=1, quant_offset=None, **kw):
        """the bad plane is plane `plane` of the call, behind good ones"""
        if quant_offset is not None:
            kw["quant"] = co.ptr + quant_offset
        arr = (_lib.QuantPlane * (plane + 1))()
        keep = []
        for k in range(plane + 1):
            tab = table(records if k == plane else good)
            keep.append(tab)
            a = arr[k]
            a.coeffs, a.quant, a.bytes, a.codeblocks, a.ncodeblocks = co.ptr, qu.ptr, co.stride * co.height, tab, len(tab)
            a.is_intra, a.summary = 0, summ.ptr
            if k == plane:
                for name, v in kw.items():
                    setattr(a, name, v)
        rc = lib.schro_hip_quantise_batch(ctx.h, arr, plane + 1, bps)
        msg = lib.schro_hip_last_error()
        return rc, (msg.decode() if msg else "")

    for name, (kw, words) in cases.items():
        rc, msg = call(**kw)
        assert rc == EINVAL, (name, rc, msg)
        assert "quantise_batch" in msg and all(w in msg for w in words), (name, msg)
    # ... and the same planes, unspoilt, are taken
    rc, msg = call(good)
    assert rc == 0, msg
    ctx.synchronize()
    # the subtract call's refusals
    bad = (_lib.ConvertPlane * 1)(_lib.ConvertPlane(co.ptr, co.stride, qu.ptr, *SUBTRACT_REFUSAL))
    assert lib.schro_hip_subtract_batch(ctx.h, bad, 1, 0) == EINVAL and b"subtract_batch: plane 0" in lib.schro_hip_last_error()
    assert lib.schro_hip_subtract_batch(None, bad, 1, 0) == EINVAL
    for p in (co, qu, summ):
        p.free()
    return len(cases)
