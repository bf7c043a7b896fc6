"""CPU: the seeded draws of tests/stats_input_draws.py -- deterministic, every drawn call legal (the statistics calls by
their host-only _check twins over the addresses of the layout the GPU test uses, the unpack pictures by the restatement
tests/unpack_ref.py, which raises where the library refuses) -- and what the draws together cover."""
import numpy as np

import picture_stats_cases as K
import schroedinger_amd as sa
import stats_input_draws as D
import unpack_ref as U

BASE = 0x7f0000000000           # never dereferenced: the checks are host only


class At:
    """A region of a layout at an address, as the wrappers take a plane."""

    def __init__(self, spec):
        self.ptr, self.stride, self.width, self.height, self.dtype = BASE + spec.offset, spec.stride, spec.width, spec.height, spec.dtype


def at(spec):
    return At(spec) if spec is not None else None


def same(a, b):
    """Draws compare equal: dicts of numbers, dtypes and tuples."""
    return repr(a) == repr(b)


def test_the_unpack_tile_lengths_come_from_the_library():
    from schroedinger_amd import _lib
    assert "schro_hip_unpack_geometry" in _lib.EXPORTED_SYMBOLS
    g = sa.unpack_geometry()
    assert g["tile_bytes"] > 0 and g["tile_bytes"] % 16 == 0 and g["tile_rows"] > 0      # whole 16-byte pieces
    assert sorted(g["iwt"]) == [(f, b) for f in range(7) for b in (2, 4)] and sa.UNPACK_GEOMETRY == 2 + 4 * 14
    for (f, bpp), (uc, ur, hc, hr) in g["iwt"].items():
        assert uc > 0 and ur > 0 and hc >= hr >= 0
        assert uc * bpp % 128 == 0                      # a tile's band rows are whole 128-byte lines (iwt_fwd.hip FwdGeo)
        assert (hr == 0) == (f in (3, 4))               # only the Haar filters reach no neighbour
    assert D.TILE_BYTES == g["tile_bytes"]


def test_the_generators_are_deterministic():
    for gen in (D.unpack_calls, D.sums_calls, D.lowpass_calls, D.ssim_calls):
        first, again = list(gen()), list(gen())
        assert same(first, again) and len(first) == (D.UNPACK_CALLS if gen is D.unpack_calls else D.STATS_CALLS)
        assert not same(first, list(gen(seed=1)))


def test_every_statistics_call_is_accepted_by_its_check_twin():
    for call in D.sums_calls():
        _lay, specs = D.sums_layout(call)
        sa.plane_sums_check([(at(a), at(b), at(r)) for a, b, r in specs])
    for call in D.lowpass_calls():
        _lay, specs = D.lowpass_layout(call)
        sa.lowpass2_check([(at(p), e["hs"], e["vs"], at(c)) for (p, c), e in zip(specs, call)])
    for call in D.ssim_calls():
        _lay, specs = D.ssim_layout(call)
        sa.ssim_check([(at(a), at(b), at(m), at(s), at(r)) for a, b, m, s, r in specs])


def source_shape(p):
    """A source of the right shape for the restatement (zeros: only the sizes and formats are judged here)."""
    if len(p["src"]) == 3:
        fmt, sw, sh = p["src"]
        return (np.zeros((sh, U.row_bytes(fmt, sw)), np.uint8), fmt, sw, sh)
    dt, hs, vs, sw, sh = p["src"]
    return ([np.zeros((U.shifted(sh, vs if k else 0), U.shifted(sw, hs if k else 0)), dt) for k in range(3)], hs, vs, sw, sh)


def test_every_unpack_picture_is_accepted_by_the_restatement():
    for call in D.unpack_calls():
        assert 1 <= len(call) <= 12
        for p in call:
            out = U.convert(source_shape(p), p["dtype"], p["hs"], p["vs"], p["w"], p["h"])              # raises Refused
            assert [a.shape for a in out] == [(U.shifted(p["h"], p["vs"] if k else 0), U.shifted(p["w"], p["hs"] if k else 0)) for k in range(3)]
            assert p["w"] * p["dtype"].itemsize <= 2 * D.TILE_BYTES + 40


def test_what_the_unpack_draws_cover():
    pictures = [p for call in D.unpack_calls() for p in call]
    packed = [p for p in pictures if len(p["src"]) == 3]
    assert {(p["src"][0], p["dtype"].itemsize) for p in packed} == {(f, b) for f in U.PACKED for b in (1, 2, 4) if not (f == U.AY64 and b == 1)}
    assert {(np.dtype(p["src"][0]).itemsize, p["dtype"].itemsize) for p in pictures if len(p["src"]) == 5} == {(s, d) for s in (1, 2, 4) for d in (1, 2, 4)}
    sizes = [(p["src"][-2], p["src"][-1], p["w"], p["h"]) for p in pictures]
    assert any(sw > w or sh > h for sw, sh, w, h in sizes) and any(sw < w or sh < h for sw, sh, w, h in sizes)   # crop, extension
    assert not any((w < sw or h < sh) and (w > sw or h > sh) for sw, sh, w, h in sizes)                          # never a mix
    for bpp in (1, 2, 4):
        crossing = [p for p in pictures if p["dtype"].itemsize == bpp and p["w"] * bpp > D.TILE_BYTES]
        assert len(crossing) >= 5, (bpp, len(crossing))
        # ... at least three of them stored with 16-byte stores (tile column 1 and later on the vector path), and some not
        vector = [p for p in crossing if D.vector_stores(p)]
        assert len(vector) >= 3 and len(vector) < len(crossing), (bpp, len(vector), len(crossing))
    # a chroma change (u8 destinations only), and starts and strides off their alignment on both sides
    changes = [p for p in pictures if (p["hs"], p["vs"]) != tuple(U.NATURAL[p["src"][0]][1:] if len(p["src"]) == 3 else p["src"][1:3])]
    assert changes and all(p["dtype"] == np.uint8 for p in changes)
    for key in ("src_skew", "src_pad", "dst_skew", "dst_pad"):
        assert {0} < {p[key] for p in pictures}
    assert all(D.vector_stores(p) for p in pictures if "dst_stride" in p)
    assert all(p["dst_stride"] >= p["w"] * p["dtype"].itemsize for p in pictures if "dst_stride" in p)


def test_what_the_statistics_draws_cover():
    for gen in (D.sums_calls, D.lowpass_calls):
        lengths = [len(c) for c in gen()]
        assert max(lengths) > K.TABLE_ROUND and min(lengths) < 40 and max(lengths) <= 200
    lengths = [len(c) for c in D.ssim_calls()]
    assert 3 * max(lengths) > 2 * max(lengths) > K.TABLE_ROUND and max(lengths) <= D.MOST_SSIM_PICTURES   # entries of the low-pass tables
    for gen in (D.sums_calls, D.lowpass_calls, D.ssim_calls):
        sizes = [(e["w"], e["h"]) for c in gen() for e in c]
        assert any(w > 300 and h <= 4 for w, h in sizes) and any(h > 300 and w <= 4 for w, h in sizes)
        assert all((w < 300 and h < 80) or (max(w, h) <= 2100 and min(w, h) <= 4) for w, h in sizes)
    entries = [e for c in D.lowpass_calls() for e in c]
    assert {e["hs"] for e in entries} == {e["vs"] for e in entries} == set(K.SIGMAS)
    assert {(e["dtype"].name, e["kind"]) for e in entries} == {("uint8", "noise"), ("uint8", "steps"), ("int16", "noise"), ("int16", "steps"),
                                                               ("int16", "full")}
    entries = [e for c in D.sums_calls() for e in c]
    assert {(e["dtype"].name, e["second"]) for e in entries} == {("uint8", False), ("uint8", True), ("int16", False)}
    entries = [e for c in D.ssim_calls() for e in c]
    assert {e["map"] for e in entries} == {False, True} and {e["kind"] for e in entries} == {"same", "noisy", "unrelated"}
