"""CPU: tests/rough_hint_ref.py -- the restatement of schro_rough_me_heirarchical_scan_hint -- against properties the C text
implies.  None compares the restatement with itself on the same path."""
import ctypes as C
import os

import numpy as np
import pytest

import analysis_ref as A
import oracle_lib as O
import rough_hint_cases as K
import rough_hint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def have_ref_kernels():
    try:
        O.reforc()
        return True
    except Exception:
        return False


def sad_at(frame, ref, x, y, dx, dy, bw, bh, ext):
    """The SAD of the bw x bh block at (x, y) of frame against (x + dx, y + dy) of ref: through the reference's compiled
    kernel (schro_metric_absdiff_u8 on edge-extended copies) where oracle/_ref is built, else through block_at."""
    if have_ref_kernels():
        e = ext + 64
        f, r = np.ascontiguousarray(A.edgeextend(frame, e)), np.ascontiguousarray(A.edgeextend(ref, e))
        at = lambda a, px, py: C.c_void_p(a.ctypes.data + (py + e) * a.strides[0] + (px + e))
        return A.sad_orc(at(f, x, y), f.strides[0], at(r, x + dx, y + dy), r.strides[0], bw, bh)
    return int(np.abs(A.block_at(frame, x, y, bw, bh).astype(np.int32) - A.block_at(ref, x + dx, y + dy, bw, bh).astype(np.int32)).sum())


@pytest.mark.parametrize("name", ["partial_blocks", "beyond_the_picture", "odd_counts_shift2", "extension_32", "block_12x12", "block_16x8",
                                  "ref_1_shift2", "shift3_odd", "hints_wild"])
def test_every_stored_metric_is_the_sad_at_the_stored_vector(name):
    c = K.CASES[name]
    frame, ref, _ = K.inputs(name)
    field, _ = K.expected(name)
    shift, skip, r = c["shift"], 1 << c["shift"], c["ref_index"]
    seen = 0
    for j in range(c["nby"]):
        for i in range(c["nbx"]):
            mv = field[j * c["nbx"] + i]
            if i % skip or j % skip:
                assert mv.tobytes() == np.array([(1, 0, 0, (0, 0, 0, 0))], O.MV_DTYPE).tobytes()   # schro_motion_field_set (mf, 0, 1)
                continue
            x, y = (i >> shift) * c["xb"], (j >> shift) * c["yb"]
            bw, bh = min(c["w"] - x, c["xb"]), min(c["h"] - y, c["yb"])
            assert mv["flags"] == 1 and mv["chroma_metric"] == 0 and mv["v"][1 - r] == 0 and mv["v"][3 - r] == 0
            if mv["metric"] == A.METRIC_INVALID:
                assert mv["v"][r] == 0 and mv["v"][2 + r] == 0
                continue
            dx, dy = int(mv["v"][r]), int(mv["v"][2 + r])
            assert dx % skip == 0 and dy % skip == 0        # stored << shift
            if bw <= 0 or bh <= 0:
                assert mv["metric"] == 0
                continue
            assert mv["metric"] == sad_at(frame, ref, x, y, dx >> shift, dy >> shift, bw, bh, c["ext"]), (i, j)
            seen += 1
    assert seen > 10


def shifted_pyramids(w, h, n_levels, dx, dy, seed):
    """Pyramids of a frame and of a reference whose EVERY level is the frame's level moved by (dx, dy) >> level (built per
    level: downsampling a moved picture is not the moved downsampled picture at odd phases)."""
    frames = A.pyramid(K.texture(w, h, seed), n_levels)
    refs = [K.moved(f, dx >> k, dy >> k, 0, noise=0) for k, f in enumerate(frames)]
    return frames, refs


@pytest.mark.parametrize("vec", [(8, -16), (-16, 8), (16, 16), (0, -8)])
def test_a_shifted_reference_yields_its_vector_at_every_interior_block(vec):
    """ref (x, y) = frame (x - dx, y - dy) at every level, (dx, dy) a multiple of 2 << shift of the top level and within
    its reach of 12: every block whose block and match lie inside the pictures finds (dx, dy) with SAD 0, at every level."""
    n_levels, (dx, dy) = 2, vec
    assert dx % (2 << n_levels) == 0 and dy % (2 << n_levels) == 0 and max(abs(dx), abs(dy)) >> n_levels <= 12
    w, h = 256, 192
    frames, refs = shifted_pyramids(w, h, n_levels, dx, dy, 77)
    P = dict(x_num_blocks=w // 8, y_num_blocks=h // 8, xbsep_luma=8, ybsep_luma=8)
    fields = R.rough_scan(frames, refs, P, n_levels, 0)
    for shift in range(1, n_levels + 1):
        lh, lw = frames[shift].shape
        checked = 0
        for j in range(0, P["y_num_blocks"], 1 << shift):
            for i in range(0, P["x_num_blocks"], 1 << shift):
                x, y = (i >> shift) * 8, (j >> shift) * 8
                mx, my = x + (dx >> shift), y + (dy >> shift)
                margin = 8      # keep clear of the repeated edge samples, where other vectors give SAD 0 too
                if x + 8 > lw or y + 8 > lh or mx < margin or my < margin or mx + 8 > lw - margin or my + 8 > lh - margin:
                    continue
                mv = fields[shift][j * P["x_num_blocks"] + i]
                assert (int(mv["v"][0]), int(mv["v"][2]), int(mv["metric"])) == (dx, dy, 0), (shift, i, j)
                checked += 1
        assert checked >= 4, shift


@pytest.mark.parametrize("ext", [0, 32])
def test_a_flat_picture_yields_the_zero_vector_everywhere(ext):
    """Every SAD is 0: the first candidate (the zero vector) wins the candidate test, the gravity position is kept by the
    scan.  Any other tie rule moves a vector."""
    w, h, n_levels = 96, 80, 3
    flat = A.pyramid(np.full((h, w), 90, np.uint8), n_levels)
    P = dict(x_num_blocks=w // 8, y_num_blocks=h // 8, xbsep_luma=8, ybsep_luma=8)
    top = R.rough_scan(flat, flat, P, n_levels, 0, ext)[n_levels]
    # the nohint level's gravity is the window's first position: its vectors are NOT zero in a flat picture
    assert top["v"].any()
    hint = np.zeros(P["x_num_blocks"] * P["y_num_blocks"], O.MV_DTYPE)
    for shift in (2, 1):
        f = R.rough_scan_hint(flat[shift], flat[shift], P, shift, 4, 0, hint, ext)
        assert not f["v"].any() and not f["metric"].any()
        hint = f
    # and under the nohint level's vectors: the zero vector is the first candidate of equal metrics, so it still wins
    f = R.rough_scan_hint(flat[2], flat[2], P, 2, 4, 0, top, ext)
    assert not f["v"].any() and not f["metric"].any()


@pytest.mark.parametrize("name", ["partial_blocks", "beyond_the_picture", "odd_counts_shift2", "hints_wild", "shift3_odd", "block_4x4"])
def test_anti_diagonal_order_gives_the_raster_field(name):
    """The relaxation the kernel relies on: a block reads its left, upper and upper-left neighbours only."""
    c = K.CASES[name]
    frame, ref, hint = K.inputs(name)
    got = R.rough_scan_hint(frame, ref, K.params_of(c), c["shift"], c["dist"], c["ref_index"], hint, c["ext"], order="diagonal")
    assert got.tobytes() == K.expected(name)[0].tobytes()
    blocks = R.block_order(c["nbx"], c["nby"], 1 << c["shift"], "diagonal")
    assert blocks != R.block_order(c["nbx"], c["nby"], 1 << c["shift"], "raster") or len(blocks) < 3


def test_candidate_list_order_and_masking():
    """schroroughmotion.c:199-228 on a field whose records name themselves."""
    nbx, nby, shift = 9, 7, 1
    hint = np.zeros(nbx * nby, O.MV_DTYPE)
    mvs = np.zeros(nbx * nby, O.MV_DTYPE)
    for k in range(nby):
        for l in range(nbx):
            hint[k * nbx + l]["v"] = (100 + l, 0, 100 + k, 0)
            mvs[k * nbx + l]["v"] = (200 + l, 0, 200 + k, 0)
    # an interior block: parents at (i -+ 2) & ~3, neighbours at i - 2
    assert R.candidates(mvs, hint, nbx, nby, 4, 2, shift, 0) == [(0, 0), (100, 100), (104, 100), (100, 104), (104, 104), (202, 202), (204, 200),
                                                                 (202, 200)]
    # the first block: (0 - 2) & ~3 = -4 stays negative -- only the parent at (0, 0) ... m = 3: (2 & ~3, 2 & ~3) = (0, 0)
    assert R.candidates(mvs, hint, nbx, nby, 0, 0, shift, 0) == [(0, 0), (100, 100)]
    # the last column / row: parents at 8 is inside nbx = 9, at 8 is outside nby = 7
    assert R.candidates(mvs, hint, nbx, nby, 8, 6, shift, 0) == [(0, 0), (104, 104), (108, 104), (206, 206), (208, 204), (206, 204)]
    # the other reference reads dx[1], dy[1]
    assert R.candidates(mvs, hint, nbx, nby, 2, 0, shift, 1) == [(0, 0), (0, 0), (0, 0), (0, 0)]


def test_negative_vectors_shift_arithmetically_and_store_as_int16():
    """A hint of (-3, -5) at shift 1: the candidate position uses (i * xbsep - 3) >> 1 (floor), the gravity -3 >> 1 = -2."""
    w, h = 64, 48
    frame = K.texture(w, h, 5)
    ref = K.moved(frame, -2, -3, 0, noise=0)
    P = dict(x_num_blocks=16, y_num_blocks=12, xbsep_luma=8, ybsep_luma=8)
    hint = K.constant_field(16, 12, -3, -5)
    f = R.rough_scan_hint(frame, ref, P, 1, 4, 0, hint)
    mv = f[6 * 16 + 8]          # an interior block: the match at (-2, -3), stored << 1
    assert (int(mv["v"][0]), int(mv["v"][2]), int(mv["metric"])) == (-4, -6, 0)
    assert R._int16(40000) == 40000 - 65536 and R._int16(-40000) == 65536 - 40000
