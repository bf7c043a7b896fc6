"""GPU: schro_hip_unpack_batch (unpack.hip) at its tile borders, against tests/unpack_ref.py bit for bit, in guarded blocks
like tests/test_gpu_unpack.py (whose `run` this file uses).

A tile of unpack_kernel is T destination bytes of a row by R rows (sa.unpack_geometry (): the library's own numbers), so
n = T / bytes per destination sample is the first sample of the second tile column.  The widest destination of
tests/test_gpu_unpack.py is 352 samples: its u8 and s16 pictures never leave the first tile column.  Here every packed
format and every planar depth goes into every destination depth at

  (n + 6, 5) -> (n + 1, 5)      a crop whose last 16-byte piece is partial, one sample into the second tile column
  (n - 4, 3) -> (n + 6, 5)      the edge extension starts inside tile column 0 and fills what there is of column 1
  (2n + 2, 4) -> (2n + 1, 3)    three tile columns
  (6, 2) -> (n + 2, 9)          nearly all of it extension, over three tile rows

(source size -> destination size), each picture once with destination planes at 256-byte boundaries whose stride is the row
rounded up to 16 bytes (the library's condition for 16-byte stores: whole pieces are stored as vectors, a row's last partial
piece sample by sample) and once a sample off the boundary with three samples of padding (scalar stores throughout).  n is
no multiple of 6, so a v210 group straddles the border; a YUYV / UYVY pair and a 16-byte source word do where the
destination is deeper than the source."""
import numpy as np
import pytest

import schroedinger_amd as sa
import test_gpu_unpack as T
import unpack_ref as U

pytestmark = pytest.mark.gpu

_G = sa.unpack_geometry()
TILE_BYTES, TILE_ROWS = _G["tile_bytes"], _G["tile_rows"]
DTYPES = [np.uint8, np.int16, np.int32]
IDS = ["u8", "s16", "s32"]
SKEWED = dict(dst_skew=1, dst_pad=3)


def samples(dtype):
    return TILE_BYTES // np.dtype(dtype).itemsize


def pairs(dtype):
    n = samples(dtype)
    return [((n + 6, 5), (n + 1, 5)), ((n - 4, 3), (n + 6, 5)), ((2 * n + 2, 4), (2 * n + 1, 3)), ((6, 2), (n + 2, 9))]


def heights():
    return [TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS]


def even_source(fmt, src):
    return (src[0] + (src[0] & 1), src[1]) if fmt in T.EVEN_ONLY else src


def both_alignments(src, dtype, hs, vs, dst):
    """The picture twice: with every destination plane at a 256-byte boundary and a stride that is a multiple of 16 (the
    luma row rounded up; the chroma planes take the same stride), which is the library's condition for 16-byte stores
    (plane_unpack.cpp: pointer | stride multiples of 16), and a sample off with three samples of padding, which is not."""
    row = dst[0] * np.dtype(dtype).itemsize
    return [T.picture(src, dtype, hs, vs, dst, dst_stride=-(-row // 16) * 16), T.picture(src, dtype, hs, vs, dst, **SKEWED)]


def vector_stores(p):
    """Whether every destination plane of a picture, as `T.run` lays it out (planes at 256-byte boundaries plus dst_skew
    samples), has a pointer and a stride that are multiples of 16."""
    bpp = p["dtype"].itemsize
    strides = [p.get("dst_stride", U.shifted(p["w"], p["hs"] if k else 0) * bpp + p.get("dst_pad", 0) * bpp) for k in range(3)]
    return all((p.get("dst_skew", 0) * bpp) % 16 == 0 and st % 16 == 0 for st in strides)


def test_the_aligned_copies_take_vector_stores_and_the_skewed_ones_do_not():
    for dtype in DTYPES:
        for src, dst in pairs(dtype):
            aligned, skewed = both_alignments((U.AYUV,) + src, dtype, 0, 0, dst)
            assert vector_stores(aligned) and not vector_stores(skewed), (dtype, dst)
            row = dst[0] * np.dtype(dtype).itemsize
            assert aligned["dst_stride"] >= row > TILE_BYTES and aligned["dst_stride"] - row < 16
        # whole pieces (16-byte stores) past the tile border, and in some rows a partial last piece (scalar) beside them
        assert any(dst[0] * np.dtype(dtype).itemsize % 16 for _src, dst in pairs(dtype))
    for h in heights():
        for p, want in zip(both_alignments((U.UYVY, 2 * TILE_BYTES + 2, h), np.uint8, 1, 1, (2 * TILE_BYTES + 2, h)), (True, False)):
            assert vector_stores(p) == want


def test_the_getter_names_the_tile_and_the_sizes_stand_around_it():
    assert TILE_BYTES % 16 == 0 and TILE_BYTES % 6 != 0 and TILE_ROWS >= 2
    for dtype in DTYPES:
        n = samples(dtype)
        assert n % 6 and (n // 2) % 6                   # a v210 group of six straddles the luma and the chroma border
        widths = {dst[0] for _src, dst in pairs(dtype)}
        assert {n + 1, n + 2, n + 6, 2 * n + 1} <= widths
        assert max(-(-w * np.dtype(dtype).itemsize // TILE_BYTES) for w in widths) == 3         # three tile columns
        assert max(-(-dst[1] // TILE_ROWS) for _src, dst in pairs(dtype)) == 3                   # three tile rows
    assert 352 * 2 < TILE_BYTES                         # (what tests/test_gpu_unpack.py reaches for u8 and s16)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_packed_format_across_the_tile_border(ctx, dtype):
    pics = []
    for fmt in U.PACKED:
        if fmt == U.AY64 and np.dtype(dtype) == np.uint8:
            continue                                    # refused (tests/test_gpu_unpack.py "ay64-u8")
        hs, vs = T.natural(fmt)
        for src, dst in pairs(dtype):
            pics += both_alignments((fmt,) + even_source(fmt, src), dtype, hs, vs, dst)
    assert len(pics) <= 85                              # SCHRO_HIP_UNPACK_MAX_PICTURES: one call takes no more
    T.run(ctx, pics, seed=30 + np.dtype(dtype).itemsize)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_planar_sources_of_every_depth_across_the_tile_border(ctx, dtype):
    pics = []
    for m, sd in enumerate(DTYPES):
        for k, (src, dst) in enumerate(pairs(dtype)):
            hs, vs = ((0, 0), (1, 0), (1, 1))[(m + k) % 3]
            pics += both_alignments((sd, hs, vs) + src, dtype, hs, vs, dst)
    T.run(ctx, pics, seed=40 + np.dtype(dtype).itemsize)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_heights_around_the_tile_rows_at_a_width_that_crosses(ctx, dtype):
    n = samples(dtype)
    formats = [f for f in U.PACKED if not (f == U.AY64 and np.dtype(dtype) == np.uint8)]
    pics = []
    for k, h in enumerate(heights()):
        for fmt in (formats[k % len(formats)], formats[(k + 3) % len(formats)]):
            hs, vs = T.natural(fmt)
            pics += both_alignments((fmt,) + even_source(fmt, (n + 1, h)), dtype, hs, vs, (n + 1, h))
        pics += both_alignments((np.int16, 1, 1, n + 3, h), dtype, 1, 1, (n + 3, h))       # 4:2:0: chroma rows rounded up
    T.run(ctx, pics, seed=50 + np.dtype(dtype).itemsize)


def test_u8_chroma_changes_across_the_tile_border(ctx):
    """AYUV 4:4:4 -> 4:2:0 (every second sample and row) and UYVY 4:2:2 -> 4:2:0 (every second row) at 2T + 2 samples: the
    chroma planes are T + 1 wide, the decimating lanes' source coordinates cross the packed row's middle."""
    w = 2 * TILE_BYTES + 2
    pics = []
    for h in heights():
        pics += both_alignments((U.AYUV, w, h), np.uint8, 1, 1, (w, h))
        pics += both_alignments((U.UYVY, w, h), np.uint8, 1, 1, (w, h))
    # ... and with the sizes changing too: a crop and an extension that begin in one chroma tile and end in the next
    pics += both_alignments((U.AYUV, w + 6, 5), np.uint8, 1, 1, (w, 5))
    pics += both_alignments((U.UYVY, w - 10, 3), np.uint8, 1, 1, (w, 5))
    pics += both_alignments((U.YUYV, w - 10, 3), np.uint8, 0, 0, (w, 5))         # repetition 4:2:2 -> 4:4:4
    T.run(ctx, pics, seed=61)
