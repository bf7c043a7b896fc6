"""The geometries and inputs of the picture-statistics tests, shared by the CPU test of the restatement
(tests/test_picture_stats_ref.py) and the GPU test (tests/test_gpu_picture_stats.py)."""
import numpy as np

import schroedinger_amd as sa

# the tile and chunk lengths of the kernels, from the library itself (schro_hip_picture_stats_geometry)
_G = sa.picture_stats_geometry()
SUMS_TILE_BYTES, SUMS_TILE_ROWS = _G["sums_tile_bytes"], _G["sums_tile_rows"]
LOWPASS_ROWS = _G["lowpass_rows"]               # rows of a row-pass workgroup (a lane a row)
LOWPASS_CHUNK = _G["lowpass_chunk"]             # columns staged in LDS at a time: the state crosses this border in registers
LOWPASS_COLS = _G["lowpass_cols"]               # columns of a column-pass workgroup (a lane a column)
LOWPASS_COL_ROWS = _G["lowpass_col_rows"]       # rows a column-pass lane loads at a time
SSIM_TILE_COLS, SSIM_TILE_ROWS = _G["ssim_tile_cols"], _G["ssim_tile_rows"]

SIGMAS = (0.375, 0.75, 1.5, 2.5, 5, 22.5)

SUMS_SIZES = [(w, h) for w in (1, 3, 63, 64, 65, 257) for h in (1, 2, 67)]


def around(*lengths):
    return sorted({n + d for n in lengths for d in (-1, 0, 1)})


# (width, height): the grid the issue names, the two long thin planes, and one below / at / one above every chunk or tile
# length of the kernels along the axis it counts (and twice the chunk: two borders)
LOWPASS_SIZES = ([(w, h) for w in (1, 2, 3, 63, 64, 65, 130) for h in (1, 2, 5, 67)]
                 + [(4099, 3), (3, 4099)]
                 + [(w, 3) for w in around(LOWPASS_CHUNK, 2 * LOWPASS_CHUNK)]           # (LOWPASS_COLS +- 1 is in the grid)
                 + [(5, h) for h in around(LOWPASS_ROWS, LOWPASS_COL_ROWS, 2 * LOWPASS_COL_ROWS)])

SSIM_SIZES = [(48, 40), (130, 67), (257, 5)]
# the SSIM tile arithmetic: widths below the eight result words' lanes, one below / at / one above both tile lengths, several
# tiles across AND down, more tiles than ssim_sum_kernel has lanes (3 x 2049: its strided loop's second turn), and the two
# widths on either side of generate_coeff's branch (width / 256 * 1.5 against 2.5)
SSIM_GEOMETRY_SIZES = [(1, 1), (2, 3), (7, 9), (255, 7), (256, 8), (257, 9), (257, 17), (3, 2049), (426, 9), (427, 9), (513, 17)]
SSIM_SUM_LANES = SSIM_TILE_COLS                 # (ssim.hip: a lane owns a column of the tile, and a tile's sum in the last kernel)

# the most entries a call takes (kMaxJobs, kMaxSsimPictures: what the _check twins refuse above) and the 64 a table lookup
# probes per round (find_job, lowpass_find)
TABLE_ROUND = 64
FULL_TABLE_JOBS = (65, 130, 256)
FULL_TABLE_PLANES = (65, 129, 256)
FULL_TABLE_PICTURES = (22, 33, 64)              # x 2 u8 and x 3 s16 low-pass planes: 66 .. 192 entries


def tiny_size(k):
    """1 .. 9 by 1 .. 9, unlike from entry to entry, and every 23rd 65 x 3: what fills a table without filling a test."""
    return (65, 3) if k % 23 == 5 else (1 + (k * 7) % 9, 1 + (k * 5 + k // 9) % 9)


def long_stride(k, row_bytes):
    """Longer than the row, even, unlike from entry to entry."""
    return (row_bytes + 1) // 2 * 2 + 2 * (k % 7) + (62 if k % 5 == 0 else 0)


def sigma_pair(k):
    """Unlike h and v sigmas for case k, every sigma of SIGMAS in turn on either axis."""
    return SIGMAS[k % len(SIGMAS)], SIGMAS[(k // 2 + 3) % len(SIGMAS)]


def noise(w, h, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    return rng.integers(-2048, 2048, (h, w)).astype(np.int16)


def full_range_s16(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-32768, 32768, (h, w)).astype(np.int16)
    a.flat[:: 7] = 32767
    a.flat[3:: 11] = -32768
    return a


def steps(w, h, dtype):
    """0 -> top steps along both axes: a quadrant pattern."""
    top = 255 if np.dtype(dtype) == np.uint8 else 32767
    a = np.zeros((h, w), dtype)
    a[:, w // 2:] = top
    a[h // 2:, :] = top - a[h // 2:, :]
    return a


def lowpass_input(kind, w, h, dtype, seed):
    if kind == "noise":
        return noise(w, h, dtype, seed)
    if kind == "steps":
        return steps(w, h, dtype)
    assert kind == "full" and np.dtype(dtype) == np.int16
    return full_range_s16(w, h, seed)


def picture(w, h, seed):
    """A smooth u8 picture with some texture."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 128 + 70 * np.sin(x / 9.0 + seed) * np.cos(y / 7.0) + rng.normal(0, 6, (h, w))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def ssim_pair(kind, w, h, seed):
    a = picture(w, h, seed)
    if kind == "same":
        return a, a.copy()
    if kind == "noisy":
        rng = np.random.default_rng(seed + 100)
        return a, np.clip(a.astype(np.int32) + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
    assert kind == "unrelated"
    return a, noise(w, h, np.uint8, seed + 200)


def lowpass_cases():
    """(width, height, dtype, kind, h sigma, v sigma, seed) of every low-pass plane both tests run."""
    out = []
    for k, (w, h) in enumerate(LOWPASS_SIZES):
        for dtype, kinds in ((np.uint8, ("noise", "steps")), (np.int16, ("noise", "steps", "full"))):
            hs, vs = sigma_pair(k + (dtype == np.int16))
            out.append((w, h, dtype, kinds[k % len(kinds)], hs, vs, 1000 + k))
    return out
