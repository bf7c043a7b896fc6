"""The seeded random batches of the encoder's front end as generators that need no device: the downsample and SAD-scan
batches of tests/dry_run_analysis_cases.py and the forward-wavelet batches of tests/dry_run_fwd_cases.py.  Those two walk
them through the Python wrappers; tests/encoder_walk_cases.py writes them into the case file of the stand-alone driver
(tests/c/encoder_walk.cpp)."""
import numpy as np

import schroedinger_amd as sa


def random_scans(rng, w, h, ext, n):
    scans = np.zeros(n, sa.SCAN_DTYPE)
    for s in scans:
        bw, bh = int(rng.integers(-2, 65)), int(rng.integers(-2, 65))
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        dist = int(rng.integers(1, 21))
        rx, ry, sw, sh = sa.metric_scan_setup(x, y, bw, bh, w, h, ext, int(rng.integers(-8, 9)), int(rng.integers(-8, 9)), dist)
        if sw <= 0 or sh <= 0:
            rx, ry, sw, sh = -ext, -ext, 1, 1
            bw, bh = min(bw, 0), min(bh, 0)     # (an empty block fits anywhere)
        s["x"], s["y"], s["block_width"], s["block_height"] = x, y, bw, bh
        s["ref_x"], s["ref_y"], s["scan_width"], s["scan_height"] = rx, ry, sw, sh
        s["gravity_x"], s["gravity_y"] = rx + int(rng.integers(0, sw)) - x, ry + int(rng.integers(0, sh)) - y
        s["dx"], s["dy"] = int(rng.integers(-99, 100)), int(rng.integers(-99, 100))
    return scans


def analysis_batches(count=100, seed=1212):
    """Per round: the planes of one schro_hip_downsample_batch call -- dicts of w, h, ext, src_stride, dst_stride (the
    destination holds (h + 1) // 2 + 2 ext rows of (w + 1) // 2 + 2 ext samples) --, the pictures of one
    schro_hip_metric_scan_batch call -- dicts of w, h, ext, scans -- and whether that call asks for the tables."""
    rng = np.random.default_rng(seed)
    for rnd in range(count):
        down = []
        for n in range(int(rng.integers(1, 7))):
            big = rng.integers(0, 8) == 0
            w, h = int(rng.integers(1, 4097 if big else 400)), int(rng.integers(1, 2305 if big else 300))
            ext = int(rng.choice([0, 0, 1, 8, 32]))
            src_stride = (w, -(-w // 64) * 64, w + 3)[int(rng.integers(0, 3))]
            dw = (w + 1) // 2 + 2 * ext
            dst_stride = (dw, -(-dw // 64) * 64, dw + 5)[int(rng.integers(0, 3))]
            down.append(dict(w=w, h=h, ext=ext, src_stride=src_stride, dst_stride=dst_stride))
        pics = []
        for n in range(int(rng.integers(1, 4))):
            w, h, ext = int(rng.integers(1, 300)), int(rng.integers(1, 200)), int(rng.choice([0, 8, 32]))
            pics.append(dict(w=w, h=h, ext=ext, scans=random_scans(rng, w, h, ext, int(rng.integers(1, 40)))))
        yield down, pics, bool(rnd & 1)


def forward_batches(count=100, seed=1111):
    """Per round: (depth, filter, sample type, [(w, h, src stride, dst stride)]) of one schro_hip_iwt_batch call: rows
    without padding, rounded to 64 bytes, or with an odd number of samples of padding."""
    rng = np.random.default_rng(seed)
    for rnd in range(count):
        depth, filt = int(rng.integers(1, 7)), int(rng.integers(0, 7))
        dtype = (np.int16, np.int32)[int(rng.integers(0, 2))]
        unit, bpp = 1 << depth, np.dtype(dtype).itemsize
        planes = []
        for n in range(int(rng.integers(1, 7))):
            big = rng.integers(0, 8) == 0
            w = unit * int(rng.integers(1, (4096 if big else 700) // unit + 1))
            h = unit * int(rng.integers(1, (2304 if big else 400) // unit + 1))
            strides = []
            for k in range(2):
                strides.append((w * bpp, -(-w * bpp // 64) * 64, -(-w * bpp // 64) * 64 + 3 * bpp)[int(rng.integers(0, 3))])
            planes.append((w, h, strides[0], strides[1]))
        yield depth, filt, dtype, planes
