"""GPU: the VC-2 low-delay intra encoder from the bytes a capture card delivers.  v210 4:2:2 rows go through
schro_hip_unpack_iwt_batch (three-level Haar) into schro_hip_lowdelay_encode_batch, the coefficient planes staying on
the device; the slice bytes must equal the same encoder's output from planes unpacked on the host with the restatement
(tests/unpack_ref.py), uploaded and transformed by schro_hip_iwt_batch.  Then schro_hip_lowdelay_batch and
schro_hip_iiwt_pack_v210_batch bring the picture back: the slices are large enough for every one of them to fit at base
index 0 (no quantisation), so the v210 bytes that come out are the ones that went in.

The slice encoder takes s16 coefficients only (the reference's encoder is s16; it refuses s32), so the chain runs in
s16: 10-bit samples through three Haar levels stay far inside 16 bits.  192 x 16 is one row of tiles."""
import numpy as np
import pytest

import lowdelay_enc_cases as K
import oracle_lib as O
import schroedinger_amd as sa
import unpack_ref as U

pytestmark = pytest.mark.gpu

W, H, DEPTH = 192, 16, 3


def encode(ctx, coeffs, P, nslices, nbytes):
    sl, ix, cn = ctx.plane(1, nbytes, np.uint8), ctx.plane(1, nslices, np.uint8), ctx.plane(1, 1, np.uint32)
    ctx.lowdelay_encode_batch([(coeffs, sl, ix, cn)], P)
    return sl, ix, cn


@pytest.mark.parametrize("filt", [3, 4], ids=["haar0", "haar1"])
def test_v210_in_slices_out_and_back(ctx, filt):
    P = K.params(W, H, 422, DEPTH, 6, 2, 2048, 1)
    assert (P["iwt_luma_width"], P["iwt_luma_height"], P["iwt_chroma_width"]) == (W, H, W // 2)
    nslices = P["n_horiz_slices"] * P["n_vert_slices"]
    nbytes = P["slice_bytes_num"] * nslices // P["slice_bytes_denom"]
    r = np.random.default_rng(filt)
    planes = [r.integers(-512, 512, (H, w)).astype(np.int16) for w in (W, W // 2, W // 2)]
    v210 = O.pack_v210(planes, 1, 0, W, H)              # the pad bits are zero, as a capture card leaves them
    assert v210.shape == (H, sa.unpack_row_bytes(sa.FORMAT_V210, W))

    # packed bytes -> coefficients -> slices, on the device
    d_v210 = ctx.upload(v210)
    co = [ctx.plane(H, w, np.int16) for w in (W, W // 2, W // 2)]
    ctx.unpack_routes(reset=True)               # (either route: the bytes are the same)
    ctx.unpack_iwt_batch([(d_v210, sa.FORMAT_V210, W, H, W, H, co, 1, 0, W, H)], DEPTH, filt)
    assert sum(ctx.unpack_routes().values()) == 1
    sl, ix, cn = encode(ctx, co, P, nslices, nbytes)

    # the same encoder on planes unpacked on the host
    host = U.chain(v210, U.V210, (W, H), (W, H), (W, H), (1, 0), np.int16)
    assert all(np.array_equal(a, b) for a, b in zip(host, planes))
    up = [ctx.upload(p) for p in host]
    co2 = [ctx.plane(H, w, np.int16) for w in (W, W // 2, W // 2)]
    ctx.iwt_batch(list(zip(up, co2)), DEPTH, filt)
    sl2, ix2, cn2 = encode(ctx, co2, P, nslices, nbytes)
    ctx.synchronize()
    for a, b in zip(co, co2):
        assert np.array_equal(a.download(), b.download())
    assert np.array_equal(sl.download(), sl2.download())
    assert np.array_equal(ix.download(), ix2.download()) and not ix.download().any(), ix.download()
    assert int(cn.download()[0, 0]) == 0 == int(cn2.download()[0, 0])

    # ... and back: the slice decoder and the inverse wavelet writing v210
    dec = [ctx.plane(H, w, np.int16) for w in (W, W // 2, W // 2)]
    back = ctx.plane(H, v210.shape[1], np.uint8)
    ctx.lowdelay_batch([(sl, dec)], P)
    ctx.iiwt_pack_v210_batch([(dec, 1, 0, back, W, H)], DEPTH, filt)
    ctx.synchronize()
    assert np.array_equal(back.download(), v210)
    for p in [d_v210, sl, ix, cn, sl2, ix2, cn2, back] + co + co2 + up + dec:
        p.free()
