"""The prologue of the 8-bit lane-per-block decoder (k_dec_px.hip): entry loads from clamped addresses, stream loads without a branch.
Every case decodes the self-indexed container (its level-2 table) and with the out-of-band index of the same encode, compares the
raster byte for byte and expects a clean status.  Small rasters with every kind of edge, rasters of more than 16384 segments (several
table chunks, last workgroups with waves that have no segment), and segments of a few dwords next to segments of more than the 512
dwords of one round of stream loads."""
import pytest

pytestmark = pytest.mark.gpu

FTL, BASE = 8, 4


def round_trip(qb3, img, w, h, b, mode):
    """img: flat device tensor; encodes it once with table and index, decodes it both ways"""
    import torch
    from qb3_amd import device as qdev
    enc = qdev.DeviceEncoder(w, h, b, 0, mode=mode, want_index=True, index_chunk=2)
    d, n, index = enc.encode(img)
    dec = qdev.DeviceDecoder(d, n)
    for ix in (None, index):
        out = dec.decode(d, index=ix)
        assert torch.equal(out, img), "decode %s differs" % ("from the table" if ix is None else "with the index")
        assert qb3.lib.qb3x_last_decode_status(dec.p) == 0


def noisy(w, h, b, seed):
    from qb3_amd import synth
    return synth.generate(w, h, b, 0, "NOISY3", seed, device="cuda").view(-1)


@pytest.mark.parametrize("case", [(509, 259, 3, FTL), (1021, 13, 1, FTL), (508, 508, 3, FTL), (333, 77, 4, BASE)], ids=lambda c: "%dx%dx%d-m%d" % c)
def test_small_rasters(qb3, case):
    """edges that are no multiple of 4, one block row, a last segment of one block (508 x 508), four bands"""
    w, h, b, mode = case
    round_trip(qb3, noisy(w, h, b, 31), w, h, b, mode)


@pytest.mark.parametrize("case", [(4100, 4100, 3, FTL), (4099, 4101, 4, BASE), (8200, 2051, 1, FTL)], ids=lambda c: "%dx%dx%d-m%d" % c)
def test_large_rasters(qb3, case):
    """just above 16384 segments, 24 table chunks: segment counts that are no multiple of a workgroup's four, unaligned rows
    (8200 x 2051 x 1, 4099 x 4101 x 4)"""
    w, h, b, mode = case
    round_trip(qb3, noisy(w, h, b, 37), w, h, b, mode)


def test_short_and_long_segments(qb3):
    """a constant top half over a bottom half of uniform random bytes, BASE: segments of a few dwords (most lanes load a clamped
    address and stage a zero) next to segments above 512 dwords (a second round of loads)"""
    import torch
    w = h = 4100
    g = torch.Generator(device="cuda").manual_seed(5)
    img = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda")
    img[h // 2:] = torch.randint(0, 256, (h - h // 2, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    round_trip(qb3, img.view(-1), w, h, 3, BASE)


def test_tile_batch(qb3):
    """five tiles of 4113 segments each (blockIdx.y in play), from the containers alone and with the indices"""
    import torch
    from qb3_amd import device as qdev, synth
    w = h = 2052
    n = 5
    imgs = torch.stack([synth.generate(w, h, 3, 0, "NOISY3", 700 + t, device="cuda") for t in range(n)])
    tc = qdev.TileBatchCoder(w, h, 3, 0, n, want_index=True, index_chunk=2)
    tc.encode(imgs)
    for use_index in (False, True):
        out = torch.zeros_like(imgs)
        tc.decode(out, use_index=use_index)
        assert torch.equal(out, imgs), "use_index=%s" % use_index
        assert qb3.lib.qb3x_last_decode_status(tc.d) == 0
