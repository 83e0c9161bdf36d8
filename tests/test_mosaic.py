"""qb3x_encode_mosaic / qb3x_decode_mosaic on the GPU (include/qb3x.h, "Mosaics"): a raster in device memory coded as a grid of tiles
where it lies and decoded back into place.  The statement of the contract is tests/qb3_mosaic.py; the byte reference is the oracle
(and qb3x_encode_tiles on the tiles cut on the host, which must write the same containers).  Shapes are the smallest at which each
route can go wrong: a 4 x 3 grid has tiles inside, a right column, a bottom row and the corner."""
import ctypes as C
import os

import numpy as np
import pytest

from qb3_mosaic import cut, grid, paste

pytestmark = pytest.mark.gpu

_sz = C.c_size_t
_vp = C.c_void_p
FTL, BASE, BEST, CF, RLE = 8, 4, 7, 1, 2
GUARD = 3                       # rows of 0xA5 in front of and behind the raster


@pytest.fixture(scope="module")
def torch_():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    return torch


class Embedded:
    """a raster inside a device buffer of 0xA5: GUARD rows in front and behind, `pad` values between its rows, `offset` values in front"""

    def __init__(self, torch, raster, pad, offset=0, fill_only=False):
        H, W, b = raster.shape
        self.tsz = raster.itemsize
        self.stride = W * b + pad                       # values
        self.start = (GUARD * self.stride + offset) * self.tsz
        host = np.full((H + 2 * GUARD) * self.stride * self.tsz + offset * self.tsz + 64, 0xA5, dtype=np.uint8)
        self.expect = host.copy()
        rows = np.ascontiguousarray(raster).view(np.uint8).reshape(H, W * b * self.tsz)
        for y in range(H):
            at = self.start + y * self.stride * self.tsz
            self.expect[at:at + rows.shape[1]] = rows[y]
        self.dev = torch.from_numpy(host if fill_only else self.expect).cuda()
        self.ptr = self.dev.data_ptr() + self.start

    def host(self):
        return self.dev.cpu().numpy()


def make_encoder(qb3, tw, th, b, dt, mode, index_chunk=0, quanta=1):
    L = qb3.lib
    p = L.qb3_create_encoder(tw, th, b, dt)
    assert p
    L.qb3_set_encoder_mode(p, mode)
    if index_chunk:
        L.qb3x_set_encoder_index_chunk(p, index_chunk)
    if quanta > 1:
        assert L.qb3_set_encoder_quanta(p, quanta, False)
    return p


def encode_mosaic(qb3, torch, emb, raster, tw, th, dt, mode, index_chunk=0, quanta=1, want_index=False, keep=None):
    """returns (containers as host arrays, sizes, device buffer, pitch, index tensor)"""
    L = qb3.lib
    H, W, b = raster.shape
    p = keep or make_encoder(qb3, tw, th, b, dt, mode, index_chunk, quanta)
    tx, ty = grid(W, H, tw, th)
    n = tx * ty
    pitch = (L.qb3_max_encoded_size(p) + 3) // 4 * 4
    dst = torch.full((n * pitch,), 0x5A, dtype=torch.uint8, device="cuda")
    isz = L.qb3x_index_size(p) if want_index else 0
    index = torch.zeros(max(1, n * isz), dtype=torch.uint8, device="cuda") if want_index else None
    sizes = (_sz * n)()
    k = L.qb3x_encode_mosaic(p, _vp(emb.ptr), W, H, emb.stride, _vp(dst.data_ptr()), pitch, _vp(index.data_ptr()) if want_index else None, sizes, None)
    state = L.qb3_get_encoder_state(p)
    if not keep:
        L.qb3_destroy_encoder(p)
    assert k == n and state == 0, (k, n, state, qb3.last_error())
    host = dst.cpu().numpy()
    return [host[i * pitch:i * pitch + sizes[i]].copy() for i in range(n)], sizes, dst, pitch, index


def encode_tiles(qb3, torch, tiles, dt, mode, index_chunk=0, quanta=1):
    """the same tiles, cut on the host and given back to back to qb3x_encode_tiles"""
    L = qb3.lib
    n, th, tw, b = tiles.shape
    p = make_encoder(qb3, tw, th, b, dt, mode, index_chunk, quanta)
    pitch = (L.qb3_max_encoded_size(p) + 3) // 4 * 4
    src = torch.from_numpy(np.ascontiguousarray(tiles).view(np.uint8).reshape(-1)).cuda()
    dst = torch.zeros(n * pitch, dtype=torch.uint8, device="cuda")
    sizes = (_sz * n)()
    k = L.qb3x_encode_tiles(p, _vp(src.data_ptr()), n, tiles[0].nbytes, _vp(dst.data_ptr()), pitch, None, sizes, None)
    L.qb3_destroy_encoder(p)
    assert k == n
    host = dst.cpu().numpy()
    return [host[i * pitch:i * pitch + sizes[i]].copy() for i in range(n)]


def decode_mosaic(qb3, torch, dst, pitch, sizes, raster, pad, offset=0, index=None, compat=None):
    """decodes into a fresh 0xA5 buffer; asserts every pixel and every byte around the raster; returns the decoder for the caller to close"""
    L = qb3.lib
    H, W, b = raster.shape
    out = Embedded(torch, raster, pad, offset, fill_only=True)
    dims = (_sz * 3)()
    d = L.qb3x_read_start_device(_vp(dst.data_ptr()), int(sizes[0]), dims, None)
    assert d, qb3.last_error()
    if compat is not None:
        L.qb3x_set_decoder_compat(d, compat)
    n = len(sizes)
    k = L.qb3x_decode_mosaic(d, _vp(dst.data_ptr()), pitch, sizes, W, H, _vp(out.ptr), out.stride, _vp(index.data_ptr()) if index is not None else None, None)
    ok = [L.qb3x_decode_tile_ok(d, i) for i in range(n)]
    assert k == n and all(ok), (k, ok, qb3.last_error())
    got = out.host()
    at = out.start
    rows = np.ascontiguousarray(raster).view(np.uint8).reshape(H, -1)
    for y in range(H):
        a = at + y * out.stride * out.tsz
        assert np.array_equal(got[a:a + rows.shape[1]], rows[y]), "row %d" % y
    assert np.array_equal(got, out.expect), "a byte outside the raster's rows was written"
    return d


def round_trip(qb3, oracle, torch, raster, tw, th, dt, mode, pad=7, offset=0, against_oracle=True, cband=None, compat=None, index_chunk=0):
    H, W, b = raster.shape
    emb = Embedded(torch, raster, pad, offset)
    got, sizes, dst, pitch, _ = encode_mosaic(qb3, torch, emb, raster, tw, th, dt, mode, index_chunk)
    assert np.array_equal(emb.host(), emb.expect), "the encoder wrote to the raster"
    tiles = cut(raster, tw, th)
    ref = encode_tiles(qb3, torch, tiles, dt, mode, index_chunk)
    for k in range(len(tiles)):
        assert len(got[k]) == len(ref[k]) and np.array_equal(got[k], ref[k]), "tile %d differs from qb3x_encode_tiles'" % k
        if against_oracle:
            want = oracle.encode(tiles[k], dt, mode, cband=cband)
            assert len(got[k]) == len(want) and np.array_equal(got[k], want), "tile %d differs from the oracle's" % k
    d = decode_mosaic(qb3, torch, dst, pitch, sizes, raster, pad, offset, compat=compat)
    qb3.lib.qb3_destroy_decoder(d)
    return got


def profile(qb3):
    from qb3_amd import device as qdev
    return qdev


def test_bytes_u8x3_ftl(qb3, oracle, torch_):
    """100 x 70 in 32 x 32 tiles: a 3 x 2 sub-grid inside, a right column 4 pixels wide, a bottom row 6 pixels high, the corner"""
    raster = oracle.generate(100, 70, 3, 0, "NOISY3", 11)
    assert grid(100, 70, 32, 32) == (4, 3)
    got = round_trip(qb3, oracle, torch_, raster, 32, 32, 0, FTL)
    assert len(got) == 12


@pytest.mark.parametrize("case", [(100, 70, 3, 0, 34, 18, 7, 0), (61, 35, 1, 5, 12, 8, 3, 1)], ids=["u8x3-34x18", "i32-offset"])
def test_tile_rows_not_dword_aligned(qb3, oracle, torch_, case):
    """a column pitch of 102 bytes; an int32 raster that starts one value off"""
    W, H, b, dt, tw, th, pad, offset = case
    raster = oracle.generate(W, H, b, dt, "NOISY3" if dt == 0 else "DEM", 12)
    round_trip(qb3, oracle, torch_, raster, tw, th, dt, FTL, pad=pad, offset=offset)


@pytest.mark.parametrize("shape", [(64, 64), (20, 9), (32, 70), (100, 32)], ids=lambda s: "%dx%d" % s)
def test_degenerate_grids(qb3, oracle, torch_, shape):
    W, H = shape
    raster = oracle.generate(W, H, 3, 0, "NOISY3", 13)
    qdev = profile(qb3)
    qdev.profile_enable(1)
    qdev.profile_reset()
    try:
        round_trip(qb3, oracle, torch_, raster, 32, 32, 0, FTL)
        rep = qdev.profile_report()
    finally:
        qdev.profile_enable(0)
    if shape == (64, 64):           # no edge tile: neither copy runs
        assert "mosaic_pad" not in rep and "mosaic_crop" not in rep, rep
    else:
        assert rep["mosaic_pad"][1] == 1 and rep["mosaic_crop"][1] == 1, rep


@pytest.mark.parametrize("case", [
    (130, 67, 8, 2, 64, 32, BASE, "LANDSAT16"),
    (130, 67, 3, 2, 64, 32, CF, "LANDSAT16"),
    (100, 36, 5, 0, 32, 16, FTL, "NOISY3"),
    (100, 70, 3, 0, 32, 32, BEST, "NOISY3"),
    (64, 44, 2, 7, 32, 16, FTL, "DEM"),
], ids=["u16x8-base", "u16x3-cf", "u8x5-ftl", "u8x3-best", "i64x2-ftl"])
def test_other_kernel_families(qb3, oracle, torch_, case):
    W, H, b, dt, tw, th, mode, gen = case
    raster = oracle.generate(W, H, b, dt, gen, 14)
    cband = None if b in (1, 3, 4) else list(range(b))
    round_trip(qb3, oracle, torch_, raster, tw, th, dt, mode, cband=cband, compat=0 if b == 5 else None)


def test_tables(qb3, oracle, torch_):
    """containers with restart tables: the bytes of qb3x_encode_tiles with the switch on; decoded from the tables alone, and with the
    caller's index array"""
    raster = oracle.generate(100, 70, 3, 0, "NOISY3", 15)
    emb = Embedded(torch_, raster, 7)
    got, sizes, dst, pitch, _ = encode_mosaic(qb3, torch_, emb, raster, 32, 32, 0, FTL, index_chunk=2)
    ref = encode_tiles(qb3, torch_, cut(raster, 32, 32), 0, FTL, index_chunk=2)
    plain = encode_tiles(qb3, torch_, cut(raster, 32, 32), 0, FTL)
    for k in range(12):
        assert np.array_equal(got[k], ref[k]), k
        assert len(got[k]) > len(plain[k]) and b"ix" in bytes(got[k][:64])
    qdev = profile(qb3)
    qdev.profile_enable(1)
    qdev.profile_reset()
    try:
        d = decode_mosaic(qb3, torch_, dst, pitch, sizes, raster, 7)
        rep = qdev.profile_report()
    finally:
        qdev.profile_enable(0)
    qb3.lib.qb3_destroy_decoder(d)
    assert not any(name.startswith("dec_index") for name in rep), rep
    # the caller's index array, one entry a container
    got2, sizes2, dst2, pitch2, index = encode_mosaic(qb3, torch_, emb, raster, 32, 32, 0, FTL, want_index=True)
    for k in range(12):
        assert np.array_equal(got2[k], plain[k]), k
    d = decode_mosaic(qb3, torch_, dst2, pitch2, sizes2, raster, 7, index=index)
    qb3.lib.qb3_destroy_decoder(d)


def test_stored_tiles(qb3, oracle, torch_):
    """incompressible data in tile 0 and in the corner tile: both raw-stored, the batch decodes around them, the handle keeps its mode"""
    W, H = 127, 95
    raster = oracle.generate(W, H, 3, 0, "NOISY3", 5).copy()
    rnd = oracle.generate(W, H, 3, 0, "RANDOM", 6)
    raster[:32, :32] = rnd[:32, :32]
    raster[64:, 96:] = rnd[64:, 96:]
    emb = Embedded(torch_, raster, 7)
    p = make_encoder(qb3, 32, 32, 3, 0, FTL)
    try:
        got, sizes, dst, pitch, _ = encode_mosaic(qb3, torch_, emb, raster, 32, 32, 0, FTL, keep=p)
        tiles = cut(raster, 32, 32)
        ref = encode_tiles(qb3, torch_, tiles, 0, FTL)
        for k in range(12):
            assert np.array_equal(got[k], ref[k]) and np.array_equal(got[k], oracle.encode(tiles[k], 0, FTL)), k
        assert [int(c[10]) for c in got] == [255] + [8] * 10 + [255]
        d = decode_mosaic(qb3, torch_, dst, pitch, sizes, raster, 7)
        qb3.lib.qb3_destroy_decoder(d)
        # the same handle again: still in its mode
        calm = oracle.generate(W, H, 3, 0, "NOISY3", 7)
        emb2 = Embedded(torch_, calm, 7)
        got2, _, _, _, _ = encode_mosaic(qb3, torch_, emb2, calm, 32, 32, 0, FTL, keep=p)
        assert all(int(c[10]) == 8 for c in got2)
        assert np.array_equal(got2[5], oracle.encode(cut(calm, 32, 32)[5], 0, FTL))
    finally:
        qb3.lib.qb3_destroy_encoder(p)


@pytest.mark.parametrize("case", [(3, RLE, 1, "CONST"), (1, FTL, 3, "NOISY3")], ids=["rle-const", "quanta3"])
def test_non_batchable_handles(qb3, oracle, torch_, case):
    """handles the batch does not take go tile by tile: the bytes of the loop over the cut tiles, the raster back"""
    b, mode, quanta, gen = case
    W, H = 70, 40
    raster = oracle.generate(W, H, b, 0, gen, 16)
    emb = Embedded(torch_, raster, 7)
    got, sizes, dst, pitch, _ = encode_mosaic(qb3, torch_, emb, raster, 32, 32, 0, mode, quanta=quanta)
    tiles = cut(raster, 32, 32)
    ref = encode_tiles(qb3, torch_, tiles, 0, mode, quanta=quanta)
    back = []
    for k in range(len(tiles)):
        assert np.array_equal(got[k], ref[k]), k
        want = oracle.encode(tiles[k], 0, mode, quanta=quanta)
        assert np.array_equal(got[k], want), k
        px, dims, _, _ = oracle.decode(want)
        back.append(px.reshape(32, 32, b))
    expect = paste(np.stack(back), W, H)            # (quanta: the dequantised values)
    if quanta == 1:
        assert np.array_equal(expect, raster)
    d = decode_mosaic(qb3, torch_, dst, pitch, sizes, expect, 7)
    qb3.lib.qb3_destroy_decoder(d)


def test_launch_sets(qb3, oracle, torch_):
    """the launches do not grow with the tile count: at most three sets (inside, bottom row, right column), one pad, one crop"""
    qdev = profile(qb3)
    counts = []
    for (W, H) in [(100, 70), (228, 134)]:
        raster = oracle.generate(W, H, 3, 0, "NOISY3", 17)
        emb = Embedded(torch_, raster, 7)
        qdev.profile_enable(1)
        qdev.profile_reset()
        try:
            got, sizes, dst, pitch, _ = encode_mosaic(qb3, torch_, emb, raster, 32, 32, 0, FTL)
            enc = qdev.profile_report()
            qdev.profile_reset()
            d = decode_mosaic(qb3, torch_, dst, pitch, sizes, raster, 7)
            dec = qdev.profile_report()
        finally:
            qdev.profile_enable(0)
        qb3.lib.qb3_destroy_decoder(d)
        assert len(got) == grid(W, H, 32, 32)[0] * grid(W, H, 32, 32)[1]
        assert enc["enc_units"][1] <= 3 and enc["mosaic_pad"][1] == 1 and "mosaic_crop" not in enc, enc
        assert dec["dec_units"][1] <= 3 and dec["mosaic_crop"][1] == 1 and "mosaic_pad" not in dec, dec
        counts.append((enc["enc_units"][1], dec["dec_units"][1]))
    assert len(got) == 40 and counts[0] == counts[1], counts


def test_mosaic_coder(qb3, oracle, torch_):
    """device.MosaicCoder on a strided 2-D view"""
    from qb3_amd import device as qdev
    W, H, b = 100, 70, 3
    raster = oracle.generate(W, H, b, 0, "NOISY3", 18)
    wide = torch_.full((H, W * b + 9), 0xA5, dtype=torch_.uint8, device="cuda")
    wide[:, :W * b] = torch_.from_numpy(raster.reshape(H, W * b)).cuda()
    mc = qdev.MosaicCoder(W, H, b, 0, tile=(32, 32))
    sizes = mc.encode(wide[:, :W * b])
    tiles = cut(raster, 32, 32)
    assert (mc.tx, mc.ty, mc.n) == (4, 3, 12)
    for k in (0, 3, 8, 11):
        assert np.array_equal(mc.container(k).cpu().numpy(), oracle.encode(tiles[k], 0, FTL)) and sizes[k] == mc.sizes[k]
    out = torch_.full_like(wide, 0x11)
    mc.decode(out[:, :W * b])
    assert torch_.equal(out[:, :W * b], wide[:, :W * b]) and bool((out[:, W * b:] == 0x11).all())
    tight = torch_.zeros((H, W, b), dtype=torch_.uint8, device="cuda")
    mc.decode(tight)
    assert np.array_equal(tight.cpu().numpy(), raster)
    mc.close()


def test_tile_batcher_tool_writes_the_mosaic(qb3, oracle, torch_, tmp_path):
    """tools/qb3tiles.cpp over the mosaic calls: the .qts file is, byte for byte, the one assembled here from qb3x_encode_tiles of the
    tiles cut on the host; the raster comes back"""
    import subprocess
    W, H, b, T = 1100, 700, 3, 512
    tool = os.path.join(os.path.dirname(qb3.LIB_PATH), "qb3tiles")
    raster = oracle.generate(W, H, b, 0, "NOISY3", 19)
    pnm = tmp_path / "in.pnm"
    pnm.write_bytes(b"P6\n%d %d\n255\n" % (W, H) + raster.tobytes())
    r = subprocess.run([tool, "-e", "-t", str(T), str(pnm), str(tmp_path / "out.qts")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ref = encode_tiles(qb3, torch_, cut(raster, T, T), 0, FTL)
    tx, ty = grid(W, H, T, T)
    head = b"QTS1" + np.array([W, H, b, 0, T, tx, ty], dtype=np.uint32).tobytes()
    off = len(head) + 16 * len(ref)
    tab = []
    for c in ref:
        tab += [off, len(c)]
        off += len(c)
    want = head + np.array(tab, dtype=np.uint64).tobytes() + b"".join(c.tobytes() for c in ref)
    assert (tmp_path / "out.qts").read_bytes() == want
    r = subprocess.run([tool, "-d", str(tmp_path / "out.qts"), str(tmp_path / "back.pnm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "back.pnm").read_bytes() == pnm.read_bytes()
