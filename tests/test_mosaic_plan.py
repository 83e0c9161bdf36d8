"""The mosaic calls' geometry and refusals (include/qb3x.h, "Mosaics"), no GPU: qb3x_mosaic_tiles against the plain statement of
tests/qb3_mosaic.py, and every refused call of qb3x_encode_mosaic / qb3x_decode_mosaic returning 0 with nothing written."""
import ctypes as C

import numpy as np
import pytest

from qb3_mosaic import cut, grid, paste

QB3E_EINV = 1
_sz = C.c_size_t


def test_cut_and_paste_agree():
    rng = np.random.default_rng(3)
    for (W, H, b, tw, th) in [(100, 70, 3, 32, 32), (64, 64, 1, 32, 32), (20, 9, 2, 32, 32), (33, 17, 3, 8, 16)]:
        r = rng.integers(0, 255, (H, W, b), dtype=np.uint8)
        t = cut(r, tw, th)
        tx, ty = grid(W, H, tw, th)
        assert t.shape == (tx * ty, th, tw, b)
        assert np.array_equal(paste(t, W, H), r)
        last = t[-1]                                    # the corner tile repeats the raster's last pixel
        assert np.array_equal(last[-1, -1], r[-1, -1])
        assert np.array_equal(t[0, 0, 0], r[0, 0])


def test_mosaic_tiles_matches_the_grid(qb3):
    L = qb3.lib
    sizes = [1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 100, 1100, 16000, 16384, 65536]
    tiles = [1, 4, 5, 32, 34, 512, 65536]
    for W in sizes:
        for H in (1, 9, 64, 65, 15000):
            for tw in tiles:
                for th in (4, 18, 32, 512):
                    tx, ty = _sz(77), _sz(77)
                    n = L.qb3x_mosaic_tiles(W, H, tw, th, C.byref(tx), C.byref(ty))
                    assert (tx.value, ty.value) == grid(W, H, tw, th), (W, H, tw, th)
                    assert n == tx.value * ty.value
                    assert L.qb3x_mosaic_tiles(W, H, tw, th, None, None) == n
    # exact multiples, a tile larger than the raster either way, a one-pixel overhang
    for (W, H, tw, th, want) in [(64, 64, 32, 32, (2, 2)), (20, 9, 32, 32, (1, 1)), (20, 70, 32, 32, (1, 3)), (100, 9, 32, 32, (4, 1)),
                                 (65, 33, 32, 32, (3, 2)), (64, 33, 32, 32, (2, 2))]:
        tx, ty = _sz(), _sz()
        assert L.qb3x_mosaic_tiles(W, H, tw, th, C.byref(tx), C.byref(ty)) == want[0] * want[1] and (tx.value, ty.value) == want
    for bad in [(0, 5, 4, 4), (5, 0, 4, 4), (5, 5, 0, 4), (5, 5, 4, 0)]:
        tx, ty = _sz(77), _sz(77)
        assert L.qb3x_mosaic_tiles(*bad, C.byref(tx), C.byref(ty)) == 0
        assert (tx.value, ty.value) == (77, 77)


def _buffers(n, pitch):
    dst = np.full(n * pitch + 8, 0xA5, dtype=np.uint8)
    sizes = (_sz * n)(*([12345] * n))
    return dst, sizes


def test_encode_mosaic_refusals(qb3):
    """everything refused is refused before anything is launched or written: 0 tiles, QB3E_EINV, the destination untouched"""
    L = qb3.lib
    W, H, b, tw, th = 100, 70, 3, 32, 32
    raster = np.zeros((H, W, b), dtype=np.uint8)
    n, pitch = 12, 4096
    vp = C.c_void_p

    def attempt(d_raster, W_, H_, stride, d_dst, dst_pitch, sizes, what):
        p = L.qb3_create_encoder(tw, th, b, qb3.QB3_U8)
        assert p
        try:
            assert L.qb3_get_encoder_state(p) == 0
            k = L.qb3x_encode_mosaic(p, d_raster, W_, H_, stride, d_dst, dst_pitch, None, sizes, None)
            assert k == 0, what
            assert L.qb3_get_encoder_state(p) == QB3E_EINV, what
        finally:
            L.qb3_destroy_encoder(p)

    dst, sizes = _buffers(n, pitch)
    base = dst.ctypes.data + (-dst.ctypes.data % 4)
    src = vp(raster.ctypes.data)
    attempt(None, W, H, 0, vp(base), pitch, sizes, "d_raster == NULL")
    attempt(src, 0, H, 0, vp(base), pitch, sizes, "W == 0")
    attempt(src, W, 0, 0, vp(base), pitch, sizes, "H == 0")
    attempt(src, W, H, W * b - 1, vp(base), pitch, sizes, "stride below W * bands")
    attempt(src, W, H, 1, vp(base), pitch, sizes, "stride of one value")
    # what qb3x_encode_tiles refuses
    attempt(src, W, H, 0, None, pitch, sizes, "d_dst == NULL")
    attempt(src, W, H, 0, vp(base), pitch + 2, sizes, "dst_pitch not a multiple of 4")
    attempt(src, W, H, 0, vp(base + 1), pitch, sizes, "d_dst not on a dword")
    attempt(src, W, H, 0, vp(base), pitch, None, "sizes == NULL")
    assert (dst == 0xA5).all() and list(sizes) == [12345] * n
    assert L.qb3x_encode_mosaic(None, src, W, H, 0, vp(base), pitch, None, sizes, None) == 0


def test_decode_mosaic_refusals(qb3, oracle):
    L = qb3.lib
    W, H, b, tw, th = 100, 70, 3, 32, 32
    tile = oracle.generate(tw, th, b, 0, "NOISY3", 1)
    c = np.ascontiguousarray(oracle.encode(tile, 0, 8))
    dims = (_sz * 3)()
    p = L.qb3_read_start(c.ctypes.data, c.size, dims)
    assert p and L.qb3_read_info(p)
    vp = C.c_void_p
    n, pitch = 12, 4096
    out = np.full(H * (W * b + 7) + 16, 0xA5, dtype=np.uint8)
    src = np.zeros(n * pitch + 8, dtype=np.uint8)
    sbase = src.ctypes.data + (-src.ctypes.data % 4)
    sizes = (_sz * n)(*([c.size] * n))
    try:
        for args, what in [((vp(sbase), pitch, sizes, W, H, None, 0), "d_raster == NULL"),
                           ((vp(sbase), pitch, sizes, 0, H, vp(out.ctypes.data), 0), "W == 0"),
                           ((vp(sbase), pitch, sizes, W, 0, vp(out.ctypes.data), 0), "H == 0"),
                           ((vp(sbase), pitch, sizes, W, H, vp(out.ctypes.data), W * b - 1), "stride below W * bands"),
                           ((None, pitch, sizes, W, H, vp(out.ctypes.data), 0), "d_src == NULL"),
                           ((vp(sbase), pitch + 1, sizes, W, H, vp(out.ctypes.data), 0), "src_pitch not a multiple of 4"),
                           ((vp(sbase + 2), pitch, sizes, W, H, vp(out.ctypes.data), 0), "d_src not on a dword"),
                           ((vp(sbase), pitch, None, W, H, vp(out.ctypes.data), 0), "sizes == NULL")]:
            assert L.qb3x_decode_mosaic(p, *args, None, None) == 0, what
        assert L.qb3x_decode_mosaic(None, vp(sbase), pitch, sizes, W, H, vp(out.ctypes.data), 0, None, None) == 0
        assert (out == 0xA5).all()
    finally:
        L.qb3_destroy_decoder(p)


def test_binding_knows_the_mosaic_calls(qb3):
    for name in ("qb3x_mosaic_tiles", "qb3x_encode_mosaic", "qb3x_decode_mosaic"):
        assert name in qb3.EXPORTED
    from qb3_amd import device
    assert hasattr(device, "MosaicCoder")
