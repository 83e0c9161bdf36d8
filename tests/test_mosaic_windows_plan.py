"""The mosaic-window calls' geometry and refusals (include/qb3x.h, "Mosaic windows"), no GPU: qb3x_mosaic_window_tiles against a count by
enumeration over the grids of tests/qb3_mosaic.py, and every refused call of qb3x_decode_mosaic_windows returning 0 with device pointers
that are sentinels -- nothing may be dereferenced, launched or written."""
import ctypes as C
import os

import numpy as np
import pytest

from qb3_mosaic import grid
from qb3_mosaic_windows import Window, brute_tiles

_sz = C.c_size_t
_vp = C.c_void_p
NAMES = ("qb3x_mosaic_window_tiles", "qb3x_decode_mosaic_windows", "qb3x_last_mosaic_whole_tiles")
SENTINEL = 0x7f5a5a5a5a5a5000         # an address nothing lives at, on a dword


def test_binding_knows_the_mosaic_window_calls(qb3):
    for name in NAMES:
        assert name in qb3.EXPORTED and hasattr(qb3.lib, name)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qb3x.h")).read()
    for name in NAMES:
        assert name + "(" in text, name
    from qb3_amd import device
    assert hasattr(device.MosaicCoder, "decode_windows") and hasattr(device.MosaicCoder, "last_windows")


CASES = [(300, 80, 132, 36), (64, 64, 64, 64), (20, 9, 16, 16)]


def rects_of(W, H, tw, th):
    """one pixel, the whole raster, across one and two tile borders, inside an edge tile; then empty ones and ones outside"""
    tx, ty = grid(W, H, tw, th)
    good = [(0, 0, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, H), (W - 1, 0, 1, H), (0, H - 1, W, 1)]
    if tx > 1:
        good += [(tw - 1, 0, 2, 1), (tw - 1, 0, 2, min(H, 3)), ((tx - 1) * tw, 0, W - (tx - 1) * tw, 1)]
    if tx > 2:
        good += [(tw - 1, 0, tw + 2, 1)]
    if ty > 1:
        good += [(0, th - 1, 1, 2), (0, (ty - 1) * th, 1, H - (ty - 1) * th)]
    if ty > 2:
        good += [(0, th - 1, 1, th + 2)]
    if tx > 1 and ty > 1:
        good += [(tw - 1, th - 1, 2, 2), ((tx - 1) * tw, (ty - 1) * th, W - (tx - 1) * tw, H - (ty - 1) * th), (tw - 3, th - 2, W - tw + 3, H - th + 2)]
    bad = [(0, 0, 0, 1), (0, 0, 1, 0), (W, 0, 1, 1), (0, H, 1, 1), (W - 1, 0, 2, 1), (0, H - 1, 1, 2), (1, 1, W, H), (0, 0, 2 ** 64 - 1, 1), (2 ** 63, 0, 2 ** 63, 1)]
    return good, bad


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_window_tiles_matches_the_enumeration(qb3, case):
    L = qb3.lib
    W, H, tw, th = case
    good, bad = rects_of(W, H, tw, th)
    rng = np.random.default_rng(W * 31 + H)
    for _ in range(200):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        good.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    for r in good:
        tiles = brute_tiles(W, H, tw, th, *r)
        assert tiles, r
        v = [_sz(77) for _ in range(4)]
        n = L.qb3x_mosaic_window_tiles(W, H, tw, th, *r, *[C.byref(x) for x in v])
        i0, j0, i1, j1 = [x.value for x in v]
        assert n == len(tiles), (r, n, len(tiles))
        assert tiles == {(i, j) for j in range(j0, j1 + 1) for i in range(i0, i1 + 1)}, r
        assert L.qb3x_mosaic_window_tiles(W, H, tw, th, *r, None, None, None, None) == n
        assert L.qb3x_mosaic_window_tiles(W, H, tw, th, *r, None, C.byref(v[1]), None, None) == n and v[1].value == j0
    for r in bad:
        v = [_sz(77) for _ in range(4)]
        assert L.qb3x_mosaic_window_tiles(W, H, tw, th, *r, *[C.byref(x) for x in v]) == 0, r
        assert [x.value for x in v] == [77] * 4, r
    for sizes in [(0, H, tw, th), (W, 0, tw, th), (W, H, 0, th), (W, H, tw, 0)]:
        assert L.qb3x_mosaic_window_tiles(*sizes, 0, 0, 1, 1, None, None, None, None) == 0, sizes


def _handle(qb3, oracle, tw=32, th=32, b=3):
    tile = oracle.generate(tw, th, b, 0, "NOISY3", 1)
    c = np.ascontiguousarray(oracle.encode(tile, 0, 8))
    dims = (_sz * 3)()
    p = qb3.lib.qb3_read_start(c.ctypes.data, c.size, dims)
    assert p and qb3.lib.qb3_read_info(p)
    return p, c


def test_decode_mosaic_windows_refusals(qb3, oracle):
    """every pointer that would be read or written on the device is a sentinel: a refusal that came too late would fault here"""
    L = qb3.lib
    W, H, b, tw, th = 100, 70, 3, 32, 32
    p, c = _handle(qb3, oracle, tw, th, b)
    n, pitch = 12, 4096
    sizes = (_sz * n)(*([c.size] * n))
    src, dst = _vp(SENTINEL), SENTINEL + (1 << 30)
    ok = [Window(3, 4, 50, 40, dst, 0), Window(0, 0, W, H, dst + (1 << 20), W * b + 5)]

    def arr(ws):
        return (Window * len(ws))(*ws)

    def call(src_=src, pitch_=pitch, sizes_=sizes, W_=W, H_=H, wins=ok, n_=None):
        a = arr(wins) if wins is not None else None
        return L.qb3x_decode_mosaic_windows(p, src_, pitch_, sizes_, W_, H_, a, len(wins) if n_ is None else n_, None)

    try:
        # what qb3x_decode_mosaic refuses
        assert call(src_=None) == 0, "d_src == NULL"
        assert call(src_=_vp(SENTINEL + 2)) == 0, "d_src not on a dword"
        assert call(pitch_=pitch + 1) == 0, "src_pitch not a multiple of 4"
        assert call(sizes_=None) == 0, "sizes == NULL"
        assert call(W_=0) == 0 and call(H_=0) == 0, "an empty raster"
        assert call(W_=2 ** 32, wins=[ok[0]]) == 0 and call(H_=2 ** 32, wins=[ok[0]]) == 0, "a raster beyond 32 bits"
        # the batch
        assert L.qb3x_decode_mosaic_windows(p, src, pitch, sizes, W, H, None, 2, None) == 0, "wins == NULL"
        assert call(n_=0) == 0, "n == 0"
        assert L.qb3x_decode_mosaic_windows(p, src, pitch, sizes, W, H, arr(ok), 2 ** 20 + 1, None) == 0, "n > 2^20"
        # one bad window refuses the batch, wherever it stands
        for bad, what in [(Window(0, 0, 0, 5, dst, 0), "w == 0"), (Window(0, 0, 5, 0, dst, 0), "h == 0"),
                          (Window(W - 4, 0, 5, 5, dst, 0), "beyond the right edge"), (Window(0, H - 4, 5, 5, dst, 0), "beyond the bottom edge"),
                          (Window(W, 0, 1, 1, dst, 0), "x0 outside"), (Window(0, H, 1, 1, dst, 0), "y0 outside"),
                          (Window(2 ** 63, 0, 2 ** 63 + 2, 1, dst, 0), "x0 + w wraps"),
                          (Window(0, 0, 5, 5, None, 0), "dst == NULL"), (Window(0, 0, 5, 5, dst, 5 * b - 1), "stride below w * bands"),
                          (Window(0, 0, 5, 5, dst, 1), "a stride of one value")]:
            assert call(wins=[bad]) == 0, what
            assert call(wins=[ok[0], bad]) == 0 and call(wins=[bad, ok[1]]) == 0, what
        # more than 2^20 pieces: 2^18 windows of four tiles each and one more
        four = Window(tw - 1, th - 1, 2, 2, dst, 0)
        many = (Window * (2 ** 18 + 1))(*([four] * (2 ** 18 + 1)))
        assert L.qb3x_mosaic_window_tiles(W, H, tw, th, four.x0, four.y0, four.w, four.h, None, None, None, None) == 4
        assert L.qb3x_decode_mosaic_windows(p, src, pitch, sizes, W, H, many, 2 ** 18 + 1, None) == 0, "more than 2^20 pieces"
        assert L.qb3x_last_mosaic_whole_tiles(p) == 0
        assert L.qb3x_window_ok(p, 0) == 0
    finally:
        L.qb3_destroy_decoder(p)


def test_handle_not_ready_and_null(qb3, oracle):
    L = qb3.lib
    p, c = _handle(qb3, oracle)
    sizes = (_sz * 12)(*([c.size] * 12))
    wins = (Window * 1)(Window(0, 0, 5, 5, SENTINEL + 4096, 0))
    try:
        assert L.qb3x_decode_mosaic_windows(None, _vp(SENTINEL), 4096, sizes, 100, 70, wins, 1, None) == 0
        assert L.qb3x_last_mosaic_whole_tiles(None) == 0
        dims = (_sz * 3)()
        q = L.qb3_read_start(c.ctypes.data, c.size, dims)       # not past qb3_read_info
        assert q
        try:
            assert L.qb3x_decode_mosaic_windows(q, _vp(SENTINEL), 4096, sizes, 100, 70, wins, 1, None) == 0
        finally:
            L.qb3_destroy_decoder(q)
    finally:
        L.qb3_destroy_decoder(p)
