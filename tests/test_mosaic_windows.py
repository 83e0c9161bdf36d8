"""qb3x_decode_mosaic_windows on the GPU (include/qb3x.h, "Mosaic windows"): rectangles of a mosaic's raster from the tiles that hold them.
Expected bytes are the source raster's crop (lossless modes) or the crop of qb3x_decode_mosaic run with the same arguments on a second
handle; every destination lies in a 0xA5-filled buffer that is compared whole (tests/qb3_mosaic_windows.py).  Shapes are the smallest
at which each thing can go wrong."""
import ctypes as C

import numpy as np
import pytest

from qb3_mosaic import grid
from qb3_mosaic_windows import Mosaic, decode_windows, pieces
from qb3_window import open_handle, windows

pytestmark = pytest.mark.gpu

_sz = C.c_size_t
FTL, BASE, BEST, RLE = 8, 4, 7, 2
U8, I8, U16, I32 = 0, 1, 2, 5
PROFILE = "dec_window_mosaic"


@pytest.fixture(scope="module")
def torch_():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    return torch


@pytest.fixture(scope="module")
def rgb(qb3, oracle, torch_):
    """uint8 x 3, FTL, 300 x 80 in tiles of 132 x 36: 3 x 3 tiles of 33 blocks a row (a 64-block segment spans rows), a right column
    36 pixels wide and a bottom row 8 pixels high, both padded by replication when coded; level-2 tables.  Shared, never changed."""
    raster = oracle.generate(300, 80, 3, U8, "NOISY3", 21)
    m = Mosaic(qb3, torch_, raster, 132, 36, U8, FTL)
    assert all(int(m.host(k)[10]) == FTL for k in range(m.n))
    return m


def touched(m, rects):
    return {k for r in rects for (k, _, _, _, _) in pieces(m.W, m.H, m.tw, m.th, *r)}


def piece_segments(qb3, m, rects):
    """the sum of qb3x_window_segments over the pieces, each asked of a handle made from its own tile"""
    L, total, handles = qb3.lib, 0, {}
    try:
        for r in rects:
            for (k, x, y, w, h) in pieces(m.W, m.H, m.tw, m.th, *r):
                if k not in handles:
                    handles[k] = (open_handle(L, m.host(k))[0], m.host(k))      # (the array outlives the handle)
                n = L.qb3x_window_segments(handles[k][0], x, y, w, h, None)
                assert n
                total += n
    finally:
        for p, _ in handles.values():
            L.qb3_destroy_decoder(p)
    return total


def test_kernel_route_segments_straddling_block_rows(qb3, rgb):
    m = rgb
    rects = [(0, 0, 300, 80),           # the whole raster
             (10, 5, 50, 20),           # inside one tile
             (120, 3, 30, 20),          # across a vertical border
             (100, 20, 80, 30),         # across four tiles
             (250, 60, 50, 20),         # ends in the corner edge tile
             (299, 79, 1, 1),
             (140, 40, 33, 17),         # a wide stride
             (5, 37, 40, 9)]            # a destination on an odd address
    d = m.handle()
    try:
        r = decode_windows(m, d, rects, m.raster, pads=[0, 0, 0, 0, 0, 0, 11, 0], odd={7})
        assert r.n == len(rects) and r.paths == [1] * len(rects), (r.paths, r.error)
        assert not r.wrong and r.clean, r.wrong
        assert r.whole == 0
        assert r.segments == piece_segments(qb3, m, rects)
    finally:
        qb3.lib.qb3_destroy_decoder(d)


@pytest.mark.parametrize("bands", [1, 4])
def test_rows_that_start_where_segments_do(qb3, oracle, torch_, bands):
    """tiles of 256 x 16: 64 blocks a block row, every row starts a segment"""
    raster = oracle.generate(600, 40, bands, U8, "NOISY3", 22)
    m = Mosaic(qb3, torch_, raster, 256, 16, U8, BASE)
    assert (m.tx, m.ty) == (3, 3)
    rects = windows(600, 40, 23, 6) + [(250, 10, 20, 12), (255, 15, 2, 2)]
    d = m.handle()
    try:
        r = decode_windows(m, d, rects, raster)
        assert r.paths == [1] * len(rects), (r.paths, r.error)
        assert not r.wrong and r.clean, r.wrong
        assert r.whole == 0 and r.segments == piece_segments(qb3, m, rects)
    finally:
        qb3.lib.qb3_destroy_decoder(d)


def test_many_pieces_one_launch(qb3, oracle, torch_):
    """72 tiles of 16 x 16, one window over everything and 64 small ones: more pieces than one level of the search, several windows in a tile"""
    from qb3_amd import device as qdev
    W, H = 144, 128
    raster = oracle.generate(W, H, 3, U8, "NOISY3", 24)
    m = Mosaic(qb3, torch_, raster, 16, 16, U8, FTL)
    assert m.n == 72
    rng = np.random.default_rng(25)
    rects = [(0, 0, W, H)]
    for _ in range(64):
        w, h = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        rects.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    assert sum(len(pieces(W, H, 16, 16, *r)) for r in rects) > 72 + 64
    d = m.handle()
    qdev.profile_enable(1)
    qdev.profile_reset()
    try:
        r = decode_windows(m, d, rects, raster)
        rep = qdev.profile_report()
    finally:
        qdev.profile_enable(0)
        qb3.lib.qb3_destroy_decoder(d)
    assert r.paths == [1] * len(rects), (r.paths, r.error)
    assert not r.wrong and r.clean, r.wrong
    assert rep[PROFILE][1] == 1 and "mosaic_crop" not in rep and "dec_units" not in rep, rep


KINDS = [
    ("u16x2-ftl", 2, U16, FTL, "LANDSAT16", 2, 1, (32, 32), (100, 70)),
    ("i32", 1, I32, FTL, "DEM", 2, 1, (32, 32), (100, 70)),
    ("u8x3-best", 3, U8, BEST, "NOISY3", 2, 1, (32, 32), (100, 70)),
    ("u8x5", 5, U8, FTL, "NOISY3", 2, 1, (32, 32), (100, 70)),
    ("rle-const", 3, U8, RLE, "CONST", 2, 1, (32, 32), (100, 70)),
    ("no-tables", 3, U8, FTL, "NOISY3", 0, 1, (32, 32), (100, 70)),
    ("quanta3-i8", 1, I8, FTL, "NOISY3", 2, 3, (32, 32), (100, 70)),
    ("3-wide-tiles", 3, U8, FTL, "NOISY3", 2, 1, (3, 16), (10, 40)),
]


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_whole_tile_route_by_kind(qb3, oracle, torch_, kind):
    _, b, dt, mode, gen, chunk, quanta, (tw, th), (W, H) = kind
    raster = oracle.generate(W, H, b, dt, gen, 26)
    m = Mosaic(qb3, torch_, raster, tw, th, dt, mode, index_chunk=chunk, quanta=quanta)
    expect, ok = m.whole(compat=0 if b == 5 else None)
    assert all(ok)
    if quanta == 1:
        assert np.array_equal(expect, raster)
    tx, ty = grid(W, H, tw, th)
    rects = [(tw - 2, th - 3, min(tw, W - tw) + 1, min(th, H - th) + 2),                # across four tiles
             ((tx - 1) * tw - 1, (ty - 1) * th - 1, W - (tx - 1) * tw + 1, H - (ty - 1) * th + 1),     # into the corner edge tile
             (1, 2, 2, 5), (1, 1, 1, 1)]                                                # two in tile 0
    d = m.handle(compat=0 if b == 5 else None)
    try:
        r = decode_windows(m, d, rects, expect, pads=[0, 3, 0, 0])
        assert r.paths == [3] * len(rects), (r.paths, r.error)
        assert not r.wrong and r.clean, r.wrong
        assert r.whole == len(touched(m, rects)), (r.whole, sorted(touched(m, rects)))
    finally:
        qb3.lib.qb3_destroy_decoder(d)


def test_mixed_tile_kinds(qb3, oracle, torch_):
    """noise in tile 0 and in the corner tile: both fall to STORED among coded tiles.  A window across both kinds has its kernel
    pieces and its whole-tile pieces side by side"""
    W, H = 127, 95
    raster = oracle.generate(W, H, 3, U8, "NOISY3", 5).copy()
    rnd = oracle.generate(W, H, 3, U8, "RANDOM", 6)
    raster[:32, :32] = rnd[:32, :32]
    raster[64:, 96:] = rnd[64:, 96:]
    m = Mosaic(qb3, torch_, raster, 32, 32, U8, FTL)
    assert [int(m.host(k)[10]) for k in range(12)] == [255] + [FTL] * 10 + [255]
    rects = [(16, 16, 40, 40),          # tiles 0 (stored), 1, 4, 5
             (40, 40, 20, 20),          # tile 5 alone
             (100, 70, 27, 25),         # the corner tile alone (stored)
             (60, 60, 60, 30)]          # tiles 5, 6, 7, 9, 10 and the corner
    d = m.handle()
    try:
        # tile 0 is the stored one: its handle has no table, everything goes whole
        r = decode_windows(m, d, rects, raster)
        assert r.paths == [3] * 4 and not r.wrong and r.clean, (r.paths, r.wrong, r.error)
        assert r.whole == len(touched(m, rects))
    finally:
        qb3.lib.qb3_destroy_decoder(d)
    # the same pixels mirrored, so that tile 0 is a coded one: the stored tiles are now tile 3 (an edge tile) and tile 8, and the
    # handle takes the kernel route for everything else
    raster2 = np.ascontiguousarray(raster[:, ::-1])
    m2 = Mosaic(qb3, torch_, raster2, 32, 32, U8, FTL)
    kinds = [int(m2.host(k)[10]) for k in range(12)]
    stored = {k for k in range(12) if kinds[k] == 255}
    assert kinds[0] == FTL and stored, kinds
    rects2 = [(W - 16 - 40, 16, 40, 40), (40, 40, 20, 20), (0, 70, 27, 25), (10, 60, 60, 30)]
    d = m2.handle()
    try:
        r = decode_windows(m2, d, rects2, raster2)
        want = [3 if touched(m2, [rc]) & stored else 1 for rc in rects2]
        assert 1 in want and 3 in want
        assert r.paths == want and not r.wrong and r.clean, (r.paths, want, r.wrong, r.error)
        assert r.whole == len(touched(m2, rects2) & stored)
    finally:
        qb3.lib.qb3_destroy_decoder(d)


def table_at(m, k):
    """offset of tile k's first "ix" chunk in its container"""
    head = bytes(m.host(k)[:96])
    at = head.index(b"ix", 11)
    assert at == bytes(m.host(0)[:96]).index(b"ix", 11)
    return at


DAMAGED = 4                             # the middle tile of the 3 x 3
AROUND = [(140, 40, 50, 20),            # inside the damaged tile
          (100, 20, 80, 30),            # across tiles 0, 1, 3 and the damaged one
          (10, 5, 50, 20),              # beside it: tile 0
          (270, 75, 30, 5)]             # the corner tile


def damaged_copy(m, torch_, at, values):
    """m with bytes of the damaged tile overwritten in a copy of the containers (the fixture stays as it is)"""
    import copy
    c = copy.copy(m)
    c.dst = m.dst.clone()
    for i, v in enumerate(values):
        c.dst[DAMAGED * m.pitch + at + i] = v
    return c


@pytest.mark.parametrize("what", ["table-byte", "ix-tag"])
def test_damage_costs_time_not_pixels(qb3, rgb, torch_, what):
    """data the decoder is built to refuse: a byte flipped inside a table chunk of one tile, or its "ix" tag overwritten.  Windows
    touching the tile get the right pixels by path 3 with one tile decoded whole; windows beside it stay on path 1"""
    t = table_at(rgb, DAMAGED)
    if what == "table-byte":
        m = damaged_copy(rgb, torch_, t + 12 + 9, [int(rgb.host(DAMAGED)[t + 12 + 9]) ^ 0x40])
    else:
        m = damaged_copy(rgb, torch_, t, [ord("q"), ord("q")])
    d = m.handle()
    try:
        r = decode_windows(m, d, AROUND, rgb.raster)
        assert r.paths == [3, 3, 1, 1], (r.paths, r.error)
        assert not r.wrong and r.clean, r.wrong
        assert r.whole == 1
    finally:
        qb3.lib.qb3_destroy_decoder(d)


def test_a_tile_cut_to_half(qb3, rgb):
    """sizes[k] halved for one tile: the bytes are the crop of qb3x_decode_mosaic given the same sizes, tile by tile as it reports them"""
    m = rgb
    sizes = (_sz * m.n)(*list(m.sizes))
    sizes[DAMAGED] = m.sizes[DAMAGED] // 2
    expect, ok = m.whole(sizes=sizes)
    assert ok == [1] * DAMAGED + [ok[DAMAGED]] + [1] * (m.n - DAMAGED - 1)
    d = m.handle()
    try:
        r = decode_windows(m, d, AROUND, expect, sizes=sizes)
        assert r.paths[2:] == [1, 1], (r.paths, r.error)
        assert r.paths[:2] == ([3, 3] if ok[DAMAGED] else [0, 0]), (r.paths, ok[DAMAGED])
        assert not r.wrong and r.clean, r.wrong
        assert r.whole == 1
    finally:
        qb3.lib.qb3_destroy_decoder(d)


@pytest.mark.parametrize("bands", [3, 5])
def test_compat_flag_agrees_with_decode_mosaic(qb3, oracle, torch_, rgb, bands):
    if bands == 3:
        m = rgb
    else:
        m = Mosaic(qb3, torch_, oracle.generate(100, 70, 5, U8, "NOISY3", 27), 32, 32, U8, FTL)
    expect, ok = m.whole(compat=qb3.QB3X_REF_CBAND0)
    assert all(ok)
    rects = [(0, 0, m.W, m.H), (m.tw - 5, m.th - 5, 30, 20)]
    d = m.handle(compat=qb3.QB3X_REF_CBAND0)
    try:
        r = decode_windows(m, d, rects, expect)
        assert r.n == 2 and not r.wrong and r.clean, (r.paths, r.wrong, r.error)
    finally:
        qb3.lib.qb3_destroy_decoder(d)


def test_mosaic_coder_decode_windows(qb3, oracle, torch_):
    from qb3_amd import device as qdev
    W, H, b = 100, 70, 3
    raster = oracle.generate(W, H, b, U8, "NOISY3", 28)
    mc = qdev.MosaicCoder(W, H, b, U8, tile=(32, 32), index_chunk=2)
    try:
        mc.encode(torch_.from_numpy(raster).cuda())
        rects = [(0, 0, W, H), (30, 30, 5, 5), (90, 60, 10, 10)]
        outs = mc.decode_windows(rects)
        for (x0, y0, w, h), o in zip(rects, outs):
            assert tuple(o.shape) == (h, w, b) and np.array_equal(o.cpu().numpy(), raster[y0:y0 + h, x0:x0 + w])
        assert mc.last_windows() == ([True] * 3, [1] * 3, 0)
        mine = [torch_.full((w * h * b + 8,), 0xA5, dtype=torch_.uint8, device="cuda") for (_, _, w, h) in rects]
        again = mc.decode_windows(rects, out=mine)
        for (x0, y0, w, h), o, buf in zip(rects, again, mine):
            assert np.array_equal(o.cpu().numpy(), raster[y0:y0 + h, x0:x0 + w]) and bool((buf[w * h * b:] == 0xA5).all())
    finally:
        mc.close()
