"""Helpers of the window-decode tests (test_window_plan.py, test_window_decode.py): the geometry rule restated in Python,
the list of windows every raster is asked for, handle plumbing."""
import ctypes as C

import numpy as np

QB3E_OK, QB3E_EINV, QB3E_LIBERR = 0, 1, 255


def blocks_of(W, H):
    return (W + 3) // 4, (H + 3) // 4


def brute_segments(W, H, x0, y0, w, h, bps=64):
    """index segments that hold a block of the window, by enumeration: pixel x is held by block min(x // 4, nbx - 1) (the last
    block column / row is shifted, not padded), block (bx, by) is number by * nbx + bx of the stream, segment g // bps"""
    nbx, nby = blocks_of(W, H)
    bx0, bx1 = min(x0 // 4, nbx - 1), min((x0 + w - 1) // 4, nbx - 1)
    by0, by1 = min(y0 // 4, nby - 1), min((y0 + h - 1) // 4, nby - 1)
    return len({(by * nbx + bx) // bps for by in range(by0, by1 + 1) for bx in range(bx0, bx1 + 1)})


def row_segments(W, H, y0, h, bps):
    """segments of the whole block rows of the window (what the strip of path 2 decodes)"""
    nbx, nby = blocks_of(W, H)
    by0, by1 = min(y0 // 4, nby - 1), min((y0 + h - 1) // 4, nby - 1)
    return ((by1 + 1) * nbx - 1) // bps + 1 - by0 * nbx // bps


def windows(W, H, seed, nrandom, bps=64):
    """(x0, y0, w, h): the whole raster, one pixel at each corner, a window ending in the (shifted) last column and row, one
    straddling a segment seam, and nrandom seeded random ones"""
    out = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]
    out.append((max(0, W - 7), max(0, H - 6), min(7, W), min(6, H)))
    nbx, nby = blocks_of(W, H)
    if nbx * nby > bps:                     # the first block of segment 1 and its neighbours
        bx, by = bps % nbx, bps // nbx
        x0, y0 = max(0, min(4 * bx, W - 1) - 1), max(0, min(4 * by, H - 1) - 1)
        out.append((x0, y0, min(3, W - x0), min(3, H - y0)))
        out.append((0, y0, W, min(2, H - y0)))          # ... and a sliver of whole rows across the seam
    rng = np.random.default_rng(seed)
    for i in range(nrandom):
        big = i % 4 == 0                                # every fourth one large, the others a few blocks
        w = int(rng.integers(1, W + 1)) if big else int(rng.integers(1, min(W, 70) + 1))
        h = int(rng.integers(1, H + 1)) if big else int(rng.integers(1, min(H, 40) + 1))
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return out


def open_handle(L, buf):
    """qb3_read_start + qb3_read_info over a host array; returns (handle, (w, h, bands))"""
    dims = (C.c_size_t * 3)()
    p = L.qb3_read_start(buf.ctypes.data, buf.size, dims)
    assert p and L.qb3_read_info(p)
    return p, tuple(dims)


def handle_error(p):
    """the decoder handle's error word: the handle starts with four size_t, two uint64 and `int error` (qb3_host.h, struct decs,
    the reference's layout QB3decode.h:36-49); there is no getter in the reference's interface"""
    return C.c_int.from_address(p + 48).value
