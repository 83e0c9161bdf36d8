"""What the tests of the 16-bit window kernels share (test_window16_plan.py, test_window16_decode.py): the shapes, the generators,
the windows every raster is asked for, and the rungs of a raster's units restated in numpy.  The device plumbing is
qb3_window_dev.py's."""
import numpy as np

import qb3_window as W
from qb3_window_dev import QB3X_WINK_U16, U16, I16  # noqa: F401

HILBERT = 0x01548CD9AEFB7623            # reference QB3common.h:193

# the smallest shapes at which each mechanism can fail, by blocks per row (nbx) against blocks per segment (NB: 64 for 1..4 bands,
# 32 for eight bands, 21 for six -- 64 / band groups)
SHAPES_NARROW = ((260, 37),     # nbx = 65: a segment is reached from two block rows
                 (256, 24),     # nbx = 64: nbx % NB == 0
                 (100, 100),    # nbx = 25 < NB: several rows a segment, partial last segment
                 (1001, 259))   # shifted last column and row
SHAPES_WIDE = ((132, 37),       # nbx = 33
               (128, 24),       # nbx = 32: nbx % NB == 0 for eight bands
               (50, 50),        # nbx = 13 < NB
               (1001, 259))
# LANDSAT16 (gradient + six bits of noise), DEM (steep gradient, wraps in int16), NOISY3 (three bits of noise: the low amplitude)
GENERATORS = ("LANDSAT16", "DEM", "NOISY3")


def shapes_of(bands):
    return SHAPES_NARROW if bands <= 4 else SHAPES_WIDE


def windows(Wd, Ht, seed, bps, nrandom=24):
    """W.windows plus: the whole raster (W.windows' first), a 1 x 1 window in the shifted last block, a window one full block column
    wide, a window ending at Wd - 1"""
    out = W.windows(Wd, Ht, seed, nrandom, bps)
    out.append((Wd - 1, Ht - 1, 1, 1))
    bx = min(3, (Wd + 3) // 4 - 1)
    out.append((4 * bx, 0, min(4, Wd - 4 * bx), Ht))
    out.append((max(0, Wd - 10), min(3, Ht - 1), min(9, Wd - 1), min(5, Ht - min(3, Ht - 1))))
    assert out[-1][0] + out[-1][2] == Wd - 1 or Wd < 11
    return out


def unit_rungs(band):
    """the rung of every unit of ONE band (a 2-D array of 16-bit values, sides multiples of 4) coded in Hilbert order with the identity
    band map, FTL: the top bit of the largest mag-sign delta of the block's sixteen values, the first against the last value of the
    block before (the stream's first against 0) -- reference QB3encode.h, restated"""
    h, w = band.shape
    assert h % 4 == 0 and w % 4 == 0
    nib = [(HILBERT >> (60 - 4 * i)) & 15 for i in range(16)]              # (y << 2) | x of the i-th value visited
    blocks = band.astype(np.int64).reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16)[:, nib]
    d = np.diff(blocks.reshape(-1), prepend=0)
    d = ((d + 32768) & 0xffff) - 32768                                      # the difference as a 16-bit two's complement number
    m = np.where(d < 0, -2 * d - 1, 2 * d).reshape(-1, 16).max(axis=1)
    return np.floor(np.log2(np.maximum(m, 1))).astype(np.int64)
