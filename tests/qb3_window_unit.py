"""What the tests of the lane-per-unit window kernels share (test_window_unit_plan.py, test_window_unit_decode.py): the (type, bands)
matrix, the shapes and band maps of a band count, the rungs of a raster's units restated in numpy for any value width, and the size of
a table entry.  Windows are qb3_window16's, the geometry rule is qb3_window's, the device plumbing and the constants are
qb3_window_dev.py's."""
import numpy as np

import qb3_window16 as W16
from qb3_window_dev import (QB3X_WINK_U16, QB3X_WINK_CF8, QB3X_WINK_UNIT, U8, I8, U16, I16, U32, I32, U64, I64, TSZ,  # noqa: F401
                            FTL, BASE, BASE_Z, CF_H, SENTINEL)

HILBERT = W16.HILBERT

# (type, bands) of the device tests: every value size, the smallest and the largest band count of each, odd and even ones, signed and unsigned
MATRIX = ((U8, 2), (U8, 5), (I8, 7), (U8, 16),
          (U16, 5), (I16, 7), (U16, 9),
          (U32, 1), (I32, 2), (U32, 3),
          (U64, 1), (I64, 2), (U64, 5), (U64, 16))
BIG = ((U8, 5), (I16, 7), (I32, 2), (U64, 1))          # these take (1001, 259) as their fourth shape
GENERATORS = ("NOISY3", "DEM", "RANDOM")
# (type, bands) of the plan tests and the blocks a segment of each holds: 64 // bands
PLAN_MATRIX = ((U8, 2, 32), (U8, 5, 12), (U8, 7, 9), (U8, 16, 4), (U16, 5, 12), (U16, 9, 7), (I32, 1, 64), (I32, 3, 21), (I64, 2, 32))


def seg_blocks(bands):
    return 64 // bands


def shapes_of(dt, bands):
    """the smallest shapes at which each mechanism can fail, with NB = 64 // bands blocks a segment"""
    NB = seg_blocks(bands)
    return ((4 * (NB + 1), 37),                         # nbx = NB + 1: a segment is reached from two block rows
            (8 * NB, 24),                               # nbx = 2 NB: nbx % NB == 0
            (4 * max(2, NB // 2) - 1, 50),              # several block rows in a segment, a partial last segment, a shifted last column
            (1001, 259) if (dt, bands) in BIG else (201, 67))      # shifted last column and row


def maps_of(bands):
    """None: the encoder's default (R-G, G, B-G for three bands and more; the identity below)"""
    if bands < 3:
        return (None,)
    return (None, list(range(bands))) + (([0, 0, 2, 2, 4],) if bands == 5 else ())


def unit_rungs(band, bits):
    """the rung of every unit of ONE band (a 2-D array, sides multiples of 4, values of `bits` bits in any integer type) coded in
    Hilbert order with the identity band map, FTL: the top bit of the largest mag-sign delta of the block's sixteen values, the first
    against the last value of the block before (the stream's first against 0) -- W16.unit_rungs for any value width, in arithmetic
    modulo 2^64 so that 64-bit values need no wider type"""
    h, w = band.shape
    assert h % 4 == 0 and w % 4 == 0
    nib = [(HILBERT >> (60 - 4 * i)) & 15 for i in range(16)]              # (y << 2) | x of the i-th value visited
    mask = np.uint64((1 << bits) - 1)
    v = band.astype(np.int64).view(np.uint64) & mask
    blocks = v.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16)[:, nib].reshape(-1)
    d = (blocks - np.concatenate((np.zeros(1, np.uint64), blocks[:-1]))) & mask      # the difference as a `bits`-bit two's complement number
    neg = (d >> np.uint64(bits - 1)) & np.uint64(1)
    m = (((d << np.uint64(1)) & mask) ^ (np.uint64(0) - neg)) & mask           # mag-sign: 2 d, or -2 d - 1 for a negative d
    m = m.reshape(-1, 16).max(axis=1)
    rung = np.zeros(m.shape, np.int64)
    for k in range(1, bits):
        rung[(m >> np.uint64(k)) > 0] = k
    return rung


def entry_bytes(bands, tsz):
    """a level-2 entry of these rasters: position, a rung byte and the entering value per band, twelve bits a unit"""
    return 6 + bands * (1 + tsz) + (seg_blocks(bands) * bands * 12 + 7) // 8
