"""What the tests of the window kernels of the remaining common-factor rasters share (test_window_best_unit_plan.py,
test_window_best_unit_decode.py): the (type, bands) matrix, rasters of any integer type that reach every unit form of a common-factor
stream, and the fields of a table entry.  Shapes and band maps are qb3_window_unit's, the device plumbing is qb3_window_dev's, the
patchwork is qb3_window_best's in the value's width."""
import numpy as np

import qb3_window_unit as WU

QB3X_WINK_CFU = 8
CF, CF_H, BEST, BASE, FTL = 1, 5, 7, 4, 8          # QB3M_CF (Z order), QB3M_CF_H, QB3M_BEST; QB3M_BASE to compare sizes with
U8, I8, U16, I16, U32, I32, U64, I64 = range(8)
TSZ = WU.TSZ
# (type, bands) of the device tests: what dec_pxu_best_kernel and dec_pxw_best_kernel take -- every value size, one band where the value
# is wider than a byte, the smallest and the largest band counts, odd and even ones, signed and unsigned
MATRIX = ((U8, 2), (U8, 5), (I8, 7), (U8, 16),
          (U16, 1), (I16, 2), (U16, 3), (U16, 4), (I16, 7), (U16, 8),
          (U32, 1), (I32, 2), (U32, 3),
          (U64, 1), (I64, 2), (U64, 5))
BIG = ((U8, 5), (I16, 7), (I32, 2), (U64, 1))          # these take (1001, 259) as their fourth shape (WU.BIG)
WITH_BEST = ((U8, 5), (U16, 8), (U32, 1), (I64, 2))    # these are coded in QB3M_BEST too
assert BIG == WU.BIG
# scaled: small random integers times k (a factor in every unit).  few: five distinct values a band, two of them a block (index-form units).  mixed: a patchwork of
# scaled, few-valued, noisy and quantised areas (the factor state changes hands inside segments and across them).  noisy: a gradient
# with noise (practically no signal units)
NAMES = ("scaled", "few", "mixed", "noisy")
SIGNAL = NAMES[:3]                                      # compressible by construction, with signal units: never STORED
FACTOR = {1: 6, 2: 1000, 4: 10 ** 6, 8: 2 ** 40 + 2 ** 20}
NOISE_BITS = {1: 3, 2: 9, 4: 20, 8: 40}


def np_unsigned(dt):
    return (np.uint8, np.uint16, np.uint32, np.uint64)[dt // 2]


def np_type(dt):
    return (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64)[dt]


def raster(name, w, h, b, dt, seed):
    """raster `name` as an array (h, w, b) of the type's numpy dtype.  The values are made as unsigned numbers of the type's width and
    reinterpreted: scaled values stay below half the range, so they are the same numbers in a signed type"""
    tsz = TSZ[dt]
    U = np_unsigned(dt)
    rng = np.random.default_rng(seed)
    k, nb = FACTOR[tsz], NOISE_BITS[tsz]

    def scaled(hh, ww):
        return (rng.integers(0, 16, size=(hh, ww, b), dtype=np.uint64) * np.uint64(k)).astype(U)

    def few(hh, ww, n=5):
        # five distinct values a band, two of them in a block of 4 x 4 (the same choice in every band): a block's deltas take few
        # values, which is what the index form codes; a quarter of the range, so that the deltas stay below the top rung
        vals = rng.integers(0, 2 ** (8 * tsz - 2), size=(n, b), dtype=np.uint64).astype(U)
        pair = rng.integers(0, n, size=((hh + 3) // 4, (ww + 3) // 4, 2))
        sel = rng.integers(0, 2, size=(hh, ww))
        return vals[pair[np.arange(hh)[:, None] // 4, np.arange(ww)[None, :] // 4, sel]]

    def noisy(hh, ww):
        slope = 1 if tsz == 1 else 37
        return (rng.integers(0, 2 ** nb, size=(hh, ww, b), dtype=np.uint64) + np.arange(ww, dtype=np.uint64)[None, :, None] * np.uint64(slope)).astype(U)

    if name == "scaled":
        m = scaled(h, w)
    elif name == "few":
        m = few(h, w)
    elif name == "noisy":
        m = noisy(h, w)
    else:
        assert name == "mixed"
        m = noisy(h, w)
        m[: h // 3] = scaled(h // 3, w)
        m[h // 3: h // 2, : w // 2] = few(h // 2 - h // 3, w // 2)
        m[h // 2:, w // 2:] = (m[h // 2:, w // 2:] // U(4)) * U(4)
    return np.ascontiguousarray(m).view(np_type(dt))


def device_raster(name, w, h, b, dt, seed):
    """the same on the device, as a tensor (h, w, b) of the type's width (torch has every signed type and uint8: the bits are what counts)"""
    import torch
    a = raster(name, w, h, b, dt, seed)
    return torch.from_numpy(a if dt == U8 else a.view((np.int8, np.int16, np.int32, np.int64)[dt // 2])).cuda()


def entry_bytes(bands, tsz):
    """a table entry of these rasters: 6 position bytes, a rung byte, an entering value and a factor per band, 3 bytes a unit"""
    return 6 + bands * (1 + 2 * tsz) + 3 * (64 // bands) * bands


def field_at(bands, tsz, lane):
    """offset of unit `lane`'s 3-byte field in its entry: 12 bits of length, then the rung the unit is entered with"""
    return 6 + bands * (1 + 2 * tsz) + 3 * lane
