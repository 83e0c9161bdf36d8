"""What the tests of the window kernels for 8-bit common-factor rasters share (test_window_best_plan.py, test_window_best_decode.py):
the shapes, the rasters that reach every unit form of a common-factor stream, and the fields of a table entry."""
import numpy as np

QB3X_WINK_CF8 = 2
CF, CF_H, BEST, BASE = 1, 5, 7, 4          # QB3M_CF (Z order), QB3M_CF_H, QB3M_BEST; QB3M_BASE to compare sizes with
MODES = (CF, CF_H, BEST)
BANDS = (1, 3, 4)
# the smallest shapes at which each mechanism can fail, by blocks per row (nbx) against the 64 blocks of a segment
SHAPES = ((260, 37),        # nbx = 65: a segment is reached from two block rows
          (256, 24),        # nbx = 64: rows start where segments do
          (100, 100),       # nbx = 25: several rows a segment, a partial last segment
          (1001, 259))      # shifted last column and row
# FEW: six distinct values (index-form units).  TERRACE: plateaus of multiples of 1000 mod 256 (common-factor units: a factor written
# once, then "same as before" across segment boundaries -- the entry's factor).  PALETTE: five odd values.  NOISY3: a gradient with
# three bits of noise (practically no signal units: the fast path alone).  scaled16: multiples of 16 (a factor in every unit).
# mixed: a patchwork of scaled, few-valued, noisy and quantised areas (the factor state changes hands inside segments and across them)
GENERATED = ("FEW", "TERRACE", "PALETTE", "NOISY3")
NAMES = GENERATED + ("scaled16", "mixed")


def mixed(w, h, b, seed):
    """the patchwork of test_gpu_parity.py's common-factor rasters, restated"""
    rng = np.random.default_rng(seed)

    def scaled(k, hh, ww):
        return (rng.integers(0, 256 // k, size=(hh, ww, b), dtype=np.uint8) * k).astype(np.uint8)

    def few(hh, ww, n=5):
        return rng.integers(0, 256, size=n, dtype=np.uint8)[rng.integers(0, n, size=(hh, ww, b))]

    m = rng.integers(0, 256, size=(h, w, b), dtype=np.uint8) // 8 + np.arange(w, dtype=np.uint8)[None, :, None]
    m[: h // 3] = scaled(6, h // 3, w)
    m[h // 3: h // 2, : w // 2] = few(h // 2 - h // 3, w // 2)
    m[h // 2:, w // 2:] = (m[h // 2:, w // 2:] // 4) * 4
    return np.ascontiguousarray(m)


def raster(generate, name, w, h, b, seed):
    """raster `name` as a uint8 array (h, w, b); generate: the oracle's generator (pyoracle.generate)"""
    if name in GENERATED:
        return generate(w, h, b, 0, name, seed)
    if name == "scaled16":
        return (np.random.default_rng(seed).integers(0, 16, size=(h, w, b), dtype=np.uint8) * 16).astype(np.uint8)
    assert name == "mixed"
    return mixed(w, h, b, seed)


def device_raster(oracle, name, Wd, Ht, bands, seed):
    import torch
    return torch.from_numpy(raster(oracle.generate, name, Wd, Ht, bands, seed)).cuda()


def entry_bytes(bands):
    """a table entry of these rasters: 6 position bytes, a rung, an entering value and a factor per band, 64 fields of 3 bytes"""
    return 6 + 3 * bands + 192


def field_at(bands, lane):
    """offset of block `lane`'s 3-byte field in its entry: 12 bits of length, then 3 bits of entering rung per band"""
    return 6 + 3 * bands + 3 * lane
