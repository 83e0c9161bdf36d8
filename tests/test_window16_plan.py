"""The 16-bit window kernels (include/qb3x.h: qb3x_set_decoder_window_kernels, QB3X_WINK_U16), the part that needs no GPU: the
switch exists and is harmless where the kernels do not apply, qb3x_window_segments counts what an enumeration counts for the
segment sizes of six and eight bands, and the generators of test_window16_decode.py reach both value decoders of the kernel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
import qb3_window16 as W16  # noqa: E402

FTL, BASE = 8, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_switch_is_exported_declared_and_bound(qb3):
    text = open(os.path.join(ROOT, "include", "qb3x.h")).read()
    name = "qb3x_set_decoder_window_kernels"
    assert name in qb3.EXPORTED and hasattr(qb3.lib, name) and name + "(decsp p, unsigned mask)" in text
    assert "#define QB3X_WINK_U16 1u" in text and qb3.QB3X_WINK_U16 == W16.QB3X_WINK_U16 == 1
    qb3.lib.qb3x_set_decoder_window_kernels(None, 1)                        # a NULL handle: no-op
    from qb3_amd import device as qdev
    assert callable(qdev.DeviceDecoder.set_window_kernels)


def test_the_switch_is_harmless_where_the_kernels_do_not_apply(qb3, oracle):
    """an oracle-made container (no table), a STORED one, a narrow one: the setter takes any mask, the handle stays good, and
    qb3x_read_window on the STORED container still crops on the host with the bit set"""
    L = qb3.lib
    for (w, h, b, dt, gen, stored) in ((64, 48, 4, 2, "LANDSAT16", False), (64, 48, 3, 2, "RANDOM", True), (3, 400, 1, 2, "DEM", False)):
        img = oracle.generate(w, h, b, dt, gen, 5)
        s = oracle.encode(img, dt, FTL)
        p, dims = W.open_handle(L, s)
        assert dims == (w, h, b) and (L.qb3_get_mode(p) == 255) == stored
        before = L.qb3x_window_segments(p, 0, 0, w, h, None)
        for mask in (W16.QB3X_WINK_U16, 0xffffffff, 0, W16.QB3X_WINK_U16):
            L.qb3x_set_decoder_window_kernels(p, mask)
            assert W.handle_error(p) == W.QB3E_OK and L.qb3x_window_segments(p, 0, 0, w, h, None) == before
        if stored:
            win = (5, 7, 11, 13)
            out = np.full(13 * 11 * b * 2 + 16, 0x5a, np.uint8)
            assert L.qb3x_read_window(p, *win, out.ctypes.data, 0) == 13 * 11 * b * 2
            assert L.qb3x_last_window_path(p) == 3 and L.qb3x_last_window_segments(p) == 0
            assert np.array_equal(out[:13 * 11 * b * 2].view(np.uint16).reshape(13, 11, b), img[7:20, 5:16]) and (out[13 * 11 * b * 2:] == 0x5a).all()
        L.qb3_destroy_decoder(p)


@pytest.mark.parametrize("bands", (6, 8))
@pytest.mark.parametrize("shape", W16.SHAPES_WIDE, ids=lambda s: "%dx%d" % s)
def test_segment_count_of_six_and_eight_bands(qb3, oracle, shape, bands):
    """uint16 of eight bands: 32 blocks a segment (two lanes a block); of six: 21 (three lanes a block, 64 // 3).  The count is the
    enumeration's, with and without the bit"""
    L = qb3.lib
    Wd, Ht = shape
    s = oracle.encode(oracle.generate(Wd, Ht, bands, 2, "LANDSAT16", 7), 2, BASE)
    p, dims = W.open_handle(L, s)
    assert dims == (Wd, Ht, bands)
    bps = C.c_size_t()
    L.qb3x_window_segments(p, 0, 0, Wd, Ht, C.byref(bps))
    assert bps.value == {6: 21, 8: 32}[bands]
    for mask in (0, W16.QB3X_WINK_U16):
        L.qb3x_set_decoder_window_kernels(p, mask)
        for win in W16.windows(Wd, Ht, 100 * bands + Wd, bps.value, 100):
            assert L.qb3x_window_segments(p, *win, None) == W.brute_segments(Wd, Ht, *win, bps=bps.value), win
    L.qb3_destroy_decoder(p)


def test_the_generators_reach_both_value_decoders(oracle):
    """The kernel decodes a unit of rung 8 or more by the code rule (px16_groups_hi) and one below 8 through the 8-bit table.  The
    rungs of a raster's units, restated in numpy from the oracle's generator output (W16.unit_rungs: one band, Hilbert order, FTL):
    the rasters of LANDSAT16 and DEM have units on both sides -- a block row starts far below the end of the row before (rung 9 and
    above: 3 and 37 times the width), the units inside a row stay at 7 and below (LANDSAT16, DEM: six bits of noise on a gradient) or below 6
    (NOISY3: three bits).  So in every wave that holds the start of a block row some lanes take one decoder and some the other.  BASE's step moves a unit by at most
    one rung, so the margins (9 against 8, 6 against 8) hold for it too."""
    rungs = {g: W16.unit_rungs(oracle.generate(256, 24, 1, 2, g, 11)[:, :, 0]) for g in W16.GENERATORS}
    for g in ("LANDSAT16", "DEM"):
        assert (rungs[g] >= 9).sum() >= 5 and (rungs[g] < 8).sum() >= 5, g
    assert (rungs["LANDSAT16"] < 8).mean() > 0.9 and (rungs["NOISY3"] < 6).mean() > 0.9
