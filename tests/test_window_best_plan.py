"""The window kernels for 8-bit common-factor rasters (include/qb3x.h: qb3x_set_decoder_window_kernels, QB3X_WINK_CF8), the part that
needs no GPU: the bit exists and is harmless where the kernels do not apply, qb3x_window_segments counts what an enumeration counts,
and the rasters of test_window_best_decode.py are what that file takes them for -- coded common-factor containers (the header's mode
byte is 1 or 5, never STORED, never an RLE mode) with the share of signal units their names promise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
import qb3_window16 as W16  # noqa: E402
import qb3_window_best as WB  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT = WB.QB3X_WINK_CF8


def test_the_bit_is_declared_and_bound(qb3):
    text = open(os.path.join(ROOT, "include", "qb3x.h")).read()
    assert "#define QB3X_WINK_CF8 2u" in text and qb3.QB3X_WINK_CF8 == BIT == 2
    assert qb3.QB3X_WINK_CF8 & qb3.QB3X_WINK_U16 == 0
    qb3.lib.qb3x_set_decoder_window_kernels(None, BIT)                      # a NULL handle: no-op


def test_the_profile_name_is_listed(qb3):
    """dec_window_best stands in the header's list of profile names (the comment of qb3x_profile_get), beside dec_window16"""
    text = open(os.path.join(ROOT, "include", "qb3x.h")).read()
    names = text[text.index("Kernel names:"):]
    names = names[:names.index("*/")]
    assert "dec_window16 (" in names and "dec_window_best (" in names


def test_the_bit_is_harmless_where_the_kernels_do_not_apply(qb3, oracle):
    """oracle-made containers (no table): 8-bit RGB in QB3M_CF_H, a STORED one, a narrow one -- the setter takes the bit alone and
    among others, the handle stays good, qb3x_window_segments counts the same, and qb3x_read_window on the STORED container still
    crops on the host"""
    L = qb3.lib
    for (w, h, b, gen, mode, stored) in ((64, 48, 3, "FEW", WB.CF_H, False), (64, 48, 3, "RANDOM", WB.CF_H, True), (3, 400, 1, "TERRACE", WB.CF_H, False)):
        img = oracle.generate(w, h, b, 0, gen, 5)
        s = oracle.encode(img, 0, mode)
        p, dims = W.open_handle(L, s)
        assert dims == (w, h, b) and (L.qb3_get_mode(p) == 255) == stored
        before = L.qb3x_window_segments(p, 0, 0, w, h, None)
        for mask in (BIT, BIT | W16.QB3X_WINK_U16, 0xffffffff, 0, BIT):
            L.qb3x_set_decoder_window_kernels(p, mask)
            assert W.handle_error(p) == W.QB3E_OK and L.qb3x_window_segments(p, 0, 0, w, h, None) == before
        if stored:
            win = (5, 7, 11, 13)
            out = np.full(13 * 11 * b + 16, 0x5a, np.uint8)
            assert L.qb3x_read_window(p, *win, out.ctypes.data, 0) == 13 * 11 * b
            assert L.qb3x_last_window_path(p) == 3 and L.qb3x_last_window_segments(p) == 0
            assert np.array_equal(out[:13 * 11 * b].reshape(13, 11, b), img[7:20, 5:16]) and (out[13 * 11 * b:] == 0x5a).all()
        L.qb3_destroy_decoder(p)


@pytest.mark.parametrize("bands", WB.BANDS)
@pytest.mark.parametrize("shape", WB.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_rasters_are_coded_common_factor_containers(oracle, shape, bands):
    """every raster of the GPU tests x QB3M_CF, QB3M_CF_H, QB3M_BEST: the mode byte of the oracle's container is 1 or 5 (BEST: the RLE0
    pass did not win).  Against QB3M_BASE the common-factor container of FEW, TERRACE and scaled16 is at least a fifth smaller -- most of
    their units carry the signal -- and NOISY3's is within 1 %: practically none of its units does"""
    w, h = shape
    for name in WB.NAMES:
        img = WB.raster(oracle.generate, name, w, h, bands, 7 * w + bands)
        assert img.shape == (h, w, bands) and img.dtype == np.uint8
        size = {}
        for mode in WB.MODES + (WB.BASE,):
            s = oracle.encode(img, 0, mode)
            size[mode] = len(s)
            if mode != WB.BASE:
                assert int(s[10]) == (1 if mode == WB.CF else 5), (name, mode, int(s[10]))
        if name in ("FEW", "TERRACE", "scaled16"):
            assert size[WB.CF_H] <= 0.8 * size[WB.BASE], (name, size)
        if name == "NOISY3":
            assert abs(size[WB.CF_H] - size[WB.BASE]) <= 0.01 * size[WB.BASE], size


def test_const_is_the_container_whose_rle_pass_won(oracle):
    """CONST in QB3M_BEST: the mode byte says 7 -- the fixture of "the RLE0 pass won: path 3" """
    assert int(oracle.encode(oracle.generate(260, 37, 3, 0, "CONST", 1), 0, WB.BEST)[10]) == 7


@pytest.mark.parametrize("shape", WB.SHAPES, ids=lambda s: "%dx%d" % s)
def test_segment_count_on_a_common_factor_handle(qb3, oracle, shape):
    """64 blocks a segment; the count is the enumeration's, with and without the bit"""
    L = qb3.lib
    Wd, Ht = shape
    s = oracle.encode(oracle.generate(Wd, Ht, 3, 0, "FEW", 7), 0, WB.CF_H)
    p, dims = W.open_handle(L, s)
    assert dims == (Wd, Ht, 3) and L.qb3_get_mode(p) == WB.CF_H
    bps = C.c_size_t()
    L.qb3x_window_segments(p, 0, 0, Wd, Ht, C.byref(bps))
    assert bps.value == 64
    for mask in (0, BIT):
        L.qb3x_set_decoder_window_kernels(p, mask)
        for win in W.windows(Wd, Ht, 300 + Wd, 100):
            assert L.qb3x_window_segments(p, *win, None) == W.brute_segments(Wd, Ht, *win), win
    L.qb3_destroy_decoder(p)
