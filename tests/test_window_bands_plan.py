"""Band-selected windows, the part that needs no GPU (include/qb3x.h: qb3x_decode_windows_bands_device, qb3x_read_windows_bands,
qb3x_last_window_gathers): the symbols exist and are bound, argument errors refuse the whole call before a byte is written, STORED
containers are cropped and selected on the host, a handle over the container's head only is refused, and qb3_amd.decode_windows takes
bands=.  Expected bytes are the numpy crop and selection of the source raster.  The decoding itself is tested on the device
(test_window_bands_decode.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
import qb3_window_unit as WU  # noqa: E402
import qb3_window_bands as WB  # noqa: E402

BASE = 4
SENTINEL = WB.SENTINEL


def test_bands_symbols_are_exported_and_bound(qb3):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qb3x.h")).read()
    for n in WB.NAMES:
        assert n in qb3.EXPORTED and hasattr(qb3.lib, n) and n + "(" in text
        assert getattr(qb3.lib, n).argtypes is not None
    assert "win_band_gather" in text
    assert qb3.lib.qb3x_last_window_gathers(None) == 0


def stored_container(oracle, dt, bands):
    """nothing compresses: the oracle stores the raster (as test_window_batch_plan.py's)"""
    img = oracle.generate(64, 48, bands, dt, "RANDOM", 5)
    s = oracle.encode(img, dt, BASE)
    assert s[10] == 255
    return img, s


def test_argument_errors_refuse_the_whole_call(qb3, oracle):
    L = qb3.lib
    img, s = stored_container(oracle, 0, 3)
    w, h, b = 64, 48, 3
    good = [(0, 0, 8, 8), (5, 7, 11, 13), (w - 1, h - 1, 1, 1)]
    nsel = 2
    sel = qb3.band_array([2, 0])
    buf = np.full(16 + sum(16 + rw * rh * 4 for _, _, rw, rh in good), SENTINEL, np.uint8)
    ptrs, at = [], 16
    for _, _, rw, rh in good:
        ptrs.append(buf.ctypes.data + at)
        at += rw * rh * 4 + 16
    wins = qb3.window_array(good, ptrs)

    def refused(wins, n, sel, nsel, handle=None):
        p = handle if handle is not None else W.open_handle(L, s)[0]
        assert L.qb3x_read_windows_bands(p, wins, n, sel, nsel) == 0
        assert W.handle_error(p) == W.QB3E_EINV
        assert L.qb3x_last_window_path(p) == 0 and L.qb3x_window_ok(p, 0) == 0 and L.qb3x_last_window_gathers(p) == 0
        L.qb3_destroy_decoder(p)
        assert (buf == SENTINEL).all()

    refused(wins, 3, None, nsel)                                            # sel == NULL
    refused(wins, 3, sel, 0)                                                # nsel == 0
    refused(wins, 3, qb3.band_array([0] * 17), 17)                          # nsel == 17
    refused(wins, 3, qb3.band_array([2, b]), 2)                             # a band number equal to the band count
    refused(qb3.window_array(good, ptrs, [0, 11 * nsel - 1, 0]), 3, sel, nsel)      # a stride of w * nsel - 1
    refused(qb3.window_array([good[0], (w - 3, 0, 4, 4), good[2]], ptrs), 3, sel, nsel)     # one bad rectangle among good ones
    refused(wins, 0, sel, nsel)
    refused(None, 3, sel, nsel)
    # a stride of w * nsel is enough, though it is below w * bands
    p, _ = W.open_handle(L, s)
    assert L.qb3x_read_windows_bands(p, qb3.window_array(good, ptrs, [0, 11 * nsel, 0]), 3, sel, nsel) == 3 and W.handle_error(p) == W.QB3E_OK
    L.qb3_destroy_decoder(p)
    buf[:] = SENTINEL
    # a head-only handle on the host call
    head = s[:40].copy()
    dims = (C.c_size_t * 3)()
    p = L.qb3x_read_start(head.ctypes.data, head.size, s.size, dims)
    assert p and L.qb3_read_info(p)
    refused(wins, 3, sel, nsel, handle=p)
    # a NULL handle
    assert L.qb3x_read_windows_bands(None, wins, 3, sel, nsel) == 0
    assert L.qb3x_decode_windows_bands_device(None, C.c_void_p(0x10000), None, wins, 3, sel, nsel, None) == 0
    # the device call decides the same before it touches the device: the pointers below are never dereferenced
    fake = C.c_void_p(0x10000)
    for src, arr, n, sl, ns in ((fake, wins, 3, None, nsel), (fake, wins, 3, sel, 0), (fake, wins, 3, qb3.band_array([0] * 17), 17),
                                (fake, wins, 3, qb3.band_array([2, b]), 2), (fake, qb3.window_array(good, ptrs, [0, 11 * nsel - 1, 0]), 3, sel, nsel),
                                (fake, qb3.window_array([good[0], (w, 0, 1, 1)], ptrs[:2]), 2, sel, nsel), (C.c_void_p(0x10002), wins, 3, sel, nsel),
                                (None, wins, 3, sel, nsel)):
        p, _ = W.open_handle(L, s)
        assert L.qb3x_decode_windows_bands_device(p, src, None, arr, n, sl, ns, None) == 0 and W.handle_error(p) == W.QB3E_EINV
        L.qb3_destroy_decoder(p)
    assert (buf == SENTINEL).all()


@pytest.mark.parametrize("dt,bands", ((0, 3), (3, 5)), ids=("u8x3", "i16x5"))
def test_stored_windows_are_cropped_and_selected_on_the_host(qb3, oracle, dt, bands):
    """uint8 x 3 and int16 x 5, STORED: one band, a reversal, a selection with repeats and the identity; tight, wide-even and wide-odd
    rows (WB.Layout), and a mosaic of four windows in one buffer.  No device is needed: path 3, no gather"""
    L = qb3.lib
    img, s = stored_container(oracle, dt, bands)
    Ht, Wd = img.shape[:2]
    tsz = img.itemsize
    rows = np.ascontiguousarray(img).view(np.uint8).reshape(Ht, -1)
    rects = W.windows(Wd, Ht, 9, 6)
    for sel in ([2], [2, 1, 0], [1, 1, 0, 1], list(range(bands))):
        nsel = len(sel)
        want = WB.select(rows, bands, tsz, sel)
        assert np.array_equal(want.reshape(Ht, Wd, nsel, tsz), np.ascontiguousarray(img[:, :, sel]).view(np.uint8).reshape(Ht, Wd, nsel, tsz))
        tw, th = 20, 12
        tiles = [((7 + 11 * i) % (Wd - tw), (5 + 13 * i) % (Ht - th), tw, th) for i in range(4)]
        for lay in (WB.Layout(rects, nsel, tsz),
                    WB.Layout(tiles, nsel, tsz, mosaic=(2 * tw * nsel, [((i % 2) * tw * nsel, (i // 2) * th) for i in range(4)], 2 * th))):
            n = len(lay.rects)
            hbuf = np.full(lay.size + 16, SENTINEL, np.uint8)
            base = (-hbuf.ctypes.data) % 16
            wins = qb3.window_array(lay.rects, [hbuf.ctypes.data + base + o for o in lay.offs], lay.strides())
            p, _ = W.open_handle(L, s)
            assert L.qb3_get_mode(p) == 255
            assert L.qb3x_read_windows_bands(p, wins, n, qb3.band_array(sel), nsel) == n and W.handle_error(p) == W.QB3E_OK
            assert all(L.qb3x_window_ok(p, i) == 1 and L.qb3x_window_path(p, i) == 3 for i in range(n))
            assert L.qb3x_last_window_path(p) == 3 and L.qb3x_last_window_gathers(p) == 0 and L.qb3x_last_window_segments(p) == 0
            L.qb3_destroy_decoder(p)
            got = hbuf[base:base + lay.size]
            for (x0, y0, w, h), off, sb in zip(lay.rects, lay.offs, lay.sbytes):
                r = np.lib.stride_tricks.as_strided(got[off:], (h, w * nsel * tsz), (sb, 1))
                assert np.array_equal(r, want[y0:y0 + h, x0 * nsel * tsz:(x0 + w) * nsel * tsz]), (sel, x0, y0, w, h)
                r[:] = SENTINEL
            assert (hbuf == SENTINEL).all(), "bytes outside the windows were written"


def test_python_decode_windows_takes_bands(qb3, oracle):
    img, s = stored_container(oracle, 3, 5)
    rects = W.windows(64, 48, 3, 4)[:6]
    for sel in ([4], [3, 0, 3]):
        got = qb3.decode_windows(s, rects, bands=sel)
        for g, (x0, y0, w, h) in zip(got, rects):
            assert g.dtype == np.int16 and g.shape == (h, w, len(sel)) and np.array_equal(g, img[y0:y0 + h, x0:x0 + w][:, :, sel])
    full = qb3.decode_windows(s, rects)                                     # bands=None: as before
    assert all(g.shape == (h, w, 5) and np.array_equal(g, img[y0:y0 + h, x0:x0 + w]) for g, (x0, y0, w, h) in zip(full, rects))
    with pytest.raises(RuntimeError):
        qb3.decode_windows(s, rects, bands=[5])
