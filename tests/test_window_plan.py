"""Window decode, the part that needs no GPU: the five entry points exist, qb3x_window_segments counts what an enumeration of
the window's blocks counts, argument errors are refused before anything is touched, and STORED containers are cropped on the
host.  The decoding itself is tested on the device (test_window_decode.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402

FTL, BASE, CF_H = 8, 4, 5
NAMES = ("qb3x_decode_window_device", "qb3x_read_window", "qb3x_window_segments", "qb3x_last_window_path", "qb3x_last_window_segments")


def test_window_symbols_are_exported_and_bound(qb3):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qb3x.h")).read()
    for n in NAMES:
        assert n in qb3.EXPORTED and hasattr(qb3.lib, n) and n + "(" in text
        assert getattr(qb3.lib, n).argtypes is not None
    assert qb3.lib.qb3x_last_window_path(None) == 0 and qb3.lib.qb3x_last_window_segments(None) == 0
    assert callable(qb3.decode_window)


def count(L, p, x0, y0, w, h):
    bps = C.c_size_t(12345)
    n = L.qb3x_window_segments(p, x0, y0, w, h, C.byref(bps))
    assert L.qb3x_window_segments(p, x0, y0, w, h, None) == n          # (the size is optional)
    return n, bps.value


@pytest.mark.parametrize("bands", (1, 3, 4))
@pytest.mark.parametrize("shape", ((4096, 64), (1000, 37), (100, 100), (8, 8)), ids=lambda s: "%dx%d" % s)
def test_segment_count_is_the_enumeration(qb3, oracle, shape, bands):
    """8-bit rasters of 1, 3 and 4 bands, FTL and BASE: 64 blocks a segment.  nbx = 1024; nbx = 250 (neither side a multiple of
    4, segments wrap rows); nbx = 25 (a segment spans three or four block rows); one segment in all"""
    L = qb3.lib
    Wd, Ht = shape
    img = oracle.generate(Wd, Ht, bands, 0, "NOISY3", 7)
    for mode in (FTL, BASE):
        s = oracle.encode(img, 0, mode)
        p, dims = W.open_handle(L, s)
        assert dims == (Wd, Ht, bands) and L.qb3_get_mode(p) == mode
        for (x0, y0, w, h) in W.windows(Wd, Ht, 1000 * bands + mode, 200):
            n, bps = count(L, p, x0, y0, w, h)
            assert bps == 64
            assert n == W.brute_segments(Wd, Ht, x0, y0, w, h), (x0, y0, w, h)
        nbx, nby = W.blocks_of(Wd, Ht)
        assert count(L, p, 0, 0, Wd, Ht)[0] == (nbx * nby + 63) // 64
        # not inside the raster, or empty: 0
        for bad in ((0, 0, Wd + 1, 1), (0, 0, 1, Ht + 1), (Wd, 0, 1, 1), (0, Ht, 1, 1), (0, 0, 0, 1), (0, 0, 1, 0), (2**64 - 1, 0, 1, 1), (1, 0, 2**64 - 1, 1)):
            assert L.qb3x_window_segments(p, *bad, None) == 0
        assert W.handle_error(p) == W.QB3E_OK                          # a question, not a call that can fail the handle
        L.qb3_destroy_decoder(p)


def test_segment_count_before_read_info_and_without_a_block_grid(qb3, oracle):
    L = qb3.lib
    img = oracle.generate(64, 64, 3, 0, "NOISY3", 1)
    s = oracle.encode(img, 0, FTL)
    dims = (C.c_size_t * 3)()
    p = L.qb3_read_start(s.ctypes.data, s.size, dims)
    assert L.qb3x_window_segments(p, 0, 0, 4, 4, None) == 0            # the handle is not at stage 2
    assert L.qb3_read_info(p) and L.qb3x_window_segments(p, 0, 0, 4, 4, None) == 1
    L.qb3_destroy_decoder(p)
    # STORED by rule (4 x 4), STORED because nothing compresses, narrow: every valid window counts 1, the size is 0
    for (w, h, b, dt, gen) in ((4, 4, 3, 0, "NOISY3"), (64, 48, 3, 0, "RANDOM"), (3, 400, 1, 0, "NOISY3"), (500, 2, 3, 2, "NOISY3")):
        s = oracle.encode(oracle.generate(w, h, b, dt, gen, 5), dt, FTL)
        p, _ = W.open_handle(L, s)
        assert (L.qb3_get_mode(p) == 255) == (gen == "RANDOM" or w * h <= 16)
        for win in ((0, 0, w, h), (w - 1, h - 1, 1, 1), (0, 0, 1, 1)):
            assert count(L, p, *win) == (1, 0)
        assert L.qb3x_window_segments(p, 0, 0, w + 1, h, None) == 0
        L.qb3_destroy_decoder(p)


@pytest.mark.parametrize("case", ((300, 200, 4, 2, FTL), (300, 200, 1, 2, BASE), (160, 120, 5, 0, FTL), (200, 90, 1, 5, FTL), (120, 80, 2, 7, BASE),
                                  (300, 200, 3, 0, CF_H), (256, 128, 8, 2, CF_H), (130, 70, 1, 7, CF_H)), ids=lambda c: "%dx%dx%d-t%d-m%d" % c)
def test_segment_count_of_other_shapes_is_bounded(qb3, oracle, case):
    """other value sizes, band counts and modes have other segment sizes: the count lies between 1 and the raster's segments,
    which is what the whole raster counts"""
    L = qb3.lib
    w, h, b, dt, mode = case
    s = oracle.encode(oracle.generate(w, h, b, dt, "NOISY3", 3), dt, mode)
    p, _ = W.open_handle(L, s)
    assert L.qb3_get_mode(p) == mode
    nbx, nby = W.blocks_of(w, h)
    n_all, bps = count(L, p, 0, 0, w, h)
    assert bps >= 1 and n_all == (nbx * nby + bps - 1) // bps
    for win in W.windows(w, h, 77, 50, bps):
        n, bps2 = count(L, p, *win)
        assert bps2 == bps and 1 <= n <= n_all
        assert n == W.brute_segments(w, h, *win, bps=bps)
    L.qb3_destroy_decoder(p)


def test_argument_errors(qb3, oracle):
    """refused with QB3E_EINV before a device is asked for and before a byte is written -- so also on a box without a GPU"""
    L = qb3.lib
    w, h, b = 64, 48, 3
    s = oracle.encode(oracle.generate(w, h, b, 0, "NOISY3", 1), 0, FTL)
    out = np.full(w * h * b + 64, 0xa5, np.uint8)
    fake_dev = C.c_void_p(0x10000)                  # never dereferenced: every call below fails its checks first
    big = 2**64 - 1
    cases = [(0, 0, 0, 4, 0), (0, 0, 4, 0, 0), (w - 3, 0, 4, 4, 0), (0, h - 3, 4, 4, 0), (big, 0, 1, 1, 0), (0, big, 1, 1, 0), (1, 0, big, 1, 0),
             (0, 1, 1, big, 0), (w, 0, 1, 1, 0), (0, 0, 8, 8, 8 * b - 1), (0, 0, 8, 8, 1)]
    for (x0, y0, ww, hh, stride) in cases:
        for host in (True, False):
            p, _ = W.open_handle(L, s)
            if host:
                assert L.qb3x_read_window(p, x0, y0, ww, hh, out.ctypes.data, stride) == 0
            else:
                assert L.qb3x_decode_window_device(p, fake_dev, None, x0, y0, ww, hh, fake_dev, stride, None) == 0
            assert W.handle_error(p) == W.QB3E_EINV, (x0, y0, ww, hh, stride, host)
            assert L.qb3x_last_window_path(p) == 0
            L.qb3_destroy_decoder(p)
    assert (out == 0xa5).all()
    # a handle that is not past qb3_read_info; a misaligned or missing source; a missing destination
    dims = (C.c_size_t * 3)()
    p = L.qb3_read_start(s.ctypes.data, s.size, dims)
    assert L.qb3x_read_window(p, 0, 0, 4, 4, out.ctypes.data, 0) == 0 and W.handle_error(p) == W.QB3E_EINV
    L.qb3_destroy_decoder(p)
    for src, dst in ((C.c_void_p(0x10002), fake_dev), (None, fake_dev), (fake_dev, None)):
        p, _ = W.open_handle(L, s)
        assert L.qb3x_decode_window_device(p, src, None, 0, 0, 4, 4, dst, 0, None) == 0 and W.handle_error(p) == W.QB3E_EINV
        L.qb3_destroy_decoder(p)
    p, _ = W.open_handle(L, s)
    assert L.qb3x_read_window(p, 0, 0, 4, 4, None, 0) == 0 and W.handle_error(p) == W.QB3E_EINV
    L.qb3_destroy_decoder(p)
    assert (out == 0xa5).all()
    # a handle over a copy of the container's head only: the host call would read the stream past that copy, like qb3_read_data
    head = s[:40].copy()
    p = L.qb3x_read_start(head.ctypes.data, head.size, s.size, dims)
    assert p and L.qb3_read_info(p)
    assert L.qb3x_read_window(p, 0, 0, 4, 4, out.ctypes.data, 0) == 0 and W.handle_error(p) == W.QB3E_EINV and (out == 0xa5).all()
    L.qb3_destroy_decoder(p)


def check_stored_window(L, s, img, win, stride_extra):
    """qb3x_read_window of a STORED container against the numpy crop; sentinel bytes in the gaps and behind the end stay"""
    x0, y0, w, h = win
    b, tsz = img.shape[2], img.itemsize
    stride = w * b + stride_extra                   # in values
    out = np.full((h * stride + 16) * tsz, 0x5a, np.uint8)
    p, _ = W.open_handle(L, s)
    assert L.qb3_get_mode(p) == 255
    n = L.qb3x_read_window(p, x0, y0, w, h, out.ctypes.data, stride if stride_extra else 0)
    assert n == h * w * b * tsz and W.handle_error(p) == W.QB3E_OK
    assert L.qb3x_last_window_path(p) == 3 and L.qb3x_last_window_segments(p) == 0
    L.qb3_destroy_decoder(p)
    rows = out[:h * stride * tsz].reshape(h, stride * tsz)
    want = np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w]).view(np.uint8).reshape(h, w * b * tsz)
    assert np.array_equal(rows[:, :w * b * tsz], want), win
    assert (rows[:, w * b * tsz:] == 0x5a).all() and (out[h * stride * tsz:] == 0x5a).all(), win


def test_stored_containers_are_cropped_on_the_host(qb3, oracle):
    L = qb3.lib
    img = oracle.generate(4, 4, 3, 0, "RANDOM", 3)
    s = oracle.encode(img, 0, FTL)
    nwin = 0
    for x0 in range(4):
        for y0 in range(4):
            for w in range(1, 5 - x0):
                for h in range(1, 5 - y0):
                    for extra in (0, 5):
                        check_stored_window(L, s, img, (x0, y0, w, h), extra)
                    nwin += 1
    assert nwin == 100
    for (w, h, b, dt) in ((1, 1, 1, 7), (16, 1, 2, 3), (2, 8, 4, 5)):           # the other tiny shapes, every value size
        img = oracle.generate(w, h, b, dt, "RANDOM", 3)
        s = oracle.encode(img, dt, FTL)
        for win in ((0, 0, w, h), (w - 1, h - 1, 1, 1), (0, 0, 1, h), (0, 0, w, 1)):
            for extra in (0, 3):
                check_stored_window(L, s, img, win, extra)
    img = oracle.generate(64, 48, 3, 2, "RANDOM", 5)                            # nothing compresses: the oracle stores it
    s = oracle.encode(img, 2, BASE)
    for win in W.windows(64, 48, 9, 30):
        for extra in (0, 7):
            check_stored_window(L, s, img, win, extra)
    assert np.array_equal(qb3.decode_window(s, 5, 7, 11, 13), img[7:20, 5:16])
    assert qb3.decode_window(s, 5, 7, 11, 13).dtype == np.uint16


def test_a_coded_window_fails_loudly_without_gpu(qb3, oracle):
    """no CPU fallback for the block codec: like qb3_read_data"""
    if qb3.lib.qb3x_device_count() > 0:
        pytest.skip("a GPU is present")
    L = qb3.lib
    s = oracle.encode(oracle.generate(32, 32, 3, 0, "NOISY3", 1), 0, FTL)
    out = np.full(32 * 32 * 3, 0xa5, np.uint8)
    p, _ = W.open_handle(L, s)
    assert L.qb3x_read_window(p, 3, 3, 8, 8, out.ctypes.data, 0) == 0
    assert W.handle_error(p) == W.QB3E_LIBERR and "no usable HIP device" in qb3.last_error()
    assert (out == 0xa5).all()
    L.qb3_destroy_decoder(p)
    with pytest.raises(RuntimeError):
        qb3.decode_window(s, 0, 0, 8, 8)
