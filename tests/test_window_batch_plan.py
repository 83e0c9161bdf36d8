"""Batched window decode, the part that needs no GPU: the four entry points exist and are bound, argument errors refuse the WHOLE
batch before a byte is written, STORED containers are cropped on the host window by window, and a handle over the container's head
only is refused.  The decoding itself is tested on the device (test_window_batch.py)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402

FTL, BASE = 8, 4
NAMES = ("qb3x_decode_windows_device", "qb3x_read_windows", "qb3x_window_ok", "qb3x_window_path")
SENTINEL = 0x5a


def test_batch_symbols_are_exported_and_bound(qb3):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qb3x.h")).read()
    for n in NAMES:
        assert n in qb3.EXPORTED and hasattr(qb3.lib, n) and n + "(" in text
        assert getattr(qb3.lib, n).argtypes is not None
    assert "qb3x_window;" in text
    assert C.sizeof(qb3.Window) == 6 * C.sizeof(C.c_size_t)
    assert qb3.lib.qb3x_window_ok(None, 0) == 0 and qb3.lib.qb3x_window_path(None, 0) == 0
    assert callable(qb3.decode_windows)


def stored_container(oracle):
    """nothing compresses: the oracle stores the raster"""
    img = oracle.generate(64, 48, 3, 2, "RANDOM", 5)
    s = oracle.encode(img, 2, BASE)
    assert s[10] == 255
    return img, s


def layout(img, rects, extras):
    """one sentinel-filled host buffer for all windows, 16 bytes between them; returns (buffer, byte offsets, strides in values)"""
    b, tsz = img.shape[2], img.itemsize
    offs, strides, at = [], [], 16
    for (x0, y0, w, h), extra in zip(rects, extras):
        offs.append(at)
        strides.append(w * b + extra)
        at += h * (w * b + extra) * tsz + 16
    return np.full(at, SENTINEL, np.uint8), offs, strides


def test_argument_errors_refuse_the_whole_batch(qb3, oracle):
    L = qb3.lib
    img, s = stored_container(oracle)
    w, h, b = 64, 48, 3
    good = [(0, 0, 8, 8), (5, 7, 11, 13), (w - 1, h - 1, 1, 1)]
    buf, offs, strides = layout(img, good, (0, 0, 0))
    ptrs = [buf.ctypes.data + o for o in offs]

    def refused(wins, n):
        p, _ = W.open_handle(L, s)
        assert L.qb3x_read_windows(p, wins, n) == 0
        assert W.handle_error(p) == W.QB3E_EINV
        assert L.qb3x_last_window_path(p) == 0 and L.qb3x_window_ok(p, 0) == 0 and L.qb3x_window_path(p, 0) == 0
        L.qb3_destroy_decoder(p)
        assert (buf == SENTINEL).all()

    wins = qb3.window_array(good, ptrs)
    refused(wins, 0)                                                # n == 0
    refused(None, 3)                                                # no array
    refused(wins, 2**20 + 1)                                        # (refused by the count alone: the array is not read)
    for bad in ((w - 3, 0, 4, 4), (0, h - 3, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (2**64 - 1, 0, 1, 1), (1, 0, 2**64 - 1, 1)):
        for at in range(3):                                         # one window out of the raster (or empty) among good ones
            rects = list(good)
            rects[at] = bad
            refused(qb3.window_array(rects, ptrs), 3)
    refused(qb3.window_array(good, ptrs, [0, 11 * b - 1, 0]), 3)    # a stride below w * bands
    refused(qb3.window_array(good, ptrs, [0, 0, 1]), 3)
    for at in range(3):                                             # a missing destination
        pp = list(ptrs)
        pp[at] = None
        refused(qb3.window_array(good, pp), 3)
    # a handle that is not past qb3_read_info
    dims = (C.c_size_t * 3)()
    p = L.qb3_read_start(s.ctypes.data, s.size, dims)
    assert L.qb3x_read_windows(p, wins, 3) == 0 and W.handle_error(p) == W.QB3E_EINV
    L.qb3_destroy_decoder(p)
    # the device call decides the same before it touches the device: the pointers below are never dereferenced
    fake = C.c_void_p(0x10000)
    for src, arr, n in ((C.c_void_p(0x10002), wins, 3), (None, wins, 3), (fake, None, 3), (fake, wins, 0),
                        (fake, qb3.window_array([good[0], (w, 0, 1, 1)], ptrs[:2]), 2)):
        p, _ = W.open_handle(L, s)
        assert L.qb3x_decode_windows_device(p, src, None, arr, n, None) == 0 and W.handle_error(p) == W.QB3E_EINV
        L.qb3_destroy_decoder(p)
    assert (buf == SENTINEL).all()


def test_a_handle_over_the_head_only_is_refused(qb3, oracle):
    L = qb3.lib
    img, s = stored_container(oracle)
    buf, offs, _ = layout(img, [(0, 0, 4, 4)], (0,))
    head = s[:40].copy()
    dims = (C.c_size_t * 3)()
    p = L.qb3x_read_start(head.ctypes.data, head.size, s.size, dims)
    assert p and L.qb3_read_info(p)
    wins = qb3.window_array([(0, 0, 4, 4)], [buf.ctypes.data + offs[0]])
    assert L.qb3x_read_windows(p, wins, 1) == 0 and W.handle_error(p) == W.QB3E_EINV and (buf == SENTINEL).all()
    L.qb3_destroy_decoder(p)


def test_stored_batch_is_cropped_on_the_host(qb3, oracle):
    L = qb3.lib
    img, s = stored_container(oracle)
    b, tsz = img.shape[2], img.itemsize
    rects = W.windows(64, 48, 9, 30)
    extras = [(0, 7)[i % 2] for i in range(len(rects))]             # tight and wide rows
    buf, offs, strides = layout(img, rects, extras)
    wins = qb3.window_array(rects, [buf.ctypes.data + o for o in offs], [st if ex else 0 for st, ex in zip(strides, extras)])
    p, _ = W.open_handle(L, s)
    assert L.qb3_get_mode(p) == 255
    assert L.qb3x_read_windows(p, wins, len(rects)) == len(rects) and W.handle_error(p) == W.QB3E_OK
    for i in range(len(rects)):
        assert L.qb3x_window_ok(p, i) == 1 and L.qb3x_window_path(p, i) == 3
    assert L.qb3x_window_ok(p, len(rects)) == 0 and L.qb3x_window_path(p, len(rects)) == 0
    assert L.qb3x_last_window_path(p) == 3 and L.qb3x_last_window_segments(p) == 0
    L.qb3_destroy_decoder(p)
    for (x0, y0, w, h), off, stride in zip(rects, offs, strides):
        rows = buf[off:off + h * stride * tsz].reshape(h, stride * tsz)
        want = np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w]).view(np.uint8).reshape(h, w * b * tsz)
        assert np.array_equal(rows[:, :w * b * tsz], want), (x0, y0, w, h)
        rows[:, :w * b * tsz] = SENTINEL
    assert (buf == SENTINEL).all()                                  # gaps of wide strides, between and around the windows
    got = qb3.decode_windows(s, rects[:5])
    for g, (x0, y0, w, h) in zip(got, rects):
        assert g.dtype == np.uint16 and g.shape == (h, w, b) and np.array_equal(g, img[y0:y0 + h, x0:x0 + w])
