"""Window decode on the device (include/qb3x.h: qb3x_decode_window_device, qb3x_read_window).  The one invariant: a window is the
crop of what the whole decode writes.  Expected bytes are the numpy / torch crop of the SOURCE raster (lossless containers) or of
qb3x_decode_device on a second handle (quanta, damaged or truncated streams), never of a window call.  Every destination is filled
with a sentinel first, is longer than needed, and must still hold the sentinel everywhere outside the window rows' payload."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
from qb3_window_dev import (FTL, BASE, BASE_Z, CF_H, RLE, ZCURVE, SENTINEL,  # noqa: E402
                            as_rows, full_decode, make_container, table_chunks, to_device, window_call)

pytestmark = pytest.mark.gpu



# ---------------------------------------------------------------------------------------------------------------- path 1
@pytest.mark.parametrize("bands", (1, 3, 4))
@pytest.mark.parametrize("shape", ((4096, 4096), (1000, 37), (100, 100), (2051, 1030)), ids=lambda s: "%dx%d" % s)
def test_window_kernel(qb3, shape, bands):
    """8-bit rasters of 1, 3, 4 bands x FTL, BASE x Hilbert, Z order x identity and R-G, G, B-G band maps, level-2 table: the
    window kernel, tight and wide rows, destination addresses of every alignment (the address offset k % 4 walks through 0..3
    while tight and wide rows alternate)"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht = shape
    img = synth.generate(Wd, Ht, bands, 0, "NOISY3", 31 * bands + Wd)
    rows = as_rows(img, Ht)
    maps = (None,) if bands == 1 else (None, list(range(bands)))           # the default (R-G, G, B-G for 3 and 4 bands), identity
    k = 0
    # FTL and BASE in Hilbert order, BASE in Z order (QB3M_BASE_Z), and FTL from a handle whose Z order stuck (reference
    # QB3encode.cpp:124-132): that container has no "SC" chunk and every decoder, the reference's included, reads it in Hilbert
    # order (QB3decode.h:306-308) -- not the source's pixels, so there the whole decode of a second handle is the reference
    # (... and only where no block is shifted: the two copies of a pixel that a shifted last block repeats differ in such a decode,
    # and which of them the whole decode leaves is not defined)
    cases = [(FTL, False), (BASE, False), (BASE_Z, False)] + ([(FTL, True)] if Wd % 4 == 0 and Ht % 4 == 0 else [])
    for mode, sticky_z in cases:
        for cband in maps:
            d_c, n, _ = make_container(qb3, img, 0, mode, 2, cband, zorder=sticky_z)
            dec = qdev.DeviceDecoder(d_c, n)
            assert L.qb3_get_mode(dec.p) == mode and (L.qb3_get_order(dec.p) == ZCURVE) == (mode == BASE_Z or sticky_z)
            want = rows
            if sticky_z:
                full, st = full_decode(qb3, d_c, n)
                assert full is not None and st == 0
                want = full.view(Ht, -1)
            wins = W.windows(Wd, Ht, 5 * Wd + bands + mode, 40)
            for i, win in enumerate(wins):
                for extra in (0, 1 + (i * 7) % 29):
                    k += 1
                    window_call(qb3, dec, d_c, win, want, bands, 1, k % 4, extra)
                    assert L.qb3x_last_window_path(dec.p) == 1, win
                    assert L.qb3x_last_window_segments(dec.p) == L.qb3x_window_segments(dec.p, *win, None) == W.brute_segments(Wd, Ht, *win)
                    assert L.qb3x_last_decode_status(dec.p) == 0
            dec.close()


def test_window_kernel_dequantises_the_window(qb3):
    """quanta above 1 with a level-2 table: path 1, then the WINDOW is multiplied back (its own stride), not the raster"""
    import torch
    from qb3_amd import device as qdev, synth
    Wd, Ht, b = 1000, 300, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 11)
    d_c, n, _ = make_container(qb3, img, 0, BASE, 2, quanta=3)
    want, st = full_decode(qb3, d_c, n)
    assert want is not None and not torch.equal(want, img.reshape(-1))     # lossy: the reference bytes are the whole decode's
    dec = qdev.DeviceDecoder(d_c, n)
    for i, win in enumerate(W.windows(Wd, Ht, 3, 12)):
        window_call(qb3, dec, d_c, win, want.view(Ht, -1), b, 1, 0, (0, 9)[i % 2])
        assert qb3.lib.qb3x_last_window_path(dec.p) == 1
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- path 2
PATH2 = [(1000, 520, 4, 2, FTL, "LANDSAT16"), (1001, 259, 1, 2, BASE, "LANDSAT16"), (777, 300, 1, 5, FTL, "DEM"), (520, 301, 1, 7, BASE, "DEM"),
         (640, 203, 5, 0, FTL, "NOISY3"), (300, 222, 2, 5, BASE, "DEM"),
         (1000, 300, 3, 0, CF_H, "NOISY3"), (512, 260, 8, 2, CF_H, "LANDSAT16"), (515, 260, 1, 7, CF_H, "DEM")]


@pytest.mark.parametrize("case", PATH2, ids=lambda c: "%dx%dx%d-t%d-m%d" % c[:5])
def test_strip_of_block_rows(qb3, case):
    """one shape per decoder family that decodes strip by strip: the segments of the window's block rows, then the crop"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht, b, dt, mode, gen = case
    tsz = qb3.TYPESIZE[dt]
    img = synth.generate(Wd, Ht, b, dt, gen, 19)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, dt, mode, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    bps = C.c_size_t()
    L.qb3x_window_segments(dec.p, 0, 0, Wd, Ht, C.byref(bps))
    for i, win in enumerate(W.windows(Wd, Ht, 23, 16, bps.value)):
        window_call(qb3, dec, d_c, win, rows, b * tsz, tsz, 0, (0, 5)[i % 2])
        assert L.qb3x_last_window_path(dec.p) == 2, win
        assert L.qb3x_last_window_segments(dec.p) == W.row_segments(Wd, Ht, win[1], win[3], bps.value)
        assert L.qb3x_last_decode_status(dec.p) == 0
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- path 3
def check_path3(qb3, d_c, n, want_rows, Wd, Ht, pix, tsz, nwin=10, index=None):
    from qb3_amd import device as qdev
    dec = qdev.DeviceDecoder(d_c, n)
    for i, win in enumerate(W.windows(Wd, Ht, 41, nwin)):
        window_call(qb3, dec, d_c, win, want_rows, pix, tsz, 0, (0, 3)[i % 2], index)
        assert qb3.lib.qb3x_last_window_path(dec.p) == 3, win
    dec.close()


def test_whole_decode_and_crop(qb3, oracle):
    """everything the shortcuts do not take: a level-1 table, plain (oracle-made) containers, an out-of-band index, an RLE mode whose
    byte pass wins, a narrow raster, a STORED container in device memory, quanta without a table"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    img = synth.generate(1000, 300, 3, 0, "NOISY3", 5)
    d_c, n, _ = make_container(qb3, img, 0, FTL, 1)                            # level 1: positions and states, no block lengths
    check_path3(qb3, d_c, n, as_rows(img, 300), 1000, 300, 3, 1)
    enc = qdev.DeviceEncoder(1000, 300, 3, 0, mode=FTL, want_index=True, index_chunk=2)    # level 2, but the caller brings an index
    dst, n, index = enc.encode(img.reshape(-1))
    check_path3(qb3, dst, n, as_rows(img, 300), 1000, 300, 3, 1, 6, index)
    enc.close()
    for (w, h, b, dt, mode, gen) in ((509, 259, 3, 0, FTL, "NOISY3"), (300, 200, 1, 3, BASE, "DEM"), (3, 400, 3, 0, FTL, "NOISY3"), (64, 48, 3, 2, FTL, "RANDOM"),
                                     (600, 300, 3, 0, RLE, "TERRACE")):
        himg = oracle.generate(w, h, b, dt, gen, 5)
        s = oracle.encode(himg, dt, mode)
        if gen == "RANDOM":
            assert s[10] == 255                                             # STORED
        if mode == RLE:
            assert s[10] == RLE and len(s) < len(oracle.encode(himg, dt, 0))    # the byte pass won
        tsz = himg.itemsize
        check_path3(qb3, to_device(s), len(s), torch.from_numpy(himg.view(np.uint8).reshape(h, -1)).cuda(), w, h, b * tsz, tsz)
    # this library's own RLE container keeps its level-2 table in front of the packed bytes: still the whole decode
    timg = torch.from_numpy(oracle.generate(600, 300, 3, 0, "TERRACE", 5)).cuda()
    d_c, n, _ = make_container(qb3, timg, 0, RLE, 2)
    assert int(d_c[10]) == RLE
    check_path3(qb3, d_c, n, as_rows(timg, 300), 600, 300, 3, 1, 6)
    # quanta: lossy, the reference bytes are the whole decode's on a second handle
    for (w, h, b, dt) in ((400, 200, 3, 0), (300, 200, 1, 3)):
        himg = oracle.generate(w, h, b, dt, "NOISY3" if dt == 0 else "DEM", 9)
        s = oracle.encode(himg, dt, BASE, quanta=3)
        d_c = to_device(s)
        want, _ = full_decode(qb3, d_c, len(s))
        assert want is not None
        check_path3(qb3, d_c, len(s), want.view(h, -1), w, h, b * himg.itemsize, himg.itemsize, 8)


# ---------------------------------------------------------------------------------------------------------------- trust
def test_damaged_tables_and_short_streams_cost_time_not_pixels(qb3):
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht, b = 2048, 1024, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 77)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, 0, FTL, 2)
    host = d_c[:n].cpu().numpy()
    chunks, data_off = table_chunks(host)
    E = 6 + 2 * b + 80
    per_chunk = (65535 - 12) // E
    nseg = (Wd // 4) * (Ht // 4) // 64
    assert len(chunks) == (nseg + per_chunk - 1) // per_chunk >= 3
    win = (40, 24, 300, 40)                         # block rows 6..15 of 512 blocks: segments 48..127, all in chunk 0
    seg = (24 // 4) * (Wd // 4) // 64 + 1
    assert seg < per_chunk
    e0 = chunks[0][0] + 12 + seg * E
    far = chunks[-1][0] + 12 + 5 * E + 3
    flips = {"entry": e0 + 7, "lengths": e0 + 6 + 2 * b + 11, "head": chunks[0][0] + 6, "unused chunk": far}
    for what, at in flips.items():
        bad = d_c.clone()
        bad[at] ^= 0x10
        dec = qdev.DeviceDecoder(bad, n)
        assert L.qb3x_decoder_table_entries(dec.p) == nseg, what
        window_call(qb3, dec, bad, win, rows, b, 1, 1, 4)
        if what != "unused chunk":
            assert L.qb3x_last_window_path(dec.p) == 3, what
            assert L.qb3x_last_decode_status(dec.p) & 32, what
        else:
            assert L.qb3x_last_window_path(dec.p) in (1, 3)
        dec.close()
    # the stream ends in the middle of the window's segments: whatever the whole decode makes of it
    pos = int.from_bytes(bytes(host[e0:e0 + 6]), "little")
    cut = data_off + pos // 8 + 40
    assert cut < n
    short = torch.zeros_like(d_c)
    short[:cut] = d_c[:cut]
    want, _ = full_decode(qb3, short, cut)
    dec = qdev.DeviceDecoder(short, cut)
    window_call(qb3, dec, short, win, None if want is None else want.view(Ht, -1), b, 1, 0, 0)
    window_call(qb3, dec, short, (0, 0, 64, 8), None if want is None else want.view(Ht, -1), b, 1, 0, 0)      # (in front of the cut)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- host flavour
@pytest.mark.parametrize("case", ((4096, 4096, 3, FTL), (8192, 4100, 4, BASE)), ids=lambda c: "%dx%dx%d-m%d" % c)
def test_window_of_a_container_in_host_memory(qb3, case):
    """qb3x_read_window: the container goes up, the window comes down; a qb3_read_data behind it (the second raster takes the
    strip pipeline there) is not disturbed"""
    import torch
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht, b, mode = case
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 3)
    d_c, n, _ = make_container(qb3, img, 0, mode, 2)
    s = d_c[:n].cpu().numpy()
    himg = img.cpu().numpy()
    del d_c, img
    for i, (x0, y0, w, h) in enumerate(((1001, 517, 1024, 1024), (Wd - 5, Ht - 5, 5, 5), (0, 0, Wd, 9))):
        stride = w * b + (0, 13)[i % 2]
        out = np.full(h * stride + 32, SENTINEL, np.uint8)
        p, _ = W.open_handle(L, s)
        assert L.qb3x_read_window(p, x0, y0, w, h, out.ctypes.data, stride if i % 2 else 0) == h * w * b, qb3.last_error()
        assert L.qb3x_last_window_path(p) == 1 and L.qb3x_last_window_segments(p) == W.brute_segments(Wd, Ht, x0, y0, w, h)
        L.qb3_destroy_decoder(p)
        r = out[:h * stride].reshape(h, stride)
        assert np.array_equal(r[:, :w * b], himg[y0:y0 + h, x0:x0 + w].reshape(h, w * b))
        assert (r[:, w * b:] == SENTINEL).all() and (out[h * stride:] == SENTINEL).all()
    got = qb3.decode_window(s, 7, 9, 33, 21)
    assert got.shape == (21, 33, b) and np.array_equal(got, himg[9:30, 7:40])
    full, dims, _, _ = qb3.decode(s)
    assert dims == (Wd, Ht, b) and np.array_equal(full, himg.ravel())


# ---------------------------------------------------------------------------------------------------------------- Python, repeats
def test_python_interface(qb3):
    import torch
    from qb3_amd import device as qdev, synth
    for (w, h, b, dt, path) in ((700, 300, 3, 0, 1), (500, 260, 4, 2, 2), (300, 200, 1, 7, 2)):
        img = synth.generate(w, h, b, dt, "NOISY3", 8)
        d_c, n, _ = make_container(qb3, img, dt, FTL, 2)
        dec = qdev.DeviceDecoder(d_c, n)
        got = dec.decode_window(d_c, 13, 21, 101, 55)
        assert got.shape == (55, 101, b) and got.element_size() == qb3.TYPESIZE[dt] and str(got.dtype) == "torch." + qb3.NP_DTYPE[dt]
        assert torch.equal(got.view(torch.uint8), img[21:76, 13:114].contiguous().view(torch.uint8))
        assert dec.last_window[0] == path and dec.last_window[1] >= 1
        out = torch.zeros(55 * 101 * b * qb3.TYPESIZE[dt] + 8, dtype=torch.uint8, device="cuda")
        got2 = dec.decode_window(d_c, 13, 21, 101, 55, out=out)
        assert got2.data_ptr() == out.data_ptr() and torch.equal(got2, got)
        host = qb3.decode_window(d_c[:n].cpu().numpy(), 13, 21, 101, 55)
        assert host.dtype == np.dtype(qb3.NP_DTYPE[dt]) and np.array_equal(host.view(np.uint8), got.view(torch.uint8).cpu().numpy())
        dec.close()


def test_a_window_repeats(qb3):
    """the same window three times on one handle, and once on a fresh handle right behind an encode: identical bytes"""
    import torch
    from qb3_amd import device as qdev, synth
    Wd, Ht, b = 2051, 1030, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 2)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, 0, BASE, 2)
    win = (1001, 517, 600, 300)
    dec = qdev.DeviceDecoder(d_c, n)
    for _ in range(3):
        window_call(qb3, dec, d_c, win, rows, b, 1, 0, 0)
        assert qb3.lib.qb3x_last_window_path(dec.p) == 1
    dec.close()
    d_c2, n2, _ = make_container(qb3, img, 0, BASE, 2)     # an encode has just used LDS and registers
    dec = qdev.DeviceDecoder(d_c2, n2)
    window_call(qb3, dec, d_c2, win, rows, b, 1, 0, 0)
    assert qb3.lib.qb3x_last_window_path(dec.p) == 1 and n2 == n and torch.equal(d_c2[:n], d_c[:n])
    dec.close()
