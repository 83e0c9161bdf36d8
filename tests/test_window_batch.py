"""Batched window decode on the device (include/qb3x.h: qb3x_decode_windows_device, qb3x_read_windows).  The invariant is the single
call's: every window is the crop of what the whole decode writes.  Expected bytes are the crop of the SOURCE raster (lossless
containers) or of qb3x_decode_device on a second handle (quanta, the sticky Z order, damaged or truncated streams), never of a batch
call.  All destinations of a batch lie in ONE sentinel-filled buffer, which must hold the sentinel everywhere outside the windows'
rows afterwards."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
from qb3_window_dev import (FTL, BASE, BASE_Z, CF_H, RLE, ZCURVE, SENTINEL, Layout, as_rows, batch_call, chunk_check,  # noqa: E402
                            full_decode, make_container, paths, single_calls, table_chunks, to_device)

pytestmark = pytest.mark.gpu

_vp = C.c_void_p


def profile_counts(qb3):
    from qb3_amd import device as qdev
    return {k: v[1] for k, v in qdev.profile_report().items()}


# ---------------------------------------------------------------------------------------------------------------- path 1
@pytest.mark.parametrize("bands", (1, 3, 4))
@pytest.mark.parametrize("shape", ((4096, 4096), (1000, 37), (100, 100), (2051, 1030)), ids=lambda s: "%dx%d" % s)
def test_one_launch_for_all_windows(qb3, shape, bands):
    """8-bit rasters of 1, 3, 4 bands x FTL, BASE, BASE_Z (and the sticky Z order) x default and identity band maps: every window
    exact and on path 1, the segment count the sum of the windows' enumerations, and the bytes those of n single calls"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht = shape
    img = synth.generate(Wd, Ht, bands, 0, "NOISY3", 31 * bands + Wd)
    rows = as_rows(img, Ht)
    maps = (None,) if bands == 1 else (None, list(range(bands)))
    cases = [(FTL, False), (BASE, False), (BASE_Z, False)] + ([(FTL, True)] if Wd % 4 == 0 and Ht % 4 == 0 else [])
    k = 0
    for mode, sticky_z in cases:
        for cband in maps:
            d_c, n, _ = make_container(qb3, img, 0, mode, 2, cband, zorder=sticky_z)
            dec = qdev.DeviceDecoder(d_c, n)
            assert L.qb3_get_mode(dec.p) == mode and (L.qb3_get_order(dec.p) == ZCURVE) == (mode == BASE_Z or sticky_z)
            want = rows
            if sticky_z:                                # (that container reads in Hilbert order: the whole decode is the reference)
                full, st = full_decode(qb3, d_c, n)
                assert full is not None and st == 0
                want = full.view(Ht, -1)
            rects = W.windows(Wd, Ht, 5 * Wd + bands + mode, 40)
            assert len(rects) >= 45
            lay = Layout(rects, bands, 1, "u8", start=k)
            k += 1
            got, buf = batch_call(qb3, dec, d_c, lay)
            assert got == len(rects), qb3.last_error()
            lay.check(buf, want)
            assert paths(qb3, dec.p, len(rects)) == [1] * len(rects)
            assert all(L.qb3x_window_ok(dec.p, i) == 1 for i in range(len(rects)))
            assert L.qb3x_last_window_path(dec.p) == 1
            assert L.qb3x_last_window_segments(dec.p) == sum(W.brute_segments(Wd, Ht, *r) for r in rects)
            assert L.qb3x_last_decode_status(dec.p) == 0
            if cband is None:                           # equal to the single call, byte for byte, sentinels included
                assert torch.equal(buf, single_calls(qb3, dec, d_c, lay))
            dec.close()


@pytest.mark.parametrize("count", (1, 2, 63, 64, 65, 1000))
def test_batch_sizes(qb3, count):
    """windows of a few blocks each: many identical ones, many inside one segment (the wave search at its ends: windows of one
    wave each, neighbours in the prefix array), and seeded random ones"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht, b = 1000, 300, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 4)
    d_c, n, _ = make_container(qb3, img, 0, BASE, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    rng = np.random.default_rng(count)
    rects = []
    for i in range(count):
        kind = i % 3
        if kind == 0:
            rects.append((17, 9, 23, 11))                               # identical
        elif kind == 1:
            rects.append((4 * (i % 50), 0, 1 + i % 4, 1 + i % 3))       # inside segment 0 (blocks 0..63 of block row 0)
        else:
            w, h = int(rng.integers(1, 40)), int(rng.integers(1, 20))
            rects.append((int(rng.integers(0, Wd - w + 1)), int(rng.integers(0, Ht - h + 1)), w, h))
    lay = Layout(rects, b, 1, "u8")
    got, buf = batch_call(qb3, dec, d_c, lay)
    assert got == count, qb3.last_error()
    lay.check(buf, as_rows(img, Ht))
    assert paths(qb3, dec.p, count) == [1] * count
    assert L.qb3x_window_path(dec.p, count) == 0
    assert L.qb3x_last_window_segments(dec.p) == sum(W.brute_segments(Wd, Ht, *r) for r in rects)
    dec.close()


def test_mosaic_and_one_launch(qb3):
    """a 2048 x 2048 region as 64 windows of 256 x 256 whose destinations tile one 2048-wide buffer through dst_stride; the library's
    profile shows ONE dec_window launch for the batch -- a loop over the single call would show 64"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht, b = 4096, 2304, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 12)
    d_c, n, _ = make_container(qb3, img, 0, FTL, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    X0, Y0, R, T = 1001, 131, 2048, 256
    rects = [(X0 + T * i, Y0 + T * j, T, T) for j in range(R // T) for i in range(R // T)]
    buf = torch.full((R * R * b + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    wins = qb3.window_array(rects, [buf.data_ptr() + ((y - Y0) * R + (x - X0)) * b for x, y, _, _ in rects], [R * b] * len(rects))
    qdev.profile_enable(1)
    qdev.profile_reset()
    try:
        got = L.qb3x_decode_windows_device(dec.p, _vp(d_c.data_ptr()), None, wins, len(rects), _vp(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        counts = profile_counts(qb3)
    finally:
        qdev.profile_enable(0)
        qdev.profile_reset()
    assert got == 64, qb3.last_error()
    assert counts.get("dec_window") == 1, counts
    assert paths(qb3, dec.p, 64) == [1] * 64
    assert torch.equal(buf[:R * R * b].view(R, R * b), as_rows(img, Ht)[Y0:Y0 + R, X0 * b:(X0 + R) * b])
    assert bool((buf[R * R * b:] == SENTINEL).all())
    dec.close()


def test_quanta(qb3):
    """BASE with quanta 3 and a level-2 table: path 1, every window dequantised as a raster of its own"""
    import torch
    from qb3_amd import device as qdev, synth
    Wd, Ht, b = 1000, 300, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 11)
    d_c, n, _ = make_container(qb3, img, 0, BASE, 2, quanta=3)
    want, st = full_decode(qb3, d_c, n)
    assert want is not None and not torch.equal(want, img.reshape(-1))
    dec = qdev.DeviceDecoder(d_c, n)
    rects = W.windows(Wd, Ht, 3, 12)
    lay = Layout(rects, b, 1, "u8")
    got, buf = batch_call(qb3, dec, d_c, lay)
    assert got == len(rects)
    lay.check(buf, want.view(Ht, -1))
    assert paths(qb3, dec.p, len(rects)) == [1] * len(rects)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- path 2
PATH2 = [(1000, 520, 4, 2, FTL, "LANDSAT16"), (1001, 259, 1, 2, BASE, "LANDSAT16"), (777, 300, 1, 5, FTL, "DEM"), (520, 301, 1, 7, BASE, "DEM"),
         (640, 203, 5, 0, FTL, "NOISY3"), (300, 222, 2, 5, BASE, "DEM"),
         (1000, 300, 3, 0, CF_H, "NOISY3"), (512, 260, 8, 2, CF_H, "LANDSAT16"), (515, 260, 1, 7, CF_H, "DEM")]


def union_of_row_segments(Wd, Ht, rects, bps):
    """segments of the whole block rows of every window (row_segments' rule), each counted once"""
    nbx, nby = W.blocks_of(Wd, Ht)
    segs = set()
    for (x0, y0, w, h) in rects:
        by0, by1 = min(y0 // 4, nby - 1), min((y0 + h - 1) // 4, nby - 1)
        first, end = by0 * nbx // bps, ((by1 + 1) * nbx - 1) // bps + 1
        assert end - first == W.row_segments(Wd, Ht, y0, h, bps)
        segs.update(range(first, end))
    return len(segs)


@pytest.mark.parametrize("case", PATH2, ids=lambda c: "%dx%dx%d-t%d-m%d" % c[:5])
def test_merged_strips(qb3, case):
    """one shape per decoder family that decodes strip by strip: the windows' ranges of block rows merged, a segment decoded once"""
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht, b, dt, mode, gen = case
    tsz = qb3.TYPESIZE[dt]
    img = synth.generate(Wd, Ht, b, dt, gen, 19)
    d_c, n, _ = make_container(qb3, img, dt, mode, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    bps = C.c_size_t()
    L.qb3x_window_segments(dec.p, 0, 0, Wd, Ht, C.byref(bps))
    # without the whole raster and the large windows (they make the union trivial), and with them
    small = [r for r in W.windows(Wd, Ht, 23, 16, bps.value) if r[3] <= 40]
    for rects in (small, W.windows(Wd, Ht, 23, 16, bps.value)):
        lay = Layout(rects, b * tsz, tsz, "u8")
        got, buf = batch_call(qb3, dec, d_c, lay)
        assert got == len(rects), qb3.last_error()
        lay.check(buf, as_rows(img, Ht))
        assert paths(qb3, dec.p, len(rects)) == [2] * len(rects)
        assert L.qb3x_last_window_path(dec.p) == 2
        assert L.qb3x_last_window_segments(dec.p) == union_of_row_segments(Wd, Ht, rects, bps.value)
        assert L.qb3x_last_decode_status(dec.p) == 0
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- path 3
DECODE_KERNELS = ("dec_units", "dec_segments", "dec_index_table", "dec_index_serial", "dec_index_prev", "dec_index_scan")


def check_path3_once(qb3, d_c, n, want_rows, Wd, Ht, pix, tsz, nwin=10, index=None):
    """a batch that no shortcut takes: every window on path 3 and exact, and the decode kernels ran as often as for ONE
    qb3x_decode_device on a fresh handle"""
    import torch
    from qb3_amd import device as qdev
    L = qb3.lib
    st = _vp(torch.cuda.current_stream().cuda_stream)
    rects = W.windows(Wd, Ht, 41, nwin)
    lay = Layout(rects, pix, tsz, "u8")
    qdev.profile_enable(1)
    try:
        qdev.profile_reset()
        ref = qdev.DeviceDecoder(d_c, n)
        out = torch.zeros(ref.out_bytes, dtype=torch.uint8, device="cuda")
        assert L.qb3x_decode_device(ref.p, _vp(d_c.data_ptr()), _vp(out.data_ptr()), _vp(index.data_ptr()) if index is not None else None, st)
        torch.cuda.synchronize()
        one = profile_counts(qb3)
        ref.close()
        qdev.profile_reset()
        dec = qdev.DeviceDecoder(d_c, n)
        got, buf = batch_call(qb3, dec, d_c, lay, index=index)
        many = profile_counts(qb3)
    finally:
        qdev.profile_enable(0)
        qdev.profile_reset()
    assert got == len(rects), qb3.last_error()
    lay.check(buf, want_rows)
    assert paths(qb3, dec.p, len(rects)) == [3] * len(rects) and L.qb3x_last_window_path(dec.p) == 3
    for name in DECODE_KERNELS:
        assert many.get(name, 0) == one.get(name, 0), (name, one, many)
    assert "dec_window" not in many
    dec.close()


def test_one_whole_decode_for_the_batch(qb3, oracle):
    """a level-1 table, plain (oracle-made) containers, an out-of-band index, an RLE mode whose byte pass wins, a narrow raster, a
    STORED container in device memory, quanta without a table"""
    import torch
    from qb3_amd import device as qdev, synth
    img = synth.generate(1000, 300, 3, 0, "NOISY3", 5)
    d_c, n, _ = make_container(qb3, img, 0, FTL, 1)
    check_path3_once(qb3, d_c, n, as_rows(img, 300), 1000, 300, 3, 1)
    enc = qdev.DeviceEncoder(1000, 300, 3, 0, mode=FTL, want_index=True, index_chunk=2)    # level 2, but the caller brings an index
    dst, n, index = enc.encode(img.reshape(-1))
    check_path3_once(qb3, dst, n, as_rows(img, 300), 1000, 300, 3, 1, 6, index)
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
        check_path3_once(qb3, to_device(s), len(s), torch.from_numpy(himg.view(np.uint8).reshape(h, -1)).cuda(), w, h, b * tsz, tsz)
    for (w, h, b, dt) in ((400, 200, 3, 0), (300, 200, 1, 3)):             # quanta without a table
        himg = oracle.generate(w, h, b, dt, "NOISY3" if dt == 0 else "DEM", 9)
        s = oracle.encode(himg, dt, BASE, quanta=3)
        d_c = to_device(s)
        want, _ = full_decode(qb3, d_c, len(s))
        assert want is not None
        check_path3_once(qb3, d_c, len(s), want.view(h, -1), w, h, b * himg.itemsize, himg.itemsize, 8)


# ---------------------------------------------------------------------------------------------------------------- trust
def test_damage_costs_time_window_by_window(qb3):
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht, b = 2048, 1024, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 77)
    d_c, n, _ = make_container(qb3, img, 0, FTL, 2)
    host = d_c[:n].cpu().numpy()
    chunks, data_off = table_chunks(host)
    E = 6 + 2 * b + 80
    per_chunk = (65535 - 12) // E
    nbx = Wd // 4
    nseg = nbx * (Ht // 4) // 64
    assert len(chunks) == (nseg + per_chunk - 1) // per_chunk >= 3
    want, st = full_decode(qb3, d_c, n)
    assert want is not None and st == 0 and torch.equal(want, img.reshape(-1))
    want = want.view(Ht, -1)
    # windows that read entries of chunk 0 only: block rows 6..15 are segments 48..127 (eight segments a block row)
    seg = (24 // 4) * nbx // 64 + 1                 # block row 6, blocks 64..127: pixels x 256..511, y 24..27
    assert seg < per_chunk
    holds = [(40, 24, 300, 40), (300, 26, 8, 1), (256, 20, 256, 8)]         # hold a block of segment `seg`
    beside = [(600, 24, 100, 4), (0, 24, 256, 4), (40, 40, 300, 40), (5, 600, 50, 50), (1900, 1000, 148, 24)]
    rects = holds + beside
    for r in holds:
        assert any((by * nbx + bx) // 64 == seg for by in range(r[1] // 4, (r[1] + r[3] - 1) // 4 + 1) for bx in range(r[0] // 4, (r[0] + r[2] - 1) // 4 + 1))
    for r in beside:
        assert not any((by * nbx + bx) // 64 == seg for by in range(r[1] // 4, (r[1] + r[3] - 1) // 4 + 1) for bx in range(r[0] // 4, (r[0] + r[2] - 1) // 4 + 1))
    lay = Layout(rects, b, 1, "u8")
    e0 = chunks[0][0] + 12 + seg * E

    # a flipped byte in chunk 0, which only some windows read (the last two read the table's later chunks): the chunk fails its
    # check, the table is condemned for the call -- every window from the whole decode, all of them written
    for what, at in (("entry", e0 + 7), ("lengths", e0 + 6 + 2 * b + 11), ("head", chunks[0][0] + 6)):
        bad = d_c.clone()
        bad[at] ^= 0x10
        dec = qdev.DeviceDecoder(bad, n)
        assert L.qb3x_decoder_table_entries(dec.p) == nseg, what
        ref, _ = full_decode(qb3, bad, n)
        assert ref is not None
        got, buf = batch_call(qb3, dec, bad, lay)
        assert got == len(rects), what
        lay.check(buf, ref.view(Ht, -1))
        assert paths(qb3, dec.p, len(rects)) == [3] * len(rects), what
        assert L.qb3x_last_decode_status(dec.p) & 32, what
        dec.close()

    # a block-length field of segment `seg` altered and the chunk's check recomputed: the table passes its check, the segment does
    # not decode -- the windows that hold it end on path 3, the others stay on path 1, and all are exact
    bad_host = host.copy()
    bad_host[e0 + 6 + 2 * b + 11] ^= 0x10
    c0, ln = chunks[0]
    assert ln == 12 + per_chunk * E and bad_host[c0 + 4] == 3
    assert chunk_check(host[c0 + 12:c0 + ln]) == int(host[c0 + 6]) | int(host[c0 + 7]) << 8        # (the rule restated here is the library's)
    chk = chunk_check(bad_host[c0 + 12:c0 + ln])
    bad_host[c0 + 6], bad_host[c0 + 7] = chk & 0xff, chk >> 8
    bad = to_device(bad_host)
    dec = qdev.DeviceDecoder(bad, n)
    ref, _ = full_decode(qb3, bad, n)
    assert ref is not None and torch.equal(ref, img.reshape(-1))           # (the whole decode drops the table and walks the stream)
    got, buf = batch_call(qb3, dec, bad, lay)
    assert got == len(rects)
    lay.check(buf, want)
    assert paths(qb3, dec.p, len(rects)) == [3] * len(holds) + [1] * len(beside)
    assert L.qb3x_last_window_path(dec.p) == 1
    assert L.qb3x_last_window_segments(dec.p) == sum(W.brute_segments(Wd, Ht, *r) for r in rects) + nseg
    dec.close()

    # the stream ends in the middle of the first windows' segments: whatever the whole decode makes of it
    pos = int.from_bytes(bytes(host[e0:e0 + 6]), "little")
    cut = data_off + pos // 8 + 40
    assert cut < n
    short = torch.zeros_like(d_c)
    short[:cut] = d_c[:cut]
    ref, _ = full_decode(qb3, short, cut)
    dec = qdev.DeviceDecoder(short, cut)
    got, buf = batch_call(qb3, dec, short, lay)
    if ref is None:
        assert got == 0 and paths(qb3, dec.p, len(rects)) == [0] * len(rects)
        lay.check(buf, None, skip=range(len(rects)))        # (a shortcut may have written windows before the whole decode failed)
    else:
        assert got == len(rects)
        lay.check(buf, ref.view(Ht, -1))
        assert paths(qb3, dec.p, len(rects)) == [3] * len(rects)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- host flavour
def test_windows_of_a_container_in_host_memory(qb3, oracle):
    """qb3x_read_windows over host copies of a path 1, a path 2 and a path 3 container: one upload, strided host destinations with
    sentinels; the bytes are those of the device call"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    for (Wd, Ht, b, dt, mode, level, gen, path) in ((2051, 1030, 3, 0, BASE, 2, "NOISY3", 1), (1000, 520, 4, 2, FTL, 2, "LANDSAT16", 2), (1000, 300, 3, 0, FTL, 1, "NOISY3", 3)):
        tsz = qb3.TYPESIZE[dt]
        img = synth.generate(Wd, Ht, b, dt, gen, 3)
        d_c, n, _ = make_container(qb3, img, dt, mode, level)
        s = d_c[:n].cpu().numpy()
        rects = W.windows(Wd, Ht, 8, 12)
        lay = Layout(rects, b * tsz, tsz, "u8")
        dec = qdev.DeviceDecoder(d_c, n)
        got, dbuf = batch_call(qb3, dec, d_c, lay)
        assert got == len(rects) and paths(qb3, dec.p, len(rects)) == [path] * len(rects)
        dec.close()
        hbuf = np.full(lay.size, SENTINEL, np.uint8)
        strides = [0 if sb == r[2] * lay.pix else sb // tsz for sb, r in zip(lay.sbytes, rects)]
        wins = qb3.window_array(rects, [hbuf.ctypes.data + o for o in lay.offs], strides)
        p, _ = W.open_handle(L, s)
        assert L.qb3x_read_windows(p, wins, len(rects)) == len(rects), qb3.last_error()
        assert [L.qb3x_window_path(p, i) for i in range(len(rects))] == [path] * len(rects)
        assert all(L.qb3x_window_ok(p, i) == 1 for i in range(len(rects)))
        L.qb3_destroy_decoder(p)
        assert np.array_equal(hbuf, dbuf.cpu().numpy())
        lay.check(torch.from_numpy(hbuf).cuda(), as_rows(img, Ht))


# ---------------------------------------------------------------------------------------------------------------- Python, repeats
def test_python_interface(qb3):
    import torch
    from qb3_amd import device as qdev, synth
    rects = [(13, 21, 101, 55), (0, 0, 1, 1), (250, 100, 33, 7), (13, 21, 101, 55)]
    for (w, h, b, dt, path) in ((700, 300, 3, 0, 1), (500, 260, 4, 2, 2), (300, 200, 1, 7, 2)):
        img = synth.generate(w, h, b, dt, "NOISY3", 8)
        d_c, n, _ = make_container(qb3, img, dt, FTL, 2)
        dec = qdev.DeviceDecoder(d_c, n)
        got = dec.decode_windows(d_c, rects)
        assert dec.last_windows == [path] * len(rects)
        host = qb3.decode_windows(d_c[:n].cpu().numpy(), rects)
        assert len(got) == len(host) == len(rects)
        for g, hh, (x0, y0, ww, wh) in zip(got, host, rects):
            assert g.shape == (wh, ww, b) and g.element_size() == qb3.TYPESIZE[dt] and str(g.dtype) == "torch." + qb3.NP_DTYPE[dt]
            one = dec.decode_window(d_c, x0, y0, ww, wh)
            assert torch.equal(g.view(torch.uint8), one.view(torch.uint8))
            assert torch.equal(g.view(torch.uint8), img[y0:y0 + wh, x0:x0 + ww].contiguous().view(torch.uint8))
            assert hh.shape == (wh, ww, b) and hh.dtype == np.dtype(qb3.NP_DTYPE[dt])
            assert np.array_equal(hh.view(np.uint8), g.contiguous().view(torch.uint8).cpu().numpy())
            assert np.array_equal(hh, qb3.decode_window(d_c[:n].cpu().numpy(), x0, y0, ww, wh))
        outs = [torch.zeros(wh * ww * b * qb3.TYPESIZE[dt] + 8, dtype=torch.uint8, device="cuda") for (_, _, ww, wh) in rects]
        got2 = dec.decode_windows(d_c, rects, out=outs)
        for g2, g, o in zip(got2, got, outs):
            assert g2.data_ptr() == o.data_ptr() and torch.equal(g2, g)
        dec.close()


def test_a_batch_repeats(qb3):
    """the same batch twice on one handle, then a single-window call, then the batch again: identical bytes each time (the
    handle's descriptor and status buffers are reused, the single call shares the status buffer)"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht, b = 2051, 1030, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 2)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, 0, BASE, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    rects = W.windows(Wd, Ht, 6, 60)
    lay = Layout(rects, b, 1, "u8")
    small = Layout(rects[:3], b, 1, "u8")
    bufs = []
    for step in range(4):
        if step == 2:
            one = dec.decode_window(d_c, 1001, 517, 600, 300)
            assert torch.equal(one, img[517:817, 1001:1601]) and dec.last_window[0] == 1
            got, sbuf = batch_call(qb3, dec, d_c, small)        # (a smaller batch in between: the buffers do not shrink)
            assert got == 3
            small.check(sbuf, rows)
            continue
        got, buf = batch_call(qb3, dec, d_c, lay)
        assert got == len(rects) and paths(qb3, dec.p, len(rects)) == [1] * len(rects)
        lay.check(buf, rows)
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]) and torch.equal(bufs[0], bufs[2])
    dec.close()
