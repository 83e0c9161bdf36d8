"""Ranged window reads of 8-bit common-factor rasters on the device (include/qb3x.h: QB3X_WINK_CF8 on a handle of qb3x_open_ranged;
k_dec_wins_best_ranged.hip).  The invariant is the window calls': every window is the crop of what the whole decode writes, nothing
outside a window's rows is written.  Expected bytes are the crop of the SOURCE raster (lossless containers) or of qb3x_decode_device
on a second handle (quanta), never of a window call.  What the reader is asked for is the range rule of qb3x.h, restated in
qb3_ranged.py and computed from the container's own table -- and the whole container, once, wherever the shortcut is not taken.
Containers are written by this library and held in a numpy buffer behind a reader that logs its calls.  Every damaged input is table
or stream bytes the kernel bounds by the piece it was given: no case depends on an access outside the uploaded arrays."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_ranged as R  # noqa: E402
import qb3_window as W  # noqa: E402
import qb3_window16 as W16  # noqa: E402
import qb3_window_best as WB  # noqa: E402
from qb3_ranged import check_fallback, check_host, counters, device_call, host_call, host_container, open_source  # noqa: E402
from qb3_window_best import device_raster  # noqa: E402
from qb3_window_dev import SENTINEL, Layout, as_rows, count, full_decode, make_container, paths, segments_of  # noqa: E402

pytestmark = pytest.mark.gpu

CF, CF_H, BEST = WB.CF, WB.CF_H, WB.BEST
BIT = WB.QB3X_WINK_CF8
SMALLEST = (256, 24)


# ---------------------------------------------------------------------------------------------------------------- parity
def crosses(shape, bands):
    """(raster, mode, level, band map) of a shape: the full cross on the smallest, elsewhere every raster once with modes, levels and
    band maps in rotation (each mode and level twice, the identity map on every second raster)"""
    maps = (None,) if bands < 3 else (None, list(range(bands)))
    if shape == SMALLEST:
        return [(name, mode, level, cb) for name in WB.NAMES for mode in WB.MODES for level in (1, 2) for cb in maps]
    return [(name, WB.MODES[(i + bands) % 3], 1 + (i + shape[0]) % 2, maps[i % len(maps)]) for i, name in enumerate(WB.NAMES)]


@pytest.mark.parametrize("bands", WB.BANDS)
@pytest.mark.parametrize("shape", WB.SHAPES, ids=lambda s: "%dx%d" % s)
def test_windows_from_pieces(qb3, oracle, shape, bands):
    """QB3M_CF, QB3M_CF_H, QB3M_BEST x table levels 1 and 2 x the six rasters x both band maps (the full cross on 256 x 24, thinned
    elsewhere).  Every rectangle as a single host call, then all as one batch on a fresh handle, twice (the second reads no table
    chunk); gaps 0 / 64 / 2^20; device destinations 0..3 bytes behind a dword with tight and wide rows: the crop of the source raster,
    sentinels intact, path 1 for every window, the windows' segments, and the reader asked for exactly the bytes of the plan"""
    L = qb3.lib
    Wd, Ht = shape
    full = shape == SMALLEST
    for turn, (name, mode, level, cband) in enumerate(crosses(shape, bands)):
        what = (name, mode, level, cband)
        img = device_raster(oracle, name, Wd, Ht, bands, 7 * Wd + bands)
        rows = as_rows(img, Ht)
        c = host_container(qb3, img, 0, mode, level, cband)
        assert int(c[10]) == (1 if mode == CF else 5), what
        tab = R.Table(c).shape(R.entry_bytes("cf8", bands), R.HEAD_FLAGS)
        rects = W16.windows(Wd, Ht, 5 * Wd + bands + turn, 64, 4 if full else 10)
        lay = Layout(rects, bands, 1, "cf8")
        src, p, dims = open_source(qb3, c, BIT)
        assert dims == (Wd, Ht, bands) and L.qb3x_decoder_table_entries(p) == tab.K, what
        # single calls (on the smallest shape for every third container: its full cross is about the containers)
        hbuf = None
        if not full or turn % 3 == 0:
            hbuf = np.full(lay.size, SENTINEL, np.uint8)
            cached = set()
            for k, r in enumerate(rects):
                del src.log[:]
                assert host_call(qb3, p, lay, hbuf, k) == 1, (what, r, qb3.last_error())
                assert L.qb3x_window_path(p, 0) == 1 and L.qb3x_last_window_path(p) == 1, (what, r)
                assert L.qb3x_last_window_segments(p) == W.brute_segments(Wd, Ht, *r), (what, r)
                want = R.plan_bytes(Wd, Ht, [r], tab, 0, cached)
                assert counters(qb3, p) == want == (src.bytes_logged(), len(src.log)), (what, r)
                cached.update(R.plan_chunks(Wd, Ht, [r], tab.K, tab.N))
            check_host(lay, hbuf, rows)
            assert not src.outside
        # one batch, on a fresh handle (an empty cache), twice: the second reads no table chunk
        L.qb3_destroy_decoder(p)
        src, p, _ = open_source(qb3, c, BIT)
        all_chunks = set(range(len(tab.chunks)))
        for again in (False, True):
            del src.log[:]
            hbuf2 = np.full(lay.size, SENTINEL, np.uint8)
            assert host_call(qb3, p, lay, hbuf2) == len(rects), (what, qb3.last_error())
            assert paths(qb3, p, len(rects)) == [1] * len(rects) and all(L.qb3x_window_ok(p, i) == 1 for i in range(len(rects))), what
            assert L.qb3x_last_window_segments(p) == sum(W.brute_segments(Wd, Ht, *r) for r in rects)
            if hbuf is None:
                check_host(lay, hbuf2, rows)
                hbuf = hbuf2
            assert np.array_equal(hbuf2, hbuf), what
            assert counters(qb3, p) == R.plan_bytes(Wd, Ht, rects, tab, 0, all_chunks if again else ()) == (src.bytes_logged(), len(src.log)), what
            if again:
                ranges = [tab.chunk_range(k) for k in range(len(tab.chunks))]
                assert all(off >= tab.D // 4 * 4 and (off, n) not in ranges for off, n in src.log)
        # gaps: fewer reads, at least as many bytes, the same pixels
        some = rects[5:] if Wd * Ht < 200000 else [r for r in rects if r[2] < Wd // 2][:8]
        sub = Layout(some, bands, 1, "cf8")
        got = {}
        for gap in (0, 64, 1 << 20):
            L.qb3x_set_ranged_gap(p, gap)
            del src.log[:]
            hb = np.full(sub.size, SENTINEL, np.uint8)
            assert host_call(qb3, p, sub, hb) == len(some), what
            check_host(sub, hb, rows)
            got[gap] = counters(qb3, p)
            assert got[gap] == R.plan_bytes(Wd, Ht, some, tab, gap, all_chunks) == (src.bytes_logged(), len(src.log)), (what, gap)
        assert got[0][1] >= got[64][1] >= got[1 << 20][1] >= 1 and got[0][0] <= got[64][0] <= got[1 << 20][0]
        if len(R.plan_pieces(Wd, Ht, some, tab, 0)) > 1:
            assert got[1 << 20][1] < got[0][1]
        L.qb3x_set_ranged_gap(p, 0)
        # device destinations: window k starts k % 4 bytes behind a dword; rows tight, a few bytes wider, whole dwords wider
        del src.log[:]
        dbuf = lay.buffer()
        assert {(dbuf.data_ptr() + o) % 4 for o in lay.offs} == {0, 1, 2, 3}
        extra = [sb - r[2] * bands for sb, r in zip(lay.sbytes, rects)]
        assert 0 in extra and any(e % 4 for e in extra) and any(e and e % 4 == 0 for e in extra)
        assert device_call(qb3, p, lay, dbuf) == len(rects), (what, qb3.last_error())
        assert paths(qb3, p, len(rects)) == [1] * len(rects), what
        lay.check(dbuf, rows)
        assert np.array_equal(dbuf.cpu().numpy(), hbuf), what
        assert counters(qb3, p) == R.plan_bytes(Wd, Ht, rects, tab, 0, all_chunks) == (src.bytes_logged(), len(src.log)), what
        assert not src.outside
        L.qb3_destroy_decoder(p)


def test_one_launch_of_the_kernel_that_applies(qb3, oracle):
    """from the library's profile: a batch of a common-factor raster is ONE dec_window_best_ranged launch -- no whole decode
    (dec_units), no window kernel over a container in device memory (dec_window_best), no other ranged kernel; an 8-bit FTL RGB
    handle with the bit set still goes through dec_window_ranged alone"""
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht = 260, 37
    L.qb3x_profile_enable(1)
    try:
        for bands, mode, level, want in ((3, BEST, 2, (1, 0)), (4, CF_H, 1, (1, 0)), (1, CF, 2, (1, 0)), (3, 8, 2, (0, 1))):
            img = device_raster(oracle, "mixed", Wd, Ht, bands, 1) if mode != 8 else synth.generate(Wd, Ht, bands, 0, "NOISY3", 1)
            src, p, _ = open_source(qb3, host_container(qb3, img, 0, mode, level), BIT)
            rects = W16.windows(Wd, Ht, 4, 64, 8)
            lay = Layout(rects, bands, 1, "cf8")
            buf = lay.buffer()
            L.qb3x_profile_reset()
            assert device_call(qb3, p, lay, buf) == len(rects) and paths(qb3, p, len(rects)) == [1] * len(rects)
            lay.check(buf, as_rows(img, Ht))
            assert (count(qb3, "dec_window_best_ranged"), count(qb3, "dec_window_ranged")) == want, (bands, mode)
            assert count(qb3, "dec_units") == 0 and count(qb3, "dec_window_best") == 0 and count(qb3, "dec_window") == 0
            assert count(qb3, "dec_window16_ranged") == 0
            L.qb3_destroy_decoder(p)
    finally:
        L.qb3x_profile_enable(0)


def test_quanta(qb3, oracle):
    """QB3M_CF_H with quanta 3: the crop of the whole decode, every window dequantised as a raster of its own"""
    import torch
    Wd, Ht, b = 260, 37, 3
    img = device_raster(oracle, "mixed", Wd, Ht, b, 11)
    d_c, n, _ = make_container(qb3, img, 0, CF_H, 2, quanta=3)
    want = full_decode(qb3, d_c, n)[0]
    assert want is not None and not torch.equal(want, img.reshape(-1))
    src, p, _ = open_source(qb3, d_c[:n].cpu().numpy(), BIT)
    assert qb3.lib.qb3_get_mode(p) == 5
    rects = W16.windows(Wd, Ht, 3, 64, 8)
    lay = Layout(rects, b, 1, "cf8")
    hbuf = np.full(lay.size, SENTINEL, np.uint8)
    assert host_call(qb3, p, lay, hbuf) == len(rects)
    check_host(lay, hbuf, want.view(Ht, -1))
    assert paths(qb3, p, len(rects)) == [1] * len(rects)
    dbuf = lay.buffer()
    assert device_call(qb3, p, lay, dbuf) == len(rects) and paths(qb3, p, len(rects)) == [1] * len(rects)
    lay.check(dbuf, want.view(Ht, -1))
    qb3.lib.qb3_destroy_decoder(p)


def test_python_interface(qb3, oracle, tmp_path):
    import torch
    from qb3_amd import device as qdev
    Wd, Ht, b = 260, 100, 4
    img = device_raster(oracle, "mixed", Wd, Ht, b, 8)
    c = host_container(qb3, img, 0, BEST)
    assert int(c[10]) == 5
    path = tmp_path / "a.qb3"
    c.tofile(path)
    rects = [(13, 21, 101, 55), (0, 0, 1, 1), (250, 90, 10, 7)]
    host = img.cpu().numpy()
    with qb3.open_ranged(str(path)) as rd:              # the default: read whole
        rd.read_windows(rects)
        assert rd.last_windows == [2, 2, 2] and rd.last_bytes >= len(c)
    with qb3.open_ranged(str(path), window_kernels=qb3.QB3X_WINK_CF8) as rd:
        got = rd.read_windows(rects)
        assert rd.last_windows == [1, 1, 1] and 0 < rd.last_bytes < len(c)
        rd.set_window_kernels(0)
        rd.read_windows(rects)
        assert rd.last_windows == [2, 2, 2] and rd.last_bytes >= len(c)
    for g, (x0, y0, w, h) in zip(got, rects):
        assert g.shape == (h, w, b) and g.dtype == np.uint8 and np.array_equal(g, host[y0:y0 + h, x0:x0 + w])
    rd = qdev.RangedDecoder(lambda off, n: bytes(c[off:off + n]), size=len(c), window_kernels=BIT)
    outs = rd.decode_windows(rects)
    assert rd.last_windows == [1, 1, 1] and 0 < rd.last_bytes < len(c)
    for g, (x0, y0, w, h) in zip(outs, rects):
        assert g.is_cuda and g.shape == (h, w, b) and torch.equal(g, img[y0:y0 + h, x0:x0 + w])
    rd.close()


# ---------------------------------------------------------------------------------------------------------------- falling back
def test_not_taken(qb3, oracle):
    """the bit unset on an RGB QB3M_CF_H container, and QB3X_WINK_U16 alone (path 2: strips of the whole container); the bit set on
    8-bit x 2 in QB3M_CF_H (path 2) and on a QB3M_BEST container whose RLE0 pass won (all zeros: the mode byte says 7; path 3): the
    whole container read once a call, the right pixels.  A STORED container (the oracle's: random bytes do not code) has no table and
    no stream: its rows are read from their offsets, path 3, the same reads with the bit and without"""
    import torch
    L = qb3.lib
    Wd, Ht = 260, 37
    rects = W16.windows(Wd, Ht, 41, 64, 8)
    img = device_raster(oracle, "mixed", Wd, Ht, 3, 3)
    c = host_container(qb3, img, 0, CF_H)
    assert int(c[10]) == 5
    check_fallback(qb3, c, as_rows(img, Ht), Layout(rects, 3, 1, "cf8"), (2,), mask=0)
    check_fallback(qb3, c, as_rows(img, Ht), Layout(rects, 3, 1, "cf8"), (2,), mask=W16.QB3X_WINK_U16)
    img2 = device_raster(oracle, "mixed", Wd, Ht, 2, 3)
    check_fallback(qb3, host_container(qb3, img2, 0, CF_H), as_rows(img2, Ht), Layout(rects, 2, 1, "cf8"), (2,), BIT)
    zeros = torch.zeros((Ht, Wd, 3), dtype=torch.uint8, device="cuda")
    c = host_container(qb3, zeros, 0, BEST)
    assert int(c[10]) == 7
    check_fallback(qb3, c, as_rows(zeros, Ht), Layout(rects, 3, 1, "cf8"), (3,), BIT)
    noise = oracle.generate(Wd, Ht, 3, 0, "RANDOM", 5)
    s = np.asarray(oracle.encode(noise, 0, CF_H), np.uint8)
    lay = Layout(rects, 3, 1, "cf8")
    asked = []
    for mask in (0, BIT):
        src, p, _ = open_source(qb3, s, mask)
        assert L.qb3_get_mode(p) == 255
        hbuf = np.full(lay.size, SENTINEL, np.uint8)
        assert host_call(qb3, p, lay, hbuf) == len(rects)
        check_host(lay, hbuf, torch.from_numpy(noise.reshape(Ht, -1)).cuda())
        assert paths(qb3, p, len(rects)) == [3] * len(rects) and not src.outside
        asked.append((list(src.log), counters(qb3, p)))
        L.qb3_destroy_decoder(p)
    assert asked[0] == asked[1]


@pytest.mark.parametrize("bands", WB.BANDS)
def test_damaged_tables_cost_time_and_bytes(qb3, oracle, bands):
    """the chunk that holds the entries of the window's segments, damaged.  A flipped entry byte under the old check fails the host's
    check before a byte of the stream is asked for: every window from the whole container, once.  Under a check sealed again, a
    block's length and a block's entering rung pass it and are caught by the kernel's consistency tests (where a block's units end,
    the rung they leave): singly and inside a batch only the windows that hold the damaged segment fall back, the others keep path
    1; the pixels are the source's, and the bytes are the plan's plus the whole container, once"""
    L = qb3.lib
    Wd, Ht = 1001, 259
    img = device_raster(oracle, "mixed", Wd, Ht, bands, 5)
    rows = as_rows(img, Ht)
    c = host_container(qb3, img, 0, CF_H)
    assert int(c[10]) == 5
    tab = R.Table(c).shape(R.entry_bytes("cf8", bands), R.HEAD_FLAGS)
    nbx = (Wd + 3) // 4
    seg = (6 * nbx + 10) // 64 + 1                      # the second segment of block row 6 from column 10
    holds = [(40, 24, 300, 40), (120, 20, 120, 8)]
    beside = [(600, 24, 100, 4), (5, 200, 50, 50)]
    assert all(seg in segments_of(Wd, Ht, r) for r in holds) and not any(seg in segments_of(Wd, Ht, r) for r in beside)
    e0 = tab.entry_offset(seg)
    lay = Layout(holds + beside, bands, 1, "cf8")
    for at in (e0 + WB.field_at(bands, 9), e0 + 7, tab.chunks[0][0] + 6):          # unsealed: a field, an entering value, the check itself
        bad = c.copy()
        bad[at] ^= 0x10
        check_fallback(qb3, bad, rows, lay, (3,), BIT)

    def longer(b):                          # block 5's length + 1
        at = e0 + WB.field_at(bands, 5)
        f = int(b[at]) | int(b[at + 1]) << 8
        f = (f & 0xf000) | ((f + 1) & 0xfff)
        b[at], b[at + 1] = f & 255, f >> 8

    def other_rung(b):                      # block 5 entered one rung higher in band 0
        at = e0 + WB.field_at(bands, 5) + 1
        b[at] = (int(b[at]) & 0x8f) | ((((int(b[at]) >> 4) & 7) + 1) & 7) << 4

    for what, change in (("length", longer), ("rung", other_rung)):
        bad = c.copy()
        change(bad)
        assert not np.array_equal(bad, c)
        R.seal(bad, tab.chunks[seg // tab.N][0])
        src, p, _ = open_source(qb3, bad, BIT)
        one = Layout(holds[:1], bands, 1, "cf8")                  # singly: the window falls back, from the whole container
        hb = np.full(one.size, SENTINEL, np.uint8)
        assert host_call(qb3, p, one, hb) == 1, what
        check_host(one, hb, rows)
        assert paths(qb3, p, 1) == [3] and src.log.count((0, len(c))) == 1 and not src.outside, what
        assert counters(qb3, p)[0] == R.plan_bytes(Wd, Ht, holds[:1], tab)[0] + len(c), what
        one = Layout(beside[:1], bands, 1, "cf8")                 # ... and a window beside the damage does not
        hb = np.full(one.size, SENTINEL, np.uint8)
        del src.log[:]
        assert host_call(qb3, p, one, hb) == 1 and paths(qb3, p, 1) == [1] and (0, len(c)) not in src.log, what
        check_host(one, hb, rows)
        L.qb3_destroy_decoder(p)
        src, p, _ = open_source(qb3, bad, BIT)               # inside a batch, device and host destinations
        buf = lay.buffer()
        assert device_call(qb3, p, lay, buf) == len(lay.rects), what
        lay.check(buf, rows)
        assert paths(qb3, p, len(lay.rects)) == [3] * len(holds) + [1] * len(beside), what
        assert src.log.count((0, len(c))) == 1 and not src.outside
        assert counters(qb3, p)[0] == R.plan_bytes(Wd, Ht, lay.rects, tab)[0] + len(c), what
        del src.log[:]
        hbuf = np.full(lay.size, SENTINEL, np.uint8)
        assert host_call(qb3, p, lay, hbuf) == len(lay.rects), what
        check_host(lay, hbuf, rows)
        assert paths(qb3, p, len(lay.rects)) == [3] * len(holds) + [1] * len(beside), what
        assert src.log.count((0, len(c))) == 1 and not src.outside
        L.qb3_destroy_decoder(p)


@pytest.mark.parametrize("bands", WB.BANDS)
def test_truncated_stream(qb3, oracle, bands):
    """a container cut in front of, inside and behind the segments of a window (block rows 2 and 3 of 256 x 24: segments 2 and 3 of
    six), its size passed truthfully: whatever qb3x_read_windows makes of the same bytes with the same bit, byte for byte.  The shape
    has no shifted edge block, so every pixel has one writer in the whole decode (the finding of the 16-bit ranged
    section)"""
    L = qb3.lib
    Wd, Ht = SMALLEST
    assert Wd % 4 == 0 and Ht % 4 == 0
    img = device_raster(oracle, "mixed", Wd, Ht, bands, 4)
    c = host_container(qb3, img, 0, BEST)
    assert int(c[10]) == 5
    tab = R.Table(c).shape(R.entry_bytes("cf8", bands), R.HEAD_FLAGS)
    assert tab.K == 6
    rects = [(8, 8, 200, 8)] + W16.windows(Wd, Ht, 6, 64, 8)
    assert segments_of(Wd, Ht, rects[0]) == {2, 3}
    lay = Layout(rects, bands, 1, "cf8")
    cuts = (tab.D + (tab.pos(1) + tab.pos(2)) // 16, tab.D + (tab.pos(3) + tab.pos(4)) // 16, tab.D + tab.pos(5) // 8 + 5, len(c) - 3)
    assert tab.D < cuts[0] < tab.D + tab.pos(2) // 8 <= tab.D + tab.pos(3) // 8 < cuts[1] < tab.D + tab.pos(4) // 8 < cuts[2] < len(c)
    for cut in cuts:
        short = c[:cut].copy()
        want = np.full(lay.size, SENTINEL, np.uint8)
        ref, _ = W.open_handle(L, short)
        L.qb3x_set_decoder_window_kernels(ref, BIT)
        n_ref = L.qb3x_read_windows(ref, qb3.window_array(rects, [want.ctypes.data + o for o in lay.offs], lay.strides()), len(rects))
        ref_paths = [L.qb3x_window_path(ref, i) for i in range(len(rects))]
        L.qb3_destroy_decoder(ref)
        src, p, _ = open_source(qb3, short, BIT)
        hbuf = np.full(lay.size, SENTINEL, np.uint8)
        assert host_call(qb3, p, lay, hbuf) == n_ref, cut
        assert [bool(v) for v in paths(qb3, p, len(rects))] == [bool(v) for v in ref_paths]
        if n_ref == len(rects):
            assert np.array_equal(hbuf, want), cut
        assert not src.outside
        L.qb3_destroy_decoder(p)


def test_a_small_window_reads_a_small_part(qb3):
    """Derived, not measured.  A 64 x 64 window in the middle of a 2051 x 1030 x 4 raster (513 blocks a row) has at most 17 block
    rows, each a run of at most two segments.  The host takes no run longer than its segments' staging, px_cap_dw words a segment:
    64 blocks x 4 bands x 176 bits (the longest common-factor unit of 8-bit data: 149 of a plain unit, 27 of signal, flags, rung
    switch and factor) in words, + 2.  It reads at most three table chunks (two that hold the window's entries, and the last), none
    longer than a chunk's 16-bit length + pad + mark.  NOISY3 codes to more than three bits a value (three bits of noise), a stream
    of 3 MB or more.  So a cold call asks the reader for less than a fifth of the container -- and for exactly the plan computed
    from the container's table beforehand"""
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht, b = 2051, 1030, 4
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 9)
    c = host_container(qb3, img, 0, BEST)
    assert int(c[10]) == 5 and len(c) >= 3 << 20
    tab = R.Table(c).shape(R.entry_bytes("cf8", b), R.HEAD_FLAGS)
    r = ((Wd - 64) // 2, (Ht - 64) // 2, 64, 64)
    cap_dw = (64 * b * 176 + 31) // 32 + 2
    bound = 17 * 2 * cap_dw * 4 + 3 * (R.CHUNK_MAX + R.IX_PAD + 2)
    assert W.brute_segments(Wd, Ht, *r) <= 17 * 2 and len(R.plan_chunks(Wd, Ht, [r], tab.K, tab.N)) <= 3
    want = R.plan_bytes(Wd, Ht, [r], tab)
    print("plan %d bytes in %d reads, bound %d, container %d" % (want[0], want[1], bound, len(c)))
    assert want[0] <= bound < len(c) // 5
    src, p, _ = open_source(qb3, c, BIT)
    lay = Layout([r], b, 1, "cf8")
    hbuf = np.full(lay.size, SENTINEL, np.uint8)
    assert host_call(qb3, p, lay, hbuf) == 1 and L.qb3x_last_window_path(p) == 1
    check_host(lay, hbuf, as_rows(img, Ht))
    assert counters(qb3, p) == want == (src.bytes_logged(), len(src.log)) and not src.outside
    L.qb3_destroy_decoder(p)


# ---------------------------------------------------------------------------------------------------------------- the tool
def test_qb3window_reads_a_common_factor_file_in_pieces_with_K(qb3, oracle, tmp_path):
    """qb3window on an 8-bit RGB QB3M_BEST file: with -K the crop from a part of the file on path 1, without it the same crop from
    the whole file"""
    import subprocess
    Wd, Ht, b = 260, 100, 3
    img = device_raster(oracle, "mixed", Wd, Ht, b, 3)
    c = host_container(qb3, img, 0, BEST)
    assert int(c[10]) == 5
    c.tofile(tmp_path / "a.qb3")
    x0, y0, w, h = 101, 37, 120, 40
    want = img.cpu().numpy()[y0:y0 + h, x0:x0 + w]
    hdr = b"P6\n%d %d\n255\n" % (w, h)
    tool = os.path.join(os.path.dirname(qb3.LIB_PATH), "qb3window")
    for flags, path in ((["-K"], 1), ([], 2)):
        r = subprocess.run([tool, "-v"] + flags + [str(tmp_path / "a.qb3"), "%d,%d,%d,%d" % (x0, y0, w, h), str(tmp_path / "win.pnm")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = (tmp_path / "win.pnm").read_bytes()
        assert got.startswith(hdr) and np.array_equal(np.frombuffer(got[len(hdr):], np.uint8).reshape(h, w, b), want)
        assert "on path %d" % path in r.stdout
        nbytes = int(r.stdout.split(": ")[-1].split(" bytes")[0])
        assert (0 < nbytes < len(c)) if path == 1 else nbytes >= len(c)
