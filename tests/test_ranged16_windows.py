"""Ranged window reads of 16-bit rasters on the device (include/qb3x.h: QB3X_WINK_U16 on a handle of qb3x_open_ranged;
k_dec_wins16_ranged.hip).  The invariant is the window calls': every window is the crop of what the whole decode writes, nothing
outside a window's rows is written.  Expected bytes are the crop of the SOURCE raster (lossless containers) or of
qb3x_decode_device on a second handle (quanta), never of a window call.  What the reader is asked for is the range rule of qb3x.h
with the raster's blocks per segment, restated in qb3_ranged.py and computed from the container's own table -- and the whole
container, once, wherever the shortcut is not taken.  Containers are written by this library at level 2 and held in a numpy
buffer behind a reader that logs its calls."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_ranged as R  # noqa: E402
import qb3_window as W  # noqa: E402
import qb3_window16 as W16  # noqa: E402
from qb3_ranged import check_fallback, check_host, counters, device_call, host_call, host_container, open_source  # noqa: E402
from qb3_window_dev import FTL, BASE, BASE_Z, CF_H, SENTINEL, Layout, as_rows, count, full_decode, make_container, paths  # noqa: E402

pytestmark = pytest.mark.gpu

U16, I16 = W16.U16, W16.I16
BIT = W16.QB3X_WINK_U16


class Placed(Layout):
    """tight windows at chosen addresses: window k starts at a multiple of 16 plus mods[k] bytes"""

    def __init__(self, rects, pix, mods):
        self.rects, self.pix, self.tsz, self.offs, self.sbytes = rects, pix, 2, [], []
        at = 16
        for (x0, y0, w, h), m in zip(rects, mods):
            at = (at + 15) // 16 * 16 + m
            self.offs.append(at)
            self.sbytes.append(w * pix)
            at += h * w * pix + 6
        self.size = at + 64


def segment_size(qb3, p, Wd, Ht):
    bps = C.c_size_t()
    qb3.lib.qb3x_window_segments(p, 0, 0, Wd, Ht, C.byref(bps))
    return bps.value


# ---------------------------------------------------------------------------------------------------------------- parity
PARITY = [(b, s) for b in (1, 2, 3, 4, 6, 8) for s in (W16.shapes_of(b) if b in (4, 8) else (W16.shapes_of(b)[0], W16.shapes_of(b)[3]))]


@pytest.mark.parametrize("case", PARITY, ids=lambda c: "%d-%dx%d" % (c[0], c[1][0], c[1][1]))
def test_windows_from_pieces(qb3, case):
    """FTL, BASE, BASE_Z; LANDSAT16 and DEM in turn; uint16, and int16 for the BASE container of 1, 4 and 8 bands.  Every rectangle as
    a single host call, then all as one batch on a fresh handle, twice (the second reads no table chunk); a positive gap; device
    destinations 0 and 2 bytes behind a dword with tight, wide-even and wide-odd rows (for eight bands also tight rows on and off a
    16-byte address: both store forms): the crop of the source raster, sentinels intact, path 1, the window's segments, and the
    reader asked for exactly the bytes of the plan."""
    from qb3_amd import synth
    L = qb3.lib
    bands, (Wd, Ht) = case
    pix, E, B = 2 * bands, R.entry_bytes("u16", bands), R.blocks_per_segment("u16", bands)
    rects = W16.windows(Wd, Ht, 5 * Wd + bands, B, 16)
    for turn, mode in enumerate((FTL, BASE, BASE_Z)):
        dt = I16 if mode == BASE and bands in (1, 4, 8) else U16
        img = synth.generate(Wd, Ht, bands, dt, ("LANDSAT16", "DEM")[(turn + bands + Wd) % 2], 31 * bands + Wd)
        rows = as_rows(img, Ht)
        c = host_container(qb3, img, dt, mode)
        tab = R.Table(c).shape(E)
        src, p, dims = open_source(qb3, c, BIT)
        assert dims == (Wd, Ht, bands) and L.qb3_get_mode(p) == mode and L.qb3x_decoder_table_entries(p) == tab.K
        assert segment_size(qb3, p, Wd, Ht) == B
        lay = Layout(rects, pix, 2, "u16")
        # single calls
        hbuf = np.full(lay.size, SENTINEL, np.uint8)
        cached = set()
        for k, r in enumerate(rects):
            del src.log[:]
            assert host_call(qb3, p, lay, hbuf, k) == 1, (r, qb3.last_error())
            assert L.qb3x_window_path(p, 0) == 1 and L.qb3x_last_window_path(p) == 1, r
            assert L.qb3x_last_window_segments(p) == W.brute_segments(Wd, Ht, *r, bps=B), r
            want = R.plan_bytes(Wd, Ht, [r], tab, 0, cached, B)
            assert counters(qb3, p) == want == (src.bytes_logged(), len(src.log)), r
            cached.update(R.plan_chunks(Wd, Ht, [r], tab.K, tab.N, B))
        check_host(lay, hbuf, rows)
        assert not src.outside
        # one batch, on a fresh handle (an empty cache), twice: the second reads no table chunk
        L.qb3_destroy_decoder(p)
        src, p, _ = open_source(qb3, c, BIT)
        all_chunks = set(range(len(tab.chunks)))
        for again in (False, True):
            del src.log[:]
            hbuf2 = np.full(lay.size, SENTINEL, np.uint8)
            assert host_call(qb3, p, lay, hbuf2) == len(rects), qb3.last_error()
            assert paths(qb3, p, len(rects)) == [1] * len(rects) and all(L.qb3x_window_ok(p, i) == 1 for i in range(len(rects)))
            assert L.qb3x_last_window_segments(p) == sum(W.brute_segments(Wd, Ht, *r, bps=B) for r in rects)
            assert np.array_equal(hbuf2, hbuf)
            assert counters(qb3, p) == R.plan_bytes(Wd, Ht, rects, tab, 0, all_chunks if again else (), B) == (src.bytes_logged(), len(src.log))
            if again:
                ranges = [tab.chunk_range(k) for k in range(len(tab.chunks))]
                assert all(off >= tab.D // 4 * 4 and (off, n) not in ranges for off, n in src.log)
        # gaps: fewer reads, at least as many bytes, the same pixels
        some = rects[5:] if Wd * Ht < 200000 else [r for r in rects if r[2] < Wd // 2][:8]
        sub = Layout(some, pix, 2, "u16")
        got = {}
        for gap in (0, 64, 1 << 20):
            L.qb3x_set_ranged_gap(p, gap)
            del src.log[:]
            hb = np.full(sub.size, SENTINEL, np.uint8)
            assert host_call(qb3, p, sub, hb) == len(some)
            check_host(sub, hb, rows)
            got[gap] = counters(qb3, p)
            assert got[gap] == R.plan_bytes(Wd, Ht, some, tab, gap, all_chunks, B) == (src.bytes_logged(), len(src.log)), gap
        assert got[0][1] >= got[64][1] >= got[1 << 20][1] >= 1 and got[0][0] <= got[64][0] <= got[1 << 20][0]
        if len(R.plan_pieces(Wd, Ht, some, tab, 0, B)) > 1:
            assert got[1 << 20][1] < got[0][1]
        L.qb3x_set_ranged_gap(p, 0)
        # device destinations: window k starts k % 8 halfwords behind a dword; rows tight, wide-even, wide-odd
        del src.log[:]
        dbuf = lay.buffer()
        assert {(dbuf.data_ptr() + o) % 4 for o in lay.offs} == {0, 2}
        assert device_call(qb3, p, lay, dbuf) == len(rects), qb3.last_error()
        assert paths(qb3, p, len(rects)) == [1] * len(rects)
        lay.check(dbuf, rows)
        assert np.array_equal(dbuf.cpu().numpy(), hbuf)
        assert counters(qb3, p) == R.plan_bytes(Wd, Ht, rects, tab, 0, all_chunks, B) == (src.bytes_logged(), len(src.log))
        if bands == 8:          # whole blocks of tight windows whose rows lie on a 16-byte address, 8 behind one, 4 and 2 behind one
            inner = [r for r in rects if r[2] >= 12 and r[3] >= 4][:8]
            mods = [(0, 8, 4, 2)[k % 4] for k in range(len(inner))]
            pl = Placed(inner, pix, mods)
            dbuf = pl.buffer()
            assert len(inner) >= 4 and sorted({(dbuf.data_ptr() + o) % 16 for o in pl.offs}) == [0, 2, 4, 8] and all(sb % 16 == 0 for sb in pl.sbytes)
            assert device_call(qb3, p, pl, dbuf) == len(inner) and paths(qb3, p, len(inner)) == [1] * len(inner)
            pl.check(dbuf, rows)
        assert not src.outside
        L.qb3_destroy_decoder(p)


def test_one_launch_of_the_kernel_that_applies(qb3):
    """a 16-bit batch is ONE dec_window16_ranged launch and no dec_window_ranged; an 8-bit RGB handle with the bit set is the reverse"""
    from qb3_amd import synth
    L = qb3.lib
    L.qb3x_profile_enable(1)
    try:
        for bands, dt, gen, pix, want in ((4, U16, "LANDSAT16", 8, (1, 0)), (3, 0, "NOISY3", 3, (0, 1))):
            img = synth.generate(260, 37, bands, dt, gen, 1)
            src, p, _ = open_source(qb3, host_container(qb3, img, dt, FTL), BIT)
            rects = W16.windows(260, 37, 4, 64, 8)
            lay = Layout(rects, pix, 2, "u16") if dt else Layout(rects, pix, 1, "u8")
            buf = lay.buffer()
            L.qb3x_profile_reset()
            assert device_call(qb3, p, lay, buf) == len(rects) and paths(qb3, p, len(rects)) == [1] * len(rects)
            lay.check(buf, as_rows(img, 37))
            assert (count(qb3, "dec_window16_ranged"), count(qb3, "dec_window_ranged")) == want
            assert count(qb3, "dec_window16") == 0 and count(qb3, "dec_window") == 0
            L.qb3_destroy_decoder(p)
    finally:
        L.qb3x_profile_enable(0)


def test_quanta(qb3):
    """BASE with quanta 3: the crop of the whole decode, every window dequantised as a raster of its own"""
    import torch
    from qb3_amd import synth
    Wd, Ht, b = 260, 37, 4
    img = synth.generate(Wd, Ht, b, U16, "LANDSAT16", 11)
    d_c, n, _ = make_container(qb3, img, U16, BASE, 2, quanta=3)
    want = full_decode(qb3, d_c, n)[0]
    assert want is not None and not torch.equal(want, img.reshape(-1).view(torch.uint8))
    src, p, _ = open_source(qb3, d_c[:n].cpu().numpy(), BIT)
    rects = W16.windows(Wd, Ht, 3, 64, 8)
    lay = Layout(rects, 2 * b, 2, "u16")
    hbuf = np.full(lay.size, SENTINEL, np.uint8)
    assert host_call(qb3, p, lay, hbuf) == len(rects)
    check_host(lay, hbuf, want.view(Ht, -1))
    assert paths(qb3, p, len(rects)) == [1] * len(rects)
    dbuf = lay.buffer()
    assert device_call(qb3, p, lay, dbuf) == len(rects) and paths(qb3, p, len(rects)) == [1] * len(rects)
    lay.check(dbuf, want.view(Ht, -1))
    qb3.lib.qb3_destroy_decoder(p)


def test_python_interface(qb3, tmp_path):
    import torch
    from qb3_amd import device as qdev, synth
    Wd, Ht, b = 260, 100, 2
    img = synth.generate(Wd, Ht, b, U16, "DEM", 8)
    c = host_container(qb3, img, U16, FTL)
    path = tmp_path / "a.qb3"
    c.tofile(path)
    rects = [(13, 21, 101, 55), (0, 0, 1, 1), (250, 90, 10, 7)]
    host = img.cpu().numpy()
    with qb3.open_ranged(str(path)) as rd:              # the default: read whole
        rd.read_windows(rects)
        assert rd.last_windows == [2, 2, 2] and rd.last_bytes >= len(c)
    with qb3.open_ranged(str(path), window_kernels=BIT) as rd:
        got = rd.read_windows(rects)
        assert rd.last_windows == [1, 1, 1] and 0 < rd.last_bytes < len(c)
        rd.set_window_kernels(0)
        rd.read_windows(rects)
        assert rd.last_windows == [2, 2, 2]
    for g, (x0, y0, w, h) in zip(got, rects):
        assert g.shape == (h, w, b) and g.dtype == np.uint16 and np.array_equal(g, host.view(np.uint16)[y0:y0 + h, x0:x0 + w])
    rd = qdev.RangedDecoder(lambda off, n: bytes(c[off:off + n]), size=len(c), window_kernels=BIT)
    outs = rd.decode_windows(rects)
    assert rd.last_windows == [1, 1, 1] and 0 < rd.last_bytes < len(c)
    for g, (x0, y0, w, h) in zip(outs, rects):
        assert g.is_cuda and g.shape == (h, w, b) and torch.equal(g.view(torch.uint8), img[y0:y0 + h, x0:x0 + w].contiguous().view(torch.uint8))
    rd.close()


# ---------------------------------------------------------------------------------------------------------------- falling back
def test_not_taken(qb3):
    """the bit unset on uint16 x 4; the bit set with one odd device destination in the batch; uint16 x 5; uint16 x 4 in QB3M_CF_H; a
    level-1 table: the whole container read once, the right pixels, the path reported today"""
    from qb3_amd import synth
    Wd, Ht = 260, 37
    rects = W16.windows(Wd, Ht, 41, 64, 8)
    img = synth.generate(Wd, Ht, 4, U16, "LANDSAT16", 3)
    rows = as_rows(img, Ht)
    c = host_container(qb3, img, U16, FTL)
    check_fallback(qb3, c, rows, Layout(rects, 8, 2, "u16"), (2,), mask=0)
    odd = Layout(rects, 8, 2, "u16")
    odd.offs[3] += 1                                   # (six sentinel bytes lie between two windows)
    check_fallback(qb3, c, rows, odd, (2,), BIT, host=False)
    img5 = synth.generate(Wd, Ht, 5, U16, "LANDSAT16", 3)
    check_fallback(qb3, host_container(qb3, img5, U16, FTL), as_rows(img5, Ht), Layout(rects, 10, 2, "u16"), (2,), BIT)
    check_fallback(qb3, host_container(qb3, img, U16, CF_H), rows, Layout(rects, 8, 2, "u16"), (2,), BIT)
    check_fallback(qb3, host_container(qb3, img, U16, FTL, level=1), rows, Layout(rects, 8, 2, "u16"), (3,), BIT)


@pytest.mark.parametrize("bands", (4, 8))
def test_damaged_tables_cost_time_and_bytes(qb3, bands):
    """a flipped entry byte fails the host's check: the whole container, once.  In chunks sealed again, an entry whose position is
    moved and one whose lane-length field is changed pass it and are caught by the kernel's consistency tests or by the bounds of
    the piece: status words, no fault, nothing outside the windows -- those windows come from the fallback, the others keep path 1"""
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht = 1001, 259
    pix, E, B = 2 * bands, R.entry_bytes("u16", bands), R.blocks_per_segment("u16", bands)
    img = synth.generate(Wd, Ht, bands, U16, "DEM", 5)
    rows = as_rows(img, Ht)
    c = host_container(qb3, img, U16, FTL)
    tab = R.Table(c).shape(E)
    nbx = (Wd + 3) // 4
    seg = (6 * nbx + 10) // B + 1                       # block row 6: its first block is column 30 for both segment sizes
    assert seg * B == 6 * nbx + 30
    holds = [(40, 24, 300, 40), (130, 26, 8, 1), (120, 20, 120, 8)]         # each has a block of segment seg
    beside = [(600, 24, 100, 4), (5, 200, 50, 50)]                          # none has a block of seg - 1, seg
    for r in beside:
        bx0, bx1, by0, by1, _ = R.block_rect(Wd, Ht, r)
        assert not {seg - 1, seg} & {(by * nbx + bx) // B for by in range(by0, by1 + 1) for bx in range(bx0, bx1 + 1)}
    e0 = tab.entry_offset(seg)
    lay = Layout(holds + beside, pix, 2, "u16")
    for at in (e0 + 7, e0 + 6 + 3 * bands + 11, tab.chunks[0][0] + 6, tab.chunks[-1][0] + tab.chunks[-1][1] - 1):
        bad = c.copy()
        bad[at] ^= 0x10
        check_fallback(qb3, bad, rows, lay, (3,), BIT)
    damaged = []
    for moved in (tab.pos(seg) + 40, tab.pos(seg + 2), tab.pos(seg - 3), tab.pos(seg + 1) + 8 * 4096, (1 << 48) - 1):
        bad = c.copy()
        bad[e0:e0 + 6] = np.frombuffer(int(moved).to_bytes(6, "little"), np.uint8)
        damaged.append(("position %d" % moved, bad))
    bad = c.copy()                                      # lane 5's first length field + 1
    fields, nf = e0 + 6 + 3 * bands, E - 6 - 3 * bands
    v = int.from_bytes(bytes(bad[fields:fields + nf]), "little")
    bit = 20 * 5
    v = (v & ~(1023 << bit)) | (((((v >> bit) & 1023) + 1) & 1023) << bit)
    bad[fields:fields + nf] = np.frombuffer(v.to_bytes(nf, "little"), np.uint8)
    damaged.append(("lane length", bad))
    for what, bad in damaged:
        R.seal(bad, tab.chunks[seg // tab.N][0])
        src, p, _ = open_source(qb3, bad, BIT)
        buf = lay.buffer()
        assert device_call(qb3, p, lay, buf) == len(lay.rects), what
        lay.check(buf, rows)
        assert paths(qb3, p, len(lay.rects)) == [3] * len(holds) + [1] * len(beside), what
        assert src.log.count((0, len(c))) == 1 and not src.outside
        hbuf = np.full(lay.size, SENTINEL, np.uint8)
        assert host_call(qb3, p, lay, hbuf) == len(lay.rects), what
        check_host(lay, hbuf, rows)
        assert paths(qb3, p, len(lay.rects)) == [3] * len(holds) + [1] * len(beside), what
        L.qb3_destroy_decoder(p)


@pytest.mark.parametrize("bands", (4, 8))
def test_truncated_stream(qb3, bands):
    """a container cut inside its last segments, its size passed truthfully: whatever qb3x_read_windows makes of the same bytes.
    The shape is the one of qb3_window16.py whose sides are multiples of 4 (256 x 24: 6 segments of 64 blocks, 12 of 32).  Behind
    the cut the whole decode -- where both calls send the windows that hold a cut segment -- decodes zeros, and it stores every
    block whole: where the last block row or column is shifted (1001 x 259) a cut block and its sound neighbour write different
    values to the pixels they share, and which of the two stays is not defined.  On that shape this test failed on an MI355X at a
    different cut from run to run, with all windows written and every ok flag equal; test_ranged_windows.py::test_truncated_stream
    uses 1000 x 300 for 8-bit data and has no such pixels.  With no shifted block every pixel has one writer and the two buffers
    must be equal byte for byte."""
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht = W16.SHAPES_NARROW[1]
    assert Wd % 4 == 0 and Ht % 4 == 0
    pix, E, B = 2 * bands, R.entry_bytes("u16", bands), R.blocks_per_segment("u16", bands)
    img = synth.generate(Wd, Ht, bands, U16, "LANDSAT16", 4)
    c = host_container(qb3, img, U16, BASE)
    tab = R.Table(c).shape(E)
    rects = W16.windows(Wd, Ht, 6, B, 8)
    lay = Layout(rects, pix, 2, "u16")
    strides = [0 if sb == r[2] * pix else sb // 2 for sb, r in zip(lay.sbytes, rects)]
    for cut in (tab.D + tab.pos(tab.K - 1) // 8 + 30, tab.D + tab.pos(tab.K - 2) // 8 - 5, len(c) - 3):
        short = c[:cut].copy()
        want = np.full(lay.size, SENTINEL, np.uint8)
        ref, _ = W.open_handle(L, short)
        L.qb3x_set_decoder_window_kernels(ref, BIT)
        n_ref = L.qb3x_read_windows(ref, qb3.window_array(rects, [want.ctypes.data + o for o in lay.offs], strides), len(rects))
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
    """Derived, not measured: a 64 x 64 window in the middle of a 2051 x 1030 x 4 raster touches at most 17 block rows x 2 segments
    of 64 blocks out of about 2070, and at most three table chunks of less than 64 KB; LANDSAT16 codes to more than 6 bits a value
    (six bits of noise), a stream of 7 MB or more.  So a cold call asks the reader for less than a tenth of the container -- and
    for exactly the plan computed from the container's table beforehand"""
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht, b = 2051, 1030, 4
    img = synth.generate(Wd, Ht, b, U16, "LANDSAT16", 9)
    c = host_container(qb3, img, U16, FTL)
    assert len(c) >= 7 << 20
    tab = R.Table(c).shape(R.entry_bytes("u16", b))
    r = ((Wd - 64) // 2, (Ht - 64) // 2, 64, 64)
    assert W.brute_segments(Wd, Ht, *r) <= 17 * 2 and len(R.plan_chunks(Wd, Ht, [r], tab.K, tab.N, 64)) <= 3
    want = R.plan_bytes(Wd, Ht, [r], tab, B=64)
    assert want[0] < len(c) // 10
    src, p, _ = open_source(qb3, c, BIT)
    lay = Layout([r], 2 * b, 2, "u16")
    hbuf = np.full(lay.size, SENTINEL, np.uint8)
    assert host_call(qb3, p, lay, hbuf) == 1 and L.qb3x_last_window_path(p) == 1
    check_host(lay, hbuf, as_rows(img, Ht))
    assert counters(qb3, p) == want == (src.bytes_logged(), len(src.log)) and not src.outside
    L.qb3_destroy_decoder(p)


# ---------------------------------------------------------------------------------------------------------------- the tool
def test_qb3window_reads_a_16_bit_file_in_pieces_with_k(qb3, tmp_path):
    """qb3window on a uint16 RGB file with a level-2 table: with -k the crop from a part of the file on path 1, without it the same
    crop from the whole file (PNM samples are big endian)"""
    import subprocess
    from qb3_amd import synth
    Wd, Ht, b = 260, 100, 3
    img = synth.generate(Wd, Ht, b, U16, "LANDSAT16", 3)
    c = host_container(qb3, img, U16, FTL)
    c.tofile(tmp_path / "a.qb3")
    x0, y0, w, h = 101, 37, 120, 40
    want = img.cpu().numpy()[y0:y0 + h, x0:x0 + w]
    hdr = b"P6\n%d %d\n65535\n" % (w, h)
    tool = os.path.join(os.path.dirname(qb3.LIB_PATH), "qb3window")
    for flags, path in ((["-k"], 1), ([], 2)):
        r = subprocess.run([tool, "-v"] + flags + [str(tmp_path / "a.qb3"), "%d,%d,%d,%d" % (x0, y0, w, h), str(tmp_path / "win.pnm")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = (tmp_path / "win.pnm").read_bytes()
        assert got.startswith(hdr) and np.array_equal(np.frombuffer(got[len(hdr):], ">u2").reshape(h, w, b), want)
        assert "on path %d" % path in r.stdout
        nbytes = int(r.stdout.split(": ")[-1].split(" bytes")[0])
        assert (0 < nbytes < len(c)) if path == 1 else nbytes >= len(c)
