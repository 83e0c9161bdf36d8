"""Ranged window reads on the device (include/qb3x.h: qb3x_read_windows_ranged, qb3x_decode_windows_ranged).  The invariant is the
window calls': every window is the crop of what the whole decode writes, nothing outside a window's rows is written.  What is new is
what the reader is asked for: the table chunks and the pieces of the stream the range rule of qb3x.h names, restated in
qb3_ranged.py and computed from the container's own table -- and the whole container wherever the shortcut is not taken.
Containers are written by this library at level 2 and held in a numpy buffer behind a reader that logs its calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_ranged as R  # noqa: E402
import qb3_window as W  # noqa: E402
from qb3_ranged import check_fallback, check_host, counters, device_call, host_call, host_container  # noqa: E402
from qb3_window_dev import FTL, BASE, BASE_Z, SENTINEL, Layout, as_rows, full_decode, paths, to_device  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ((100, 100), (1000, 37), (1024, 260), (2051, 1030))


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("bands", (1, 3, 4))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_windows_from_pieces(qb3, shape, bands):
    """FTL, BASE, BASE_Z: every rectangle as a single call and all as one batch, tight and wide strides, host and device destinations
    (at all four byte alignments): the crop of the source raster, sentinels intact, path 1, and the reader asked for exactly the
    bytes of the plan, at gap 0 and at a positive gap.
    A rectangle of less than a quarter of the 2051 x 1030 raster reads less than the container: it touches at most half of a block
    row's segments in every block row, or all of them in a quarter of the rows -- at most half the stream, plus a table of 92 bytes
    per 64 blocks (about a tenth of such a stream)."""
    import torch
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht = shape
    img = synth.generate(Wd, Ht, bands, 0, "NOISY3", 31 * bands + Wd)
    rows = as_rows(img, Ht)
    rects = W.windows(Wd, Ht, 5 * Wd + bands, 24)
    for turn, mode in enumerate((FTL, BASE, BASE_Z)):
        c = host_container(qb3, img, 0, mode)
        tab = R.Table(c).shape(R.entry_bytes("u8", bands))
        src = R.Source(qb3, c)
        p, dims = src.open(qb3)
        assert p and dims == (Wd, Ht, bands) and L.qb3_get_mode(p) == mode and L.qb3x_decoder_table_entries(p) == tab.K
        lay = Layout(rects, bands, 1, "u8", start=turn)
        # single calls
        hbuf = np.full(lay.size, SENTINEL, np.uint8)
        cached = set()
        for k, r in enumerate(rects):
            del src.log[:]
            assert host_call(qb3, p, lay, hbuf, k) == 1, (r, qb3.last_error())
            assert L.qb3x_window_path(p, 0) == 1 and L.qb3x_last_window_path(p) == 1, r
            assert L.qb3x_last_window_segments(p) == W.brute_segments(Wd, Ht, *r)
            want = R.plan_bytes(Wd, Ht, [r], tab, 0, cached)
            assert counters(qb3, p) == want == (src.bytes_logged(), len(src.log)), r
            if shape == (2051, 1030) and r[2] * r[3] < Wd * Ht // 4:
                assert want[0] + sum(tab.chunk_range(k)[1] for k in cached) < len(c), r
            cached.update(R.plan_chunks(Wd, Ht, [r], tab.K, tab.N))
        check_host(lay, hbuf, rows)
        assert not src.outside
        # one batch, on a fresh handle (an empty cache), twice: the second reads no table chunk
        L.qb3_destroy_decoder(p)
        p, _ = src.open(qb3)
        for again in (False, True):
            del src.log[:]
            hbuf2 = np.full(lay.size, SENTINEL, np.uint8)
            assert host_call(qb3, p, lay, hbuf2) == len(rects), qb3.last_error()
            assert paths(qb3, p, len(rects)) == [1] * len(rects)
            assert all(L.qb3x_window_ok(p, i) == 1 for i in range(len(rects)))
            assert L.qb3x_last_window_segments(p) == sum(W.brute_segments(Wd, Ht, *r) for r in rects)
            assert np.array_equal(hbuf2, hbuf)
            all_chunks = set(range(len(tab.chunks)))
            assert counters(qb3, p) == R.plan_bytes(Wd, Ht, rects, tab, 0, all_chunks if again else ()) == (src.bytes_logged(), len(src.log))
            if again:
                # (a piece is widened to dwords: the first may start up to three bytes in front of the first stream byte, never at a chunk)
                ranges = [tab.chunk_range(k) for k in range(len(tab.chunks))]
                assert all(off >= tab.D // 4 * 4 and (off, n) not in ranges for off, n in src.log)
        # a positive gap: fewer reads, at least as many bytes, the same pixels (a window whose block rows lie apart in the stream)
        some = rects[5:] if Wd * Ht < 200000 else [r for r in rects if r[2] < Wd // 2][:8]
        sub = Layout(some, bands, 1, "u8", start=turn)
        got = {}
        for gap in (0, 64, 1 << 20):
            L.qb3x_set_ranged_gap(p, gap)
            hb = np.full(sub.size, SENTINEL, np.uint8)
            assert host_call(qb3, p, sub, hb) == len(some)
            check_host(sub, hb, rows)
            got[gap] = counters(qb3, p)
            assert got[gap] == R.plan_bytes(Wd, Ht, some, tab, gap, all_chunks), gap
        assert got[0][1] >= got[64][1] >= got[1 << 20][1] >= 1 and got[0][0] <= got[64][0] <= got[1 << 20][0]
        if len(R.plan_pieces(Wd, Ht, some, tab, 0)) > 1:
            assert got[1 << 20][1] < got[0][1]
        L.qb3x_set_ranged_gap(p, 0)
        # device destinations
        dbuf = lay.buffer()
        assert device_call(qb3, p, lay, dbuf) == len(rects), qb3.last_error()
        assert paths(qb3, p, len(rects)) == [1] * len(rects)
        lay.check(dbuf, rows)
        assert np.array_equal(dbuf.cpu().numpy(), hbuf)
        assert counters(qb3, p) == R.plan_bytes(Wd, Ht, rects, tab, 0, all_chunks)
        # the cache switched off: the chunks are read again, every call
        L.qb3x_set_ranged_cache(p, 0)
        for _ in range(2):
            dbuf = lay.buffer()
            assert device_call(qb3, p, lay, dbuf) == len(rects)
            assert counters(qb3, p) == R.plan_bytes(Wd, Ht, rects, tab, 0, ())
        lay.check(dbuf, rows)
        L.qb3_destroy_decoder(p)


def test_quanta(qb3):
    """BASE with quanta 3: the crop of the whole decode, every window dequantised as a raster of its own"""
    import torch
    from qb3_amd import synth
    Wd, Ht, b = 1000, 300, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 11)
    c = host_container(qb3, img, 0, BASE, quanta=3)
    want, st = full_decode(qb3, to_device(c), len(c))
    assert want is not None and not torch.equal(want, img.reshape(-1))
    src = R.Source(qb3, c)
    p, _ = src.open(qb3)
    rects = W.windows(Wd, Ht, 3, 12)
    lay = Layout(rects, b, 1, "u8")
    hbuf = np.full(lay.size, SENTINEL, np.uint8)
    assert host_call(qb3, p, lay, hbuf) == len(rects)
    check_host(lay, hbuf, want.view(Ht, -1))
    assert paths(qb3, p, len(rects)) == [1] * len(rects)
    dbuf = lay.buffer()
    assert device_call(qb3, p, lay, dbuf) == len(rects)
    lay.check(dbuf, want.view(Ht, -1))
    assert qb3.lib.qb3x_ranged_bytes(p) < len(c)
    qb3.lib.qb3_destroy_decoder(p)


def test_python_interface(qb3, tmp_path):
    import torch
    from qb3_amd import device as qdev, synth
    Wd, Ht, b = 700, 300, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 8)
    c = host_container(qb3, img, 0, FTL)
    path = tmp_path / "a.qb3"
    c.tofile(path)
    rects = [(13, 21, 101, 55), (0, 0, 1, 1), (250, 100, 33, 7)]
    host = img.cpu().numpy()
    with qb3.open_ranged(str(path)) as rd:
        assert (rd.width, rd.height, rd.bands) == (Wd, Ht, b)
        got = rd.read_windows(rects)
        assert rd.last_windows == [1, 1, 1] and 0 < rd.last_bytes < len(c) and rd.last_reads > 0
    for g, (x0, y0, w, h) in zip(got, rects):
        assert g.shape == (h, w, b) and g.dtype == np.uint8 and np.array_equal(g, host[y0:y0 + h, x0:x0 + w])
    calls = []
    rd = qdev.RangedDecoder(lambda off, n: (calls.append((off, n)), bytes(c[off:off + n]))[1], size=len(c))
    outs = rd.decode_windows(rects)
    assert rd.last_windows == [1, 1, 1] and rd.last_reads <= len(calls)
    for g, (x0, y0, w, h) in zip(outs, rects):
        assert g.is_cuda and torch.equal(g, img[y0:y0 + h, x0:x0 + w])
    rd.close()


# ---------------------------------------------------------------------------------------------------------------- falling back
def test_rasters_and_tables_the_shortcut_does_not_take(qb3, oracle):
    import torch
    from qb3_amd import synth
    img = synth.generate(1000, 520, 4, 2, "LANDSAT16", 3)                  # uint16 x 4, level 2: the strips of path 2
    check_fallback(qb3, host_container(qb3, img, 2, FTL), as_rows(img, 520), Layout(W.windows(1000, 520, 41, 8), 8, 2, "u8"), (2,))
    img = synth.generate(1000, 300, 3, 0, "NOISY3", 5)                      # a level-1 table
    check_fallback(qb3, host_container(qb3, img, 0, FTL, level=1), as_rows(img, 300), Layout(W.windows(1000, 300, 41, 8), 3, 1, "u8"), (3,))
    himg = oracle.generate(509, 259, 3, 0, "NOISY3", 5)                     # a plain container
    s = oracle.encode(himg, 0, FTL)
    check_fallback(qb3, s, torch.from_numpy(himg.reshape(259, -1)).cuda(), Layout(W.windows(509, 259, 41, 8), 3, 1, "u8"), (3,))


def test_damaged_tables_cost_time_and_bytes(qb3):
    """a flipped entry byte fails the host's check; an entry whose position is moved, in a chunk sealed again, passes it and is caught
    by the kernel's consistency tests or by the bounds of the piece: status words, no fault, nothing outside the windows"""
    import torch
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht, b = 2048, 1024, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 77)
    rows = as_rows(img, Ht)
    c = host_container(qb3, img, 0, FTL)
    tab = R.Table(c).shape(R.entry_bytes("u8", b))
    nbx = Wd // 4
    seg = (24 // 4) * nbx // 64 + 1                  # block row 6, blocks 64..127: pixels x 256..511, y 24..27
    holds = [(40, 24, 300, 40), (300, 26, 8, 1), (256, 20, 256, 8)]
    beside = [(600, 24, 100, 4), (5, 600, 50, 50)]
    e0 = tab.entry_offset(seg)
    for at in (e0 + 7, e0 + 6 + 2 * b + 11, tab.chunks[0][0] + 6, tab.chunks[-1][0] + tab.chunks[-1][1] - 1):
        bad = c.copy()
        bad[at] ^= 0x10
        check_fallback(qb3, bad, rows, Layout(holds + beside, b, 1, "u8"), (3,))
    for moved in (tab.pos(seg) + 40, tab.pos(seg + 2), tab.pos(seg - 3), tab.pos(seg + 1) + 8 * 4096, (1 << 48) - 1):
        bad = c.copy()
        bad[e0:e0 + 6] = np.frombuffer(int(moved).to_bytes(6, "little"), np.uint8)
        R.seal(bad, tab.chunks[0][0])
        check_fallback(qb3, bad, rows, Layout(holds, b, 1, "u8"), (3,))
        # ... and the windows beside the moved entry keep their shortcut
        src = R.Source(qb3, bad)
        p, _ = src.open(qb3)
        lay = Layout(holds + beside, b, 1, "u8")
        buf = lay.buffer()
        assert device_call(qb3, p, lay, buf) == len(lay.rects)
        lay.check(buf, rows)
        assert paths(qb3, p, len(lay.rects)) == [3] * len(holds) + [1] * len(beside), moved
        L.qb3_destroy_decoder(p)


def test_truncated_stream(qb3):
    """a container cut inside its last segments, its size passed truthfully: whatever qb3x_read_windows makes of the same bytes"""
    from qb3_amd import synth
    L = qb3.lib
    Wd, Ht, b = 1000, 300, 3
    img = synth.generate(Wd, Ht, b, 0, "NOISY3", 4)
    c = host_container(qb3, img, 0, BASE)
    tab = R.Table(c).shape(R.entry_bytes("u8", b))
    rects = W.windows(Wd, Ht, 6, 8)
    lay = Layout(rects, b, 1, "u8")
    for cut in (tab.D + tab.pos(tab.K - 1) // 8 + 30, tab.D + tab.pos(tab.K - 2) // 8 - 5, len(c) - 3):
        short = c[:cut].copy()
        strides = [0 if sb == r[2] * b else sb for sb, r in zip(lay.sbytes, rects)]
        want = np.full(lay.size, SENTINEL, np.uint8)
        ref, _ = W.open_handle(L, short)
        n_ref = L.qb3x_read_windows(ref, qb3.window_array(rects, [want.ctypes.data + o for o in lay.offs], strides), len(rects))
        ref_paths = [L.qb3x_window_path(ref, i) for i in range(len(rects))]
        L.qb3_destroy_decoder(ref)
        src = R.Source(qb3, short)
        p, _ = src.open(qb3)
        assert p
        hbuf = np.full(lay.size, SENTINEL, np.uint8)
        assert host_call(qb3, p, lay, hbuf) == n_ref, cut
        assert [bool(v) for v in paths(qb3, p, len(rects))] == [bool(v) for v in ref_paths]
        if n_ref == len(rects):
            assert np.array_equal(hbuf, want), cut
        assert not src.outside
        L.qb3_destroy_decoder(p)


# ---------------------------------------------------------------------------------------------------------------- the tool
def test_qb3window_gives_the_crop_of_the_decoded_file(qb3, oracle, tmp_path):
    """qb3window on a file cqb3x wrote with QB3X_INDEX_CHUNK=2: the crop of cqb3x -d's output, from a part of the file"""
    import subprocess
    w, h, b = 1000, 300, 3
    img = oracle.generate(w, h, b, 0, "NOISY3", 3)
    (tmp_path / "in.pnm").write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    bindir = os.path.dirname(qb3.LIB_PATH)
    env = dict(os.environ, QB3X_INDEX_CHUNK="2")
    r = subprocess.run([os.path.join(bindir, "cqb3x"), str(tmp_path / "in.pnm"), str(tmp_path / "a.qb3")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(bindir, "cqb3x"), "-d", str(tmp_path / "a.qb3"), str(tmp_path / "back.pnm")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    back = (tmp_path / "back.pnm").read_bytes()
    hdr = b"P6\n%d %d\n255\n" % (w, h)
    assert back.startswith(hdr)
    full = np.frombuffer(back[len(hdr):], np.uint8).reshape(h, w, b)
    x0, y0, ww, wh = 301, 77, 200, 120
    r = subprocess.run([os.path.join(bindir, "qb3window"), "-v", "-g", "256", str(tmp_path / "a.qb3"), "%d,%d,%d,%d" % (x0, y0, ww, wh), str(tmp_path / "win.pnm")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "win.pnm").read_bytes()
    whdr = b"P6\n%d %d\n255\n" % (ww, wh)
    assert got.startswith(whdr)
    assert np.array_equal(np.frombuffer(got[len(whdr):], np.uint8).reshape(wh, ww, b), full[y0:y0 + wh, x0:x0 + ww])
    assert "on path 1" in r.stdout
    nbytes = int(r.stdout.split(": ")[-1].split(" bytes")[0])
    assert 0 < nbytes < os.path.getsize(tmp_path / "a.qb3")
