"""Ranged window reads (include/qb3x.h: qb3x_open_ranged, qb3x_read_windows_ranged, qb3x_ranged_table_ranges), the part that needs no
device: the symbols, the open that reads only the container's head, the table chunks a batch plans to read, STORED containers, the
refusals.  The containers are the oracle's; a level-2 table is spliced into them as bytes (as tests/test_reindex_host.py does) with
made-up, increasing positions and the chunks' checks computed here by the formula: nothing decodes from it in this file."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import qb3_ranged as R
import qb3_window as W
from qb3_window_dev import chunk_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTL, BASE, STORED = 8, 4, 255
NAMES = ("qb3x_open_ranged", "qb3x_read_windows_ranged", "qb3x_decode_windows_ranged", "qb3x_ranged_bytes", "qb3x_ranged_reads",
         "qb3x_set_ranged_gap", "qb3x_set_ranged_cache", "qb3x_ranged_table_ranges")
SHAPES = ((100, 100), (1000, 37), (1024, 260), (2051, 1030))


def with_table(c, bands, W_, H_):
    """the container with the level-2 table of an 8-bit raster in front of "DT": version 3, an entry per 64 blocks of 6 + 2 * bands
    + 80 bytes, chunks of at most 65535 bytes with a pad behind each, positions that grow by 1000 bits, checks sealed"""
    c = np.asarray(c, np.uint8)
    E = 6 + 2 * bands + 80
    K = (((W_ + 3) // 4) * ((H_ + 3) // 4) + 63) // 64
    N = (65535 - R.IX_HEAD) // E
    at = R.Table(c).dt
    run = bytearray()
    for k0 in range(0, K, N):
        here = min(N, K - k0)
        ln = R.IX_HEAD + here * E
        body = bytearray(here * E)
        for j in range(here):
            body[j * E:j * E + 6] = (1000 * (k0 + j)).to_bytes(6, "little")
            body[j * E + 6:j * E + E] = bytes((7 * (k0 + j) + i) & 0xff for i in range(E - 6))
        chk = chunk_check(body)
        run += b"ix" + bytes([ln & 255, ln >> 8, 3, 2, chk & 255, chk >> 8]) + (64).to_bytes(4, "little") + body + b"zz\x04\x00"
    return np.concatenate([c[:at], np.frombuffer(bytes(run), np.uint8), c[at:]])


def test_symbols_are_declared_exported_bound_and_harmless_with_null(qb3):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qb3x.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(qb3.lib, name) and name in qb3.EXPORTED
    assert "qb3x_read_fn" in text and "qb3x_range" in text
    assert "dec_window_ranged" in open(os.path.join(ROOT, "include", "qb3x.h")).read()
    L = qb3.lib
    dims = (C.c_size_t * 3)()
    assert not L.qb3x_open_ranged(None, None, 100, dims)
    src = R.Source(qb3, np.zeros(64, np.uint8))
    assert not L.qb3x_open_ranged(src.fn, None, 64, None)
    assert not L.qb3x_open_ranged(src.fn, None, 64, dims)               # (zeros are not a container)
    assert not L.qb3x_open_ranged(src.fn, None, 10, dims) and not src.outside
    win = qb3.window_array([(0, 0, 1, 1)], [src.buf.ctypes.data])
    assert L.qb3x_read_windows_ranged(None, win, 1) == 0 and L.qb3x_decode_windows_ranged(None, win, 1, None) == 0
    assert L.qb3x_ranged_bytes(None) == 0 and L.qb3x_ranged_reads(None) == 0
    L.qb3x_set_ranged_gap(None, 5)
    L.qb3x_set_ranged_cache(None, 5)
    assert L.qb3x_ranged_table_ranges(None, win, 1, None, 0) == 0


def test_a_handle_that_is_not_ranged_is_refused(qb3, oracle):
    L = qb3.lib
    s = oracle.encode(oracle.generate(64, 48, 3, 0, "NOISY3", 5), 0, FTL)
    p, _ = W.open_handle(L, s)
    out = np.full(64, 0x5c, np.uint8)
    win = qb3.window_array([(0, 0, 2, 2)], [out.ctypes.data])
    assert L.qb3x_read_windows_ranged(p, win, 1) == 0 and W.handle_error(p) == W.QB3E_EINV
    assert L.qb3x_ranged_table_ranges(p, win, 1, None, 0) == 0
    assert (out == 0x5c).all()
    L.qb3_destroy_decoder(p)


@pytest.mark.parametrize("bands", (1, 3))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_open_reads_the_head_and_nothing_else(qb3, oracle, shape, bands):
    """dims, mode and table entries are those of qb3_read_start + qb3_read_info over the whole buffer; no read touches an entry of the
    table or a byte behind "DT" + 4"""
    L = qb3.lib
    Wd, Ht = shape
    plain = oracle.encode(oracle.generate(Wd, Ht, bands, 0, "NOISY3", 2), 0, FTL if bands == 3 else BASE)
    for c in (plain, with_table(plain, bands, Wd, Ht)):
        ref, rdims = W.open_handle(L, c)
        src = R.Source(qb3, c)
        p, dims = src.open(qb3)
        assert p and dims == rdims == (Wd, Ht, bands)
        assert L.qb3_get_mode(p) == L.qb3_get_mode(ref) and L.qb3_get_type(p) == L.qb3_get_type(ref) and L.qb3_get_order(p) == L.qb3_get_order(ref)
        assert L.qb3x_decoder_table_entries(p) == L.qb3x_decoder_table_entries(ref)
        assert L.qb3_decoded_size(p) == L.qb3_decoded_size(ref)
        tab = R.Table(c)
        if c is not plain:
            assert L.qb3x_decoder_table_entries(p) == (((Wd + 3) // 4) * ((Ht + 3) // 4) + 63) // 64
            assert len(tab.chunks) == (3 if shape == (2051, 1030) else 1)
        assert src.log and not src.outside
        for off, n in src.log:
            assert off + n <= tab.dt + 4, (off, n)
            for at, ln in tab.chunks:
                assert off + n <= at + R.IX_HEAD or off >= at + ln, "a read inside the entries of the chunk at %d: %r" % (at, (off, n))
        assert src.bytes_logged() < 200
        assert L.qb3x_ranged_bytes(p) == 0 and L.qb3x_ranged_reads(p) == 0
        L.qb3_destroy_decoder(p)
        L.qb3_destroy_decoder(ref)


def test_open_fails_when_the_reader_fails(qb3, oracle):
    c = with_table(oracle.encode(oracle.generate(1024, 260, 3, 0, "NOISY3", 2), 0, FTL), 3, 1024, 260)
    full = R.Source(qb3, c)
    p, _ = full.open(qb3)
    assert p
    qb3.lib.qb3_destroy_decoder(p)
    for k in range(len(full.log)):
        src = R.Source(qb3, c, fail_after=k)
        p, _ = src.open(qb3)
        assert not p, k


def table_ranges(qb3, p, rects):
    wins = qb3.window_array(rects, [0] * len(rects))
    n = qb3.lib.qb3x_ranged_table_ranges(p, wins, len(rects), None, 0)
    out = (qb3.Range * max(n, 1))()
    assert qb3.lib.qb3x_ranged_table_ranges(p, wins, len(rects), out, n) == n
    return [(int(out[i].offset), int(out[i].size)) for i in range(n)]


@pytest.mark.parametrize("bands", (1, 3))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_table_ranges_follow_the_rule(qb3, oracle, shape, bands):
    """qb3x_ranged_table_ranges against the rule restated in qb3_ranged.py: single rectangles, and batches that share chunks"""
    L = qb3.lib
    Wd, Ht = shape
    c = with_table(oracle.encode(oracle.generate(Wd, Ht, bands, 0, "NOISY3", 2), 0, FTL), bands, Wd, Ht)
    tab = R.Table(c).shape(R.entry_bytes("u8", bands))
    src = R.Source(qb3, c)
    p, _ = src.open(qb3)
    assert p and L.qb3x_decoder_table_entries(p) == tab.K
    del src.log[:]
    rects = W.windows(Wd, Ht, 3 * Wd + bands, 24)
    seen = set()
    for r in rects:
        want = [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, [r], tab.K, tab.N)]
        assert table_ranges(qb3, p, [r]) == want, r
        seen.add(len(want))
    if shape == (2051, 1030):
        assert seen == {1, 2, 3}                         # the last chunk alone, with one more, all three
        assert tab.chunk_range(2)[0] + tab.chunk_range(2)[1] == tab.D
    for batch in (rects, rects[1:5], rects[5:], rects[::3]):
        assert table_ranges(qb3, p, batch) == [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, batch, tab.K, tab.N)]
    # a short output array gets the first ranges, the count is the whole list's; a bad rectangle plans nothing
    wins = qb3.window_array(rects, [0] * len(rects))
    one = (qb3.Range * 1)()
    assert L.qb3x_ranged_table_ranges(p, wins, len(rects), one, 1) == len(R.plan_chunks(Wd, Ht, rects, tab.K, tab.N))
    assert (int(one[0].offset), int(one[0].size)) == tab.chunk_range(0)
    assert table_ranges(qb3, p, [(0, 0, Wd + 1, 1)]) == [] and table_ranges(qb3, p, [(0, 0, 0, 1)]) == []
    assert src.log == []                                 # pure planning
    L.qb3_destroy_decoder(p)
    # a container without a table plans nothing
    plain = R.Source(qb3, oracle.encode(oracle.generate(Wd, Ht, bands, 0, "NOISY3", 2), 0, FTL))
    p, _ = plain.open(qb3)
    assert p and table_ranges(qb3, p, [(0, 0, 1, 1)]) == []
    L.qb3_destroy_decoder(p)


@pytest.mark.parametrize("case", ((64, 32, 3, 0), (200, 40, 1, 2), (4, 4, 3, 0)), ids=lambda c: "%dx%dx%d-t%d" % c)
def test_stored_windows_read_their_rows_only(qb3, oracle, case):
    """a STORED container: every window is the crop, and the reader was asked for the windows' rows and nothing else; no device"""
    L = qb3.lib
    Wd, Ht, b, dt = case
    img = oracle.generate(Wd, Ht, b, dt, "RANDOM", 9)
    c = oracle.encode(img, dt, FTL)
    assert c[10] == STORED
    tsz = img.itemsize
    pix = b * tsz
    raw = img.view(np.uint8).reshape(Ht, Wd * pix)
    src = R.Source(qb3, c)
    p, _ = src.open(qb3)
    assert p
    D = R.Table(c).D
    rects = W.windows(Wd, Ht, 4, 6)
    for batch in [[r] for r in rects] + [rects]:
        del src.log[:]
        outs, ptrs, strides = [], [], []
        for k, (x0, y0, w, h) in enumerate(batch):
            extra = 0 if k % 2 == 0 else 3
            outs.append(np.full((h, (w + extra) * pix), 0x5c, np.uint8))
            ptrs.append(outs[-1].ctypes.data)
            strides.append((w + extra) * b)
        wins = qb3.window_array(batch, ptrs, strides)
        assert L.qb3x_read_windows_ranged(p, wins, len(batch)) == len(batch), qb3.last_error()
        want_log = []
        for k, ((x0, y0, w, h), o) in enumerate(zip(batch, outs)):
            assert np.array_equal(o[:, :w * pix], raw[y0:y0 + h, x0 * pix:(x0 + w) * pix]), (x0, y0, w, h)
            assert (o[:, w * pix:] == 0x5c).all()
            assert L.qb3x_window_ok(p, k) == 1 and L.qb3x_window_path(p, k) == 3
            if w == Wd and strides[k] == Wd * b:
                want_log.append((D + y0 * Wd * pix, h * Wd * pix))
            else:
                want_log += [(D + (y0 + y) * Wd * pix + x0 * pix, w * pix) for y in range(h)]
        assert src.log == want_log
        assert L.qb3x_ranged_bytes(p) == sum(n for _, n in want_log) and L.qb3x_ranged_reads(p) == len(want_log)
        assert L.qb3x_last_window_path(p) == 3
    L.qb3_destroy_decoder(p)


def test_refusals_call_no_reader(qb3, oracle):
    """an empty rectangle, one outside the raster, n == 0, no array, no destination: QB3E_EINV before anything is read -- one bad
    rectangle refuses the batch; a reader that fails fails the call with QB3E_ERR"""
    L = qb3.lib
    Wd, Ht, b = 100, 100, 3
    coded = with_table(oracle.encode(oracle.generate(Wd, Ht, b, 0, "NOISY3", 2), 0, FTL), b, Wd, Ht)
    stored = oracle.encode(oracle.generate(Wd, Ht, b, 0, "RANDOM", 2), 0, FTL)
    assert stored[10] == STORED
    out = np.full(Wd * Ht * b, 0x5c, np.uint8)
    good = (3, 4, 20, 10)
    for c in (coded, stored):
        for rects, n in (([(0, 0, 0, 5)], 1), ([(0, 0, 5, 0)], 1), ([(Wd, 0, 1, 1)], 1), ([(Wd - 3, 0, 4, 1)], 1), ([(0, Ht - 1, 1, 2)], 1),
                         ([good, (0, 0, Wd + 1, 1)], 2), ([good], 0)):
            src = R.Source(qb3, c)
            p, _ = src.open(qb3)
            assert p
            del src.log[:]
            wins = qb3.window_array(rects, [out.ctypes.data] * len(rects))
            assert L.qb3x_read_windows_ranged(p, wins, n) == 0 and W.handle_error(p) == W.QB3E_EINV, (rects, n)
            assert L.qb3x_decode_windows_ranged(p, wins, n, None) == 0
            assert src.log == [] and L.qb3x_ranged_reads(p) == 0
            L.qb3_destroy_decoder(p)
        for wins in (None, qb3.window_array([good], [0])):            # no array; no destination
            src = R.Source(qb3, c)
            p, _ = src.open(qb3)
            del src.log[:]
            assert L.qb3x_read_windows_ranged(p, wins, 1) == 0 and W.handle_error(p) == W.QB3E_EINV and src.log == []
            L.qb3_destroy_decoder(p)
    assert (out == 0x5c).all()
    # the reader fails: STORED rows
    src = R.Source(qb3, stored)
    p, _ = src.open(qb3)
    src.fail_after = len(src.log) + 3
    wins = qb3.window_array([good], [out.ctypes.data])
    assert L.qb3x_read_windows_ranged(p, wins, 1) == 0 and W.handle_error(p) == R.QB3E_ERR
    assert L.qb3x_window_ok(p, 0) == 0
    L.qb3_destroy_decoder(p)
