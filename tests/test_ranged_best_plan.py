"""Ranged window reads of 8-bit common-factor rasters (include/qb3x.h: QB3X_WINK_CF8 on a handle of qb3x_open_ranged), the part that
needs no device: with the bit qb3x_ranged_table_ranges plans the chunks of the range rule for the rasters the common-factor window
kernels take (8-bit, 1 / 3 / 4 bands, QB3M_CF, QB3M_CF_H, QB3M_BEST where the RLE0 pass did not win); without it, with QB3X_WINK_U16
alone, and for every other raster it plans what it planned before.  The containers are the oracle's; a table is spliced into them as
bytes (as test_ranged16_plan.py does) with made-up, increasing positions and sealed checks: nothing decodes from it in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_ranged as R  # noqa: E402
import qb3_window16 as W16  # noqa: E402
import qb3_window_best as WB  # noqa: E402
from qb3_window_dev import chunk_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTL = 8
BIT, U16BIT = WB.QB3X_WINK_CF8, W16.QB3X_WINK_U16
# the four shapes of the window kernels' tests, and one whose table has three chunks for 3 and 4 bands (640 segments) and two for one
SHAPES = WB.SHAPES + ((1280, 512),)
RASTERS = ("FEW", "TERRACE", "NOISY3")     # test_window_best_plan.py: coded common-factor containers at every shape, band count, mode


def with_table(c, E, blocks, W_, H_, version=3, flags=R.HEAD_FLAGS):
    """the container with a table in front of "DT": an entry of E bytes per `blocks` blocks, chunks of at most 65535 bytes with a pad
    behind each, positions that grow by 1000 bits, checks sealed"""
    c = np.asarray(c, np.uint8)
    K = (((W_ + 3) // 4) * ((H_ + 3) // 4) + blocks - 1) // blocks
    N = (R.CHUNK_MAX - R.IX_HEAD) // E
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
        run += b"ix" + bytes([ln & 255, ln >> 8, version, flags, chk & 255, chk >> 8]) + blocks.to_bytes(4, "little") + body + b"zz\x04\x00"
    return np.concatenate([c[:at], np.frombuffer(bytes(run), np.uint8), c[at:]])


def table_ranges(qb3, p, rects):
    wins = qb3.window_array(rects, [0] * len(rects))
    n = qb3.lib.qb3x_ranged_table_ranges(p, wins, len(rects), None, 0)
    out = (qb3.Range * max(n, 1))()
    assert qb3.lib.qb3x_ranged_table_ranges(p, wins, len(rects), out, n) == n
    return [(int(out[i].offset), int(out[i].size)) for i in range(n)]


def windows_of(Wd, Ht, seed):
    """W16.windows, and for the large shape three windows chosen by segment: in the first chunk, across the first seam, in the last"""
    rects = W16.windows(Wd, Ht, seed, 64, 12)
    if (Wd, Ht) == (1280, 512):
        rects += [(0, 0, 64, 4), (0, 4 * 60, 1280, 12), (1200, 500, 80, 12)]
    return rects


@pytest.mark.parametrize("bands", WB.BANDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_table_ranges_follow_the_rule_with_the_bit(qb3, oracle, shape, bands):
    """QB3M_CF, QB3M_CF_H and QB3M_BEST containers (mode byte 1 or 5, asserted) with a table of head flags 3, version 3, 64 blocks
    and entries of 6 + 3 * bands + 192 bytes.  Without the bit, and with QB3X_WINK_U16 alone: nothing is planned (the file is read
    whole).  With QB3X_WINK_CF8: the chunk ranges of the rule restated in qb3_ranged.py, for single rectangles and for batches
    that share chunks; a bad rectangle plans nothing; the reader is never called"""
    L = qb3.lib
    Wd, Ht = shape
    E = R.entry_bytes("cf8", bands)
    assert E == 6 + 3 * bands + 192
    for turn, mode in enumerate(WB.MODES):
        name = RASTERS[(turn + bands + Wd) % 3]
        plain = oracle.encode(WB.raster(oracle.generate, name, Wd, Ht, bands, 7 * Wd + bands), 0, mode)
        assert int(plain[10]) == (1 if mode == WB.CF else 5), (name, mode)         # a coded common-factor container, or the case tests nothing
        c = with_table(plain, E, R.blocks_per_segment("cf8", bands), Wd, Ht)
        tab = R.Table(c).shape(E, R.HEAD_FLAGS)
        nseg = (((Wd + 3) // 4) * ((Ht + 3) // 4) + 63) // 64
        assert tab.K == nseg and tab.N == min((R.CHUNK_MAX - R.IX_HEAD) // E, nseg) and len(tab.chunks) == (nseg + tab.N - 1) // tab.N
        if shape == (1280, 512):        # the chunk count from E and IX_HEAD: 640 entries at 316 (3 bands), 312 (4) or 325 (1) a chunk
            assert nseg == 640 and len(tab.chunks) == -(-640 // ((65535 - R.IX_HEAD) // E)) == (2 if bands == 1 else 3)
        src = R.Source(qb3, c)
        p, dims = src.open(qb3)
        assert p and dims == (Wd, Ht, bands) and L.qb3x_decoder_table_entries(p) == tab.K
        del src.log[:]
        rects = windows_of(Wd, Ht, 3 * Wd + bands + mode)
        for mask in (0, U16BIT):                                                    # today's answer: nothing
            L.qb3x_set_decoder_window_kernels(p, mask)
            assert table_ranges(qb3, p, rects[:1]) == [] and table_ranges(qb3, p, rects) == [], mask
        for mask in (BIT, BIT | U16BIT):
            L.qb3x_set_decoder_window_kernels(p, mask)
            seen = set()
            for r in rects:
                want = [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, [r], tab.K, tab.N)]
                assert want and table_ranges(qb3, p, [r]) == want, (mode, r)
                seen.add(len(want))
            assert seen >= set(range(1, len(tab.chunks) + 1)) or len(tab.chunks) == 1
            for batch in (rects, rects[1:5], rects[5:], rects[::3]):
                assert table_ranges(qb3, p, batch) == [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, batch, tab.K, tab.N)]
        last = len(tab.chunks) - 1
        assert tab.chunk_range(last)[0] + tab.chunk_range(last)[1] == tab.D
        wins = qb3.window_array(rects, [0] * len(rects))
        one = (qb3.Range * 1)()
        assert L.qb3x_ranged_table_ranges(p, wins, len(rects), one, 1) == len(R.plan_chunks(Wd, Ht, rects, tab.K, tab.N))
        assert (int(one[0].offset), int(one[0].size)) == tab.chunk_range(0)
        assert table_ranges(qb3, p, [(0, 0, Wd + 1, 1)]) == [] and table_ranges(qb3, p, [(0, 0, 0, 1)]) == []
        assert table_ranges(qb3, p, [rects[0], (0, 0, Wd + 1, 1)]) == []
        L.qb3x_set_decoder_window_kernels(p, 0)
        assert table_ranges(qb3, p, rects) == []                                    # ... and back
        assert src.log == [] and not src.outside                                    # pure planning
        L.qb3_destroy_decoder(p)


def plans(qb3, c, rects, K):
    """([ranges of each rectangle], ranges of the batch) without the bit and with it, on one handle that never calls its reader"""
    L = qb3.lib
    src = R.Source(qb3, c)
    p, _ = src.open(qb3)
    assert p and L.qb3x_decoder_table_entries(p) == K
    del src.log[:]
    got = []
    for mask in (0, BIT):
        L.qb3x_set_decoder_window_kernels(p, mask)
        got.append(([table_ranges(qb3, p, [r]) for r in rects], table_ranges(qb3, p, rects)))
    assert src.log == [] and not src.outside
    L.qb3_destroy_decoder(p)
    return got


def test_the_bit_changes_nothing_for_an_ftl_container(qb3, oracle):
    """8-bit RGB in QB3M_FTL with a level-2 table: the ranges of qb3_ranged.py's rule, with and without the bit"""
    Wd, Ht = 1001, 259
    rects = W16.windows(Wd, Ht, 11, 64)
    c = with_table(oracle.encode(oracle.generate(Wd, Ht, 3, 0, "NOISY3", 2), 0, FTL), 6 + 2 * 3 + 80, 64, Wd, Ht, flags=2)
    tab = R.Table(c).shape(R.entry_bytes("u8", 3))
    without, with_bit = plans(qb3, c, rects, tab.K)
    assert without == with_bit
    assert with_bit[1] == [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, rects, tab.K, tab.N)]
    assert with_bit[0] == [[tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, [r], tab.K, tab.N)] for r in rects]


def segment_blocks(qb3, plain):
    L = qb3.lib
    src = R.Source(qb3, plain)
    p, dims = src.open(qb3)
    assert p
    bps = C.c_size_t()
    L.qb3x_window_segments(p, 0, 0, dims[0], dims[1], C.byref(bps))
    L.qb3_destroy_decoder(p)
    return bps.value


@pytest.mark.parametrize("case", ((2, 0), (5, 0), (4, W16.U16)), ids=("u8x2", "u8x5", "u16x4"))
def test_the_bit_plans_nothing_for_other_common_factor_rasters(qb3, oracle, case):
    """8-bit x 2 and x 5 and uint16 x 4 in QB3M_CF_H, each with the table this library's parser takes for it (head flags 3, the
    raster's own blocks per segment, a field per block or per unit -- whichever entry size the handle accepts, asserted through the
    entry count): nothing is planned, with the bit and without"""
    bands, dt = case
    Wd, Ht = 260, 37
    tsz = 2 if dt else 1
    plain = oracle.encode(oracle.generate(Wd, Ht, bands, dt, "LANDSAT16" if dt else "FEW", 2), dt, WB.CF_H)
    assert int(plain[10]) == 5
    bps = segment_blocks(qb3, plain)
    assert bps
    K = (65 * 10 + bps - 1) // bps
    rects = W16.windows(Wd, Ht, 11, bps, 8)
    accepted = 0
    for fields in (bps * bands, bps):
        c = with_table(plain, 6 + bands * (1 + 2 * tsz) + 3 * fields, bps, Wd, Ht)
        src = R.Source(qb3, c)
        p, _ = src.open(qb3)
        assert p
        entries = qb3.lib.qb3x_decoder_table_entries(p)
        qb3.lib.qb3_destroy_decoder(p)
        if entries != K:
            continue
        accepted += 1
        for singles, batch in plans(qb3, c, rects, K):
            assert batch == [] and all(s == [] for s in singles)
    assert accepted == 1


def test_the_bit_plans_nothing_without_a_usable_table(qb3, oracle):
    """an 8-bit RGB QB3M_CF_H container with no table, and one whose table says head flags 2 (entries without factors: not this
    raster's): nothing is planned either way"""
    Wd, Ht = 260, 37
    rects = W16.windows(Wd, Ht, 11, 64, 8)
    plain = oracle.encode(oracle.generate(Wd, Ht, 3, 0, "FEW", 2), 0, WB.CF_H)
    assert int(plain[10]) == 5
    for singles, batch in plans(qb3, plain, rects, 0):
        assert batch == [] and all(s == [] for s in singles)
    c = with_table(plain, 6 + 2 * 3 + 80, 64, Wd, Ht, flags=2)
    src = R.Source(qb3, c)
    p, _ = src.open(qb3)
    K = qb3.lib.qb3x_decoder_table_entries(p)
    qb3.lib.qb3_destroy_decoder(p)
    for singles, batch in plans(qb3, c, rects, K):
        assert batch == [] and all(s == [] for s in singles)
    # ... while the same container with the table of its own kind is planned (the control of the two cases above)
    c = with_table(plain, R.entry_bytes("cf8", 3), 64, Wd, Ht)
    tab = R.Table(c).shape(R.entry_bytes("cf8", 3), R.HEAD_FLAGS)
    without, with_bit = plans(qb3, c, rects, tab.K)
    assert without[1] == [] and with_bit[1] == [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, rects, tab.K, tab.N)]


def test_header_text(qb3):
    """the profile name of the new kernels is listed, and the sentence that said the bit adds no pieces is gone"""
    text = " ".join(open(os.path.join(ROOT, "include", "qb3x.h")).read().replace("\n * ", " ").split())
    names = text[text.index("Kernel names:"):]
    assert "dec_window_best_ranged (" in names[:names.index("*/")]
    assert "adds NO pieces" not in text and "QB3X_WINK_CF8 adds" not in text
