"""Ranged window reads of 16-bit rasters (include/qb3x.h: QB3X_WINK_U16 on a handle of qb3x_open_ranged), the part that needs no
device: with the bit qb3x_ranged_table_ranges plans the chunks of the range rule with the raster's own blocks per segment (64, 32
for eight bands, 21 for six) and entry size; without it, and for every raster the 16-bit window kernels do not take, it plans what
it planned before.  The containers are the oracle's; a level-2 table is spliced into them as bytes (as test_ranged_plan.py does
for 8-bit rasters) with made-up, increasing positions and sealed checks: nothing decodes from it in this file."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_ranged as R  # noqa: E402
import qb3_window16 as W16  # noqa: E402
from qb3_window_dev import chunk_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTL, BASE = 8, 4
BIT = W16.QB3X_WINK_U16
U16, I16 = W16.U16, W16.I16
# (bands, width, height): the first shape of qb3_window16.py for the band count, the one with a shifted last column and row, and a
# table of three chunks (1016 entries of 190 bytes) so that single windows read the last chunk only, two chunks, and all
CASES = ((1, 260, 37), (4, 260, 37), (6, 132, 37), (8, 132, 37), (1, 1001, 259), (4, 1001, 259), (6, 1001, 259), (8, 1001, 259), (8, 1000, 520))


def with_table(c, E, blocks, W_, H_, version=3, flags=2):
    """the container with a level-2 table in front of "DT": an entry of E bytes per `blocks` blocks, chunks of at most 65535 bytes
    with a pad behind each, positions that grow by 1000 bits, checks sealed"""
    c = np.asarray(c, np.uint8)
    K = (((W_ + 3) // 4) * ((H_ + 3) // 4) + blocks - 1) // blocks
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
        run += b"ix" + bytes([ln & 255, ln >> 8, version, flags, chk & 255, chk >> 8]) + blocks.to_bytes(4, "little") + body + b"zz\x04\x00"
    return np.concatenate([c[:at], np.frombuffer(bytes(run), np.uint8), c[at:]])


def table_ranges(qb3, p, rects):
    wins = qb3.window_array(rects, [0] * len(rects))
    n = qb3.lib.qb3x_ranged_table_ranges(p, wins, len(rects), None, 0)
    out = (qb3.Range * max(n, 1))()
    assert qb3.lib.qb3x_ranged_table_ranges(p, wins, len(rects), out, n) == n
    return [(int(out[i].offset), int(out[i].size)) for i in range(n)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d" % (c[1], c[2], c[0]))
def test_table_ranges_follow_the_rule_with_the_rasters_segment_size(qb3, oracle, case):
    """without the bit: nothing is planned (a 16-bit raster is read whole); with it: the chunk ranges of the rule restated in
    qb3_ranged.py, for single rectangles and for batches that share chunks; a bad rectangle plans nothing; no read at all"""
    L = qb3.lib
    bands, Wd, Ht = case
    dt = I16 if case == (4, 260, 37) else U16
    E, B = R.entry_bytes("u16", bands), R.blocks_per_segment("u16", bands)
    c = with_table(oracle.encode(oracle.generate(Wd, Ht, bands, dt, "LANDSAT16", 2), dt, FTL if bands != 6 else BASE), E, B, Wd, Ht)
    tab = R.Table(c).shape(E)
    src = R.Source(qb3, c)
    p, dims = src.open(qb3)
    assert p and dims == (Wd, Ht, bands) and L.qb3x_decoder_table_entries(p) == tab.K
    del src.log[:]
    rects = W16.windows(Wd, Ht, 3 * Wd + bands, B)
    assert table_ranges(qb3, p, rects[:1]) == [] and table_ranges(qb3, p, rects) == []         # the default mask: today's answer
    L.qb3x_set_decoder_window_kernels(p, BIT)
    seen = set()
    for r in rects:
        want = [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, [r], tab.K, tab.N, B)]
        assert want and table_ranges(qb3, p, [r]) == want, r
        seen.add(len(want))
    if case == (8, 1000, 520):
        assert tab.K == 1016 and len(tab.chunks) == 3 and seen == {1, 2, 3}
        assert tab.chunk_range(2)[0] + tab.chunk_range(2)[1] == tab.D
    for batch in (rects, rects[1:5], rects[5:], rects[::3]):
        assert table_ranges(qb3, p, batch) == [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, batch, tab.K, tab.N, B)]
    wins = qb3.window_array(rects, [0] * len(rects))
    one = (qb3.Range * 1)()
    assert L.qb3x_ranged_table_ranges(p, wins, len(rects), one, 1) == len(R.plan_chunks(Wd, Ht, rects, tab.K, tab.N, B))
    assert (int(one[0].offset), int(one[0].size)) == tab.chunk_range(0)
    assert table_ranges(qb3, p, [(0, 0, Wd + 1, 1)]) == [] and table_ranges(qb3, p, [(0, 0, 0, 1)]) == []
    assert table_ranges(qb3, p, [rects[0], (0, 0, Wd + 1, 1)]) == []
    L.qb3x_set_decoder_window_kernels(p, 0)
    assert table_ranges(qb3, p, rects) == []                                                    # ... and back
    assert src.log == [] and not src.outside                                                    # pure planning
    L.qb3_destroy_decoder(p)


def test_the_bit_changes_nothing_for_rasters_the_kernels_do_not_take(qb3, oracle):
    """an 8-bit RGB container with a table plans the same ranges with and without the bit; uint16 x 5 (a lane per unit: 12 blocks
    a segment, fields of twelve bits) and a container without a table plan nothing either way"""
    L = qb3.lib
    Wd, Ht = 1001, 259
    rects = W16.windows(Wd, Ht, 11, 64)

    def both(c, K):
        src = R.Source(qb3, c)
        p, _ = src.open(qb3)
        assert p and L.qb3x_decoder_table_entries(p) == K
        del src.log[:]
        got = []
        for mask in (0, BIT):
            L.qb3x_set_decoder_window_kernels(p, mask)
            got.append(([table_ranges(qb3, p, [r]) for r in rects], table_ranges(qb3, p, rects)))
        assert src.log == []
        L.qb3_destroy_decoder(p)
        assert got[0] == got[1]
        return got[0]

    E8 = 6 + 2 * 3 + 80
    c = with_table(oracle.encode(oracle.generate(Wd, Ht, 3, 0, "NOISY3", 2), 0, FTL), E8, 64, Wd, Ht)
    tab = R.Table(c).shape(R.entry_bytes("u8", 3))
    singles, batch = both(c, tab.K)
    assert batch == [tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, rects, tab.K, tab.N)]
    assert singles == [[tab.chunk_range(k) for k in R.plan_chunks(Wd, Ht, [r], tab.K, tab.N)] for r in rects]
    E5 = 6 + 3 * 5 + (12 * 5 * 12 + 7) // 8
    c = with_table(oracle.encode(oracle.generate(Wd, Ht, 5, U16, "LANDSAT16", 2), U16, FTL), E5, 12, Wd, Ht)
    singles, batch = both(c, R.Table(c).shape(E5).K)
    assert batch == [] and all(s == [] for s in singles)
    singles, batch = both(oracle.encode(oracle.generate(Wd, Ht, 4, U16, "LANDSAT16", 2), U16, FTL), 0)
    assert batch == [] and all(s == [] for s in singles)


def test_python_switch_and_profile_name(qb3):
    from qb3_amd import device as qdev
    assert callable(qb3.RangedReader.set_window_kernels) and qdev.RangedDecoder.set_window_kernels is qb3.RangedReader.set_window_kernels
    assert inspect.signature(qb3.open_ranged).parameters["window_kernels"].default == 0
    assert inspect.signature(qb3.RangedReader.__init__).parameters["window_kernels"].default == 0
    text = open(os.path.join(ROOT, "include", "qb3x.h")).read()
    assert "dec_window16_ranged" in text and "the ranged calls do not look at it" not in " ".join(text.replace("\n * ", " ").split())
