"""Helpers of the 16-bit ranged-window tests (test_ranged16_plan.py, test_ranged16_windows.py): the range rule of include/qb3x.h
restated as qb3_ranged.py restates it, with the entry size E and the blocks per segment B as parameters -- 16-bit rasters have
entries of 6 + 3 * bands + 160 bytes (89 for one band) and segments of 64 / band groups blocks (64 for 1..4 bands, 32 for eight,
21 for six).  Source, chunk_check, seal and block_rect are qb3_ranged.py's."""
import qb3_ranged as R
from qb3_ranged import IX_HEAD, IX_PAD, Source, block_rect, chunk_check, seal  # noqa: F401


def entry_bytes(bands):
    """an entry of a 16-bit raster's level-2 table: position, a rung byte and an entering value per band, the lane fields"""
    return 6 + 3 * bands + (80 if bands == 1 else 160)


def blocks_per_segment(bands):
    """64 / band groups: a lane decodes up to four bands of a block"""
    return {1: 64, 2: 64, 3: 64, 4: 64, 6: 21, 8: 32}[bands]


class Table(R.Table):
    """qb3_ranged.Table with the entry size given, not derived from an 8-bit raster's bands"""

    def shape(self, E):
        self.E = E
        self.N = (self.chunks[0][1] - IX_HEAD) // E
        self.K = sum((ln - IX_HEAD) // E for _, ln in self.chunks)
        assert all((ln - IX_HEAD) % E == 0 for _, ln in self.chunks)
        return self


def plan_chunks(W, H, rects, K, N, B):
    """table chunks a batch reads: S0 / N .. min(S1 + 1, K - 1) / N of every window, and the last chunk; sorted, each once"""
    out = {(K - 1) // N}
    for r in rects:
        bx0, bx1, by0, by1, nbx = block_rect(W, H, r)
        s0, s1 = (by0 * nbx + bx0) // B, min((by1 * nbx + bx1) // B + 1, K - 1)
        out.update(range(s0 // N, s1 // N + 1))
    return sorted(out)


def plan_pieces(W, H, rects, tab, B, gap=0):
    """byte ranges [(a, b)] of the stream a batch reads: a run of segments per block row of a window, its bytes widened to multiples of
    4 and clipped to the container, all of them sorted and merged where they overlap, touch or lie at most `gap` apart"""
    spans = set()
    for r in rects:
        bx0, bx1, by0, by1, nbx = block_rect(W, H, r)
        for by in range(by0, by1 + 1):
            s0, s1 = (by * nbx + bx0) // B, (by * nbx + bx1) // B
            a, b = tab.D + tab.pos(s0) // 8, tab.D + (tab.pos(s1 + 1) + 7) // 8
            a, b = min(a // 4 * 4, tab.size), min((b + 3) // 4 * 4, tab.size)
            if b > a:
                spans.add((a, b))
    out = []
    for a, b in sorted(spans):
        if out and a <= out[-1][1] + gap:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def plan_bytes(W, H, rects, tab, B, gap=0, cached=()):
    """(bytes, reads) a ranged call asks of the reader on the shortcut: the chunks that are not cached, then the pieces"""
    chunks = [k for k in plan_chunks(W, H, rects, tab.K, tab.N, B) if k not in cached]
    pieces = plan_pieces(W, H, rects, tab, B, gap)
    return sum(tab.chunk_range(k)[1] for k in chunks) + sum(b - a for a, b in pieces), len(chunks) + len(pieces)
