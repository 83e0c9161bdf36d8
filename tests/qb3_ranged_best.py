"""Helpers of the ranged-window tests for 8-bit common-factor rasters (test_ranged_best_plan.py, test_ranged_best_windows.py): the
range rule of include/qb3x.h restated as qb3_ranged.py restates it, for the entries these rasters have -- 6 position bytes, a rung, an
entering value and a factor per band, 64 fields of 3 bytes: E = 6 + 3 * bands + 192 -- and their chunks, whose head carries flags 3
(bit 0: common-factor entries, bit 1: block fields).  A segment has 64 blocks.  Source, chunk_check, seal and block_rect are
qb3_ranged.py's; entry_bytes and field_at are qb3_window_best.py's."""
import qb3_ranged as R
from qb3_ranged import IX_HEAD, IX_PAD, Source, block_rect, chunk_check, seal  # noqa: F401
from qb3_window_best import entry_bytes, field_at  # noqa: F401

B = 64              # blocks a segment
HEAD_FLAGS = 3      # of every chunk of such a table
CHUNK_MAX = 65535   # a chunk's length field has 16 bits


def per_chunk(bands):
    """entries of a full chunk: as many as its 16-bit length holds behind the head"""
    return (CHUNK_MAX - IX_HEAD) // entry_bytes(bands)


class Table(R.Table):
    """qb3_ranged.Table with the entry size of these rasters"""

    def shape(self, bands):
        self.E = entry_bytes(bands)
        self.N = (self.chunks[0][1] - IX_HEAD) // self.E
        self.K = sum((ln - IX_HEAD) // self.E for _, ln in self.chunks)
        assert all((ln - IX_HEAD) % self.E == 0 for _, ln in self.chunks)
        assert all(int(self.c[at + 5]) & 3 == HEAD_FLAGS for at, _ in self.chunks)
        return self


def plan_chunks(W, H, rects, K, N):
    """table chunks a batch reads: S0 / N .. min(S1 + 1, K - 1) / N of every window, and the last chunk; sorted, each once"""
    out = {(K - 1) // N}
    for r in rects:
        bx0, bx1, by0, by1, nbx = block_rect(W, H, r)
        s0, s1 = (by0 * nbx + bx0) // B, min((by1 * nbx + bx1) // B + 1, K - 1)
        out.update(range(s0 // N, s1 // N + 1))
    return sorted(out)


def plan_pieces(W, H, rects, tab, gap=0):
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


def plan_bytes(W, H, rects, tab, gap=0, cached=()):
    """(bytes, reads) a ranged call asks of the reader on the shortcut: the chunks that are not cached, then the pieces"""
    chunks = [k for k in plan_chunks(W, H, rects, tab.K, tab.N) if k not in cached]
    pieces = plan_pieces(W, H, rects, tab, gap)
    return sum(tab.chunk_range(k)[1] for k in chunks) + sum(b - a for a, b in pieces), len(chunks) + len(pieces)
