"""Helpers of the ranged-window tests (test_ranged_plan.py, test_ranged_windows.py): a container in a numpy buffer behind a reader that
logs its calls, and the range rule of include/qb3x.h restated in Python -- which table chunks and which pieces of the stream a batch
of windows reads."""
import ctypes as C

import numpy as np

IX_HEAD, IX_PAD = 12, 4
QB3E_ERR = 3


class Source:
    """qb3x_read_fn over a host array: every call is logged as (offset, size); fail_after: calls that succeed before one fails"""

    def __init__(self, qb3, buf, fail_after=None):
        self.buf = np.ascontiguousarray(buf, np.uint8)
        self.log, self.fail_after, self.outside = [], fail_after, False
        self.fn = qb3.READ_FN(self._rd)

    def _rd(self, _ctx, off, dst, n):
        if self.fail_after is not None and len(self.log) >= self.fail_after:
            return 1
        self.log.append((off, n))
        if off + n > self.buf.size or n == 0:
            self.outside = True
            return 1
        C.memmove(dst, self.buf.ctypes.data + off, n)
        return 0

    def open(self, qb3, size=None):
        """(handle or None, (w, h, bands)); the log keeps what the open read"""
        dims = (C.c_size_t * 3)()
        p = qb3.lib.qb3x_open_ranged(self.fn, None, self.buf.size if size is None else size, dims)
        return p, tuple(dims)

    def bytes_logged(self):
        return sum(n for _, n in self.log)


def chunk_check(entries):
    """the 16-bit check of a version 3 table chunk: sum of (byte + 1) * (i * K + 1) mod 2^32, folded (include/qb3x.h)"""
    e = np.frombuffer(bytes(entries), np.uint8).astype(np.uint64)
    i = np.arange(len(e), dtype=np.uint64)
    s = int((((e + 1) * ((i * 0x9e3779b1 + 1) & 0xffffffff)) & 0xffffffff).sum()) & 0xffffffff
    return (s ^ (s >> 16)) & 0xffff


def seal(c, at):
    """recompute the check of the table chunk at offset `at` of the (writable) container c"""
    ln = int(c[at + 2]) | int(c[at + 3]) << 8
    chk = chunk_check(c[at + IX_HEAD:at + ln])
    c[at + 6], c[at + 7] = chk & 0xff, chk >> 8


class Table:
    """the restart table of a container, as the parser finds it: T the offset of the first "ix" chunk, chunks [(offset, length)],
    N entries per chunk, K entries, E bytes an entry, D the offset of the first stream byte ("DT" + 2)"""

    def __init__(self, c):
        c = np.asarray(c, np.uint8)
        pos, self.chunks = 11, []
        while True:
            sig, ln = bytes(c[pos:pos + 2]), int(c[pos + 2]) | int(c[pos + 3]) << 8
            if sig == b"DT":
                break
            if sig == b"ix":
                self.chunks.append((pos, ln))
            pos += ln if sig in (b"ix", b"zz") else 4 + ln
        self.dt, self.D, self.size = pos, pos + 2, len(c)
        self.T = self.chunks[0][0] if self.chunks else 0
        self.c = c

    def shape(self, bands):
        self.E = 6 + 2 * bands + 80
        self.N = (self.chunks[0][1] - IX_HEAD) // self.E
        self.K = sum((ln - IX_HEAD) // self.E for _, ln in self.chunks)
        return self

    def chunk_range(self, k):
        """(offset, size) of chunk k as it is read: head, entries, pad, and the mark behind the last"""
        nch = (self.K + self.N - 1) // self.N
        here = self.N if k + 1 < nch else self.K - k * self.N
        return self.T + k * (IX_HEAD + IX_PAD + self.N * self.E), IX_HEAD + here * self.E + IX_PAD + (2 if k + 1 == nch else 0)

    def entry_offset(self, s):
        k = s // self.N
        return self.T + k * (IX_HEAD + IX_PAD + self.N * self.E) + IX_HEAD + (s - k * self.N) * self.E

    def pos(self, s):
        """P(s): the bit position of entry s; P(K): the stream's length in bits"""
        if s >= self.K:
            return 8 * (self.size - self.D)
        at = self.entry_offset(s)
        return int.from_bytes(bytes(self.c[at:at + 6]), "little")


def block_rect(W, H, r):
    nbx, nby = (W + 3) // 4, (H + 3) // 4
    x0, y0, w, h = r
    return min(x0 // 4, nbx - 1), min((x0 + w - 1) // 4, nbx - 1), min(y0 // 4, nby - 1), min((y0 + h - 1) // 4, nby - 1), nbx


def plan_chunks(W, H, rects, K, N):
    """table chunks a batch reads: S0 / N .. min(S1 + 1, K - 1) / N of every window, and the last chunk; sorted, each once"""
    out = {(K - 1) // N}
    for r in rects:
        bx0, bx1, by0, by1, nbx = block_rect(W, H, r)
        s0, s1 = (by0 * nbx + bx0) // 64, min((by1 * nbx + bx1) // 64 + 1, K - 1)
        out.update(range(s0 // N, s1 // N + 1))
    return sorted(out)


def plan_pieces(W, H, rects, tab, gap=0):
    """byte ranges [(a, b)] of the stream a batch reads: a run of segments per block row of a window, its bytes widened to multiples of
    4 and clipped to the container, all of them sorted and merged where they overlap, touch or lie at most `gap` apart"""
    spans = set()
    for r in rects:
        bx0, bx1, by0, by1, nbx = block_rect(W, H, r)
        for by in range(by0, by1 + 1):
            s0, s1 = (by * nbx + bx0) // 64, (by * nbx + bx1) // 64
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
