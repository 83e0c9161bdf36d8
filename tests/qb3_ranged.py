"""Helpers of the ranged-window tests of every family (test_ranged*_plan.py, test_ranged*_windows.py): a container in a numpy buffer
behind a reader that logs its calls; the range rule of include/qb3x.h restated in Python -- which table chunks and which pieces of the
stream a batch of windows reads -- with the entry size E and the blocks a segment B as parameters; and the plumbing of the GPU tests
(ranged calls into the sentinel-guarded destinations of qb3_window_dev.Layout)."""
import ctypes as C

import numpy as np

import qb3_window_best
import qb3_window_dev as D

IX_HEAD, IX_PAD = 12, 4
CHUNK_MAX = 65535   # a chunk's length field has 16 bits
HEAD_FLAGS = 3      # of every chunk of a cf8 table (bit 0: common-factor entries, bit 1: block fields)
QB3E_ERR = 3
_vp = C.c_void_p


def entry_bytes(rule, bands):
    """an entry of a level-2 table: position, then per band a rung byte and an entering value (cf8: and a factor), then the fields"""
    if rule == "u8":
        return 6 + 2 * bands + 80
    if rule == "u16":
        return 6 + 3 * bands + (80 if bands == 1 else 160)
    assert rule == "cf8", rule
    return qb3_window_best.entry_bytes(bands)             # 6 + 3 * bands + 192


def blocks_per_segment(rule, bands):
    """64; for 16-bit rasters 64 / band groups: a lane decodes up to four bands of a block"""
    return {1: 64, 2: 64, 3: 64, 4: 64, 6: 21, 8: 32}[bands] if rule == "u16" else 64


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


def seal(c, at):
    """recompute the check of the table chunk at offset `at` of the (writable) container c"""
    ln = int(c[at + 2]) | int(c[at + 3]) << 8
    chk = D.chunk_check(c[at + IX_HEAD:at + ln])
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

    def shape(self, E, flags=None):
        """E: the entry size; flags: what the low two bits of every chunk's head must say"""
        self.E = E
        self.N = (self.chunks[0][1] - IX_HEAD) // E
        self.K = sum((ln - IX_HEAD) // E for _, ln in self.chunks)
        assert all((ln - IX_HEAD) % E == 0 for _, ln in self.chunks)
        assert flags is None or all(int(self.c[at + 5]) & 3 == flags for at, _ in self.chunks)
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


def plan_chunks(W, H, rects, K, N, B=64):
    """table chunks a batch reads, B blocks a segment: S0 / N .. min(S1 + 1, K - 1) / N of every window, and the last chunk; sorted, each once"""
    out = {(K - 1) // N}
    for r in rects:
        bx0, bx1, by0, by1, nbx = block_rect(W, H, r)
        s0, s1 = (by0 * nbx + bx0) // B, min((by1 * nbx + bx1) // B + 1, K - 1)
        out.update(range(s0 // N, s1 // N + 1))
    return sorted(out)


def plan_pieces(W, H, rects, tab, gap=0, B=64):
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


def plan_bytes(W, H, rects, tab, gap=0, cached=(), B=64):
    """(bytes, reads) a ranged call asks of the reader on the shortcut: the chunks that are not cached, then the pieces"""
    chunks = [k for k in plan_chunks(W, H, rects, tab.K, tab.N, B) if k not in cached]
    pieces = plan_pieces(W, H, rects, tab, gap, B)
    return sum(tab.chunk_range(k)[1] for k in chunks) + sum(b - a for a, b in pieces), len(chunks) + len(pieces)


# ---------------------------------------------------------------------------------------------------------------- device plumbing
def host_container(qb3, img, dt, mode, level=2, cband=None, quanta=1):
    d_c, n, _ = D.make_container(qb3, img, dt, mode, level, cband, quanta)
    return d_c[:n].cpu().numpy()


def open_source(qb3, c, mask=0):
    """(Source, handle, (w, h, bands)) of a container behind a logging reader, the window kernels of `mask` switched on, the log empty"""
    src = Source(qb3, c)
    p, dims = src.open(qb3)
    assert p
    qb3.lib.qb3x_set_decoder_window_kernels(p, mask)
    del src.log[:]
    return src, p, dims


def host_call(qb3, p, lay, hbuf, sel=None):
    """qb3x_read_windows_ranged of the layout's windows (or of window `sel` alone) into the host buffer; returns the count"""
    ks = range(len(lay.rects)) if sel is None else [sel]
    strides = lay.strides()
    wins = qb3.window_array([lay.rects[k] for k in ks], [hbuf.ctypes.data + lay.offs[k] for k in ks], [strides[k] for k in ks])
    return qb3.lib.qb3x_read_windows_ranged(p, wins, len(ks))


def device_call(qb3, p, lay, buf):
    import torch
    n = qb3.lib.qb3x_decode_windows_ranged(p, lay.array(qb3, buf), len(lay.rects), _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return n


def check_host(lay, hbuf, rows, skip=()):
    import torch
    lay.check(torch.from_numpy(hbuf).cuda(), rows, skip)


def counters(qb3, p):
    return qb3.lib.qb3x_ranged_bytes(p), qb3.lib.qb3x_ranged_reads(p)


def check_fallback(qb3, c, rows, lay, want_paths, mask=0, host=True):
    """host (unless host is False) and device destinations: all windows written and exact, on the paths named, and the whole
    container read, once a call"""
    n = len(lay.rects)
    src, p, _ = open_source(qb3, c, mask)
    for dev in (False, True) if host else (True,):
        del src.log[:]
        if dev:
            buf = lay.buffer()
            assert device_call(qb3, p, lay, buf) == n, qb3.last_error()
            lay.check(buf, rows)
        else:
            hbuf = np.full(lay.size, D.SENTINEL, np.uint8)
            assert host_call(qb3, p, lay, hbuf) == n, qb3.last_error()
            check_host(lay, hbuf, rows)
        assert set(D.paths(qb3, p, n)) <= set(want_paths), D.paths(qb3, p, n)
        assert qb3.lib.qb3x_ranged_bytes(p) >= len(c)
        assert src.log.count((0, len(c))) == 1 and not src.outside
    qb3.lib.qb3_destroy_decoder(p)
