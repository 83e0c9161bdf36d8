"""The device plumbing of the window tests, once, for every family (8-bit, 16-bit, 8-bit common-factor, lane-per-unit, band-selected,
ranged): containers written by this library, the whole decode of a second handle, and sentinel-guarded destinations -- one call into one
buffer (window_call) and a batch packed into one buffer (Layout, batch_call, single_calls).  The invariants live in check_destination: a
window is the crop of the whole decode, and no byte outside the window's rows is written.  A family differs in where destination k is
placed (destination, Layout's `rule`), not in what is checked.  torch and qb3_amd are imported inside the functions, so that the CPU
plan tests can take constants from here without a built library."""
import ctypes as C

import numpy as np

import qb3_window as W

SENTINEL = 0xc3
FTL, BASE, BASE_Z, CF_H, RLE = 8, 4, 0, 5, 2
ZCURVE = 0x0145236789cdabef
U8, I8, U16, I16, U32, I32, U64, I64 = range(8)
TSZ = (1, 1, 2, 2, 4, 4, 8, 8)
QB3X_WINK_U16, QB3X_WINK_CF8, QB3X_WINK_UNIT = 1, 2, 4
_vp = C.c_void_p


# ---------------------------------------------------------------------------------------------------------------- containers
def make_container(qb3, img, dt, mode, level=2, cband=None, quanta=1, want_index=False, zorder=False):
    """a container in device memory, written by this library from a device raster (h, w, bands) with qb3x_set_encoder_index_chunk
    (p, level); returns (uint8 tensor with zeros behind the container, size, out-of-band index or None)"""
    import torch
    from qb3_amd import device as qdev
    h, w, b = img.shape
    enc = qdev.DeviceEncoder(w, h, b, dt, mode=mode, cband=cband, want_index=want_index, index_chunk=level)
    if zorder:
        qb3.lib.qb3_set_encoder_mode(enc.p, 0)          # the Z order sticks to the handle (reference QB3encode.cpp:124-132)
    if quanta > 1:
        assert qb3.lib.qb3_set_encoder_quanta(enc.p, quanta, False)
    dst, n, index = enc.encode(img.reshape(-1))
    out = torch.zeros((n + 3) // 4 * 4 + 64, dtype=torch.uint8, device=img.device)
    out[:n] = dst[:n]
    index = index.clone() if index is not None else None
    enc.close()
    return out, n, index


def to_device(host, pad=64):
    import torch
    out = torch.zeros((len(host) + 3) // 4 * 4 + pad, dtype=torch.uint8, device="cuda")
    out[:len(host)] = torch.from_numpy(np.ascontiguousarray(host))
    return out


def as_rows(t, h):
    """a raster (device tensor of any type) as h rows of bytes"""
    import torch
    return t.contiguous().view(torch.uint8).reshape(h, -1)


def full_decode(qb3, d_c, n):
    """qb3x_decode_device on a handle of its own: (flat uint8 tensor or None when the call fails, status)"""
    import torch
    from qb3_amd import device as qdev
    dec = qdev.DeviceDecoder(d_c, n)
    out = torch.zeros(dec.out_bytes, dtype=torch.uint8, device=d_c.device)
    got = qb3.lib.qb3x_decode_device(dec.p, _vp(d_c.data_ptr()), _vp(out.data_ptr()), None, _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    st = qb3.lib.qb3x_last_decode_status(dec.p)
    dec.close()
    return (out if got else None), st


def segment_size(qb3, dec):
    bps = C.c_size_t()
    qb3.lib.qb3x_window_segments(dec.p, 0, 0, dec.w, dec.h, C.byref(bps))
    return bps.value


def segments_of(Wd, Ht, win, bps=64):
    """the index segments that hold a block of the window (W.brute_segments' enumeration, as a set)"""
    x0, y0, w, h = win
    nbx, nby = W.blocks_of(Wd, Ht)
    bx0, bx1 = min(x0 // 4, nbx - 1), min((x0 + w - 1) // 4, nbx - 1)
    by0, by1 = min(y0 // 4, nby - 1), min((y0 + h - 1) // 4, nby - 1)
    return {(by * nbx + bx) // bps for by in range(by0, by1 + 1) for bx in range(bx0, bx1 + 1)}


def count(qb3, name):
    """launches of a kernel in the library's profile"""
    ms, cnt = C.c_double(), C.c_uint64()
    return cnt.value if qb3.lib.qb3x_profile_get(name.encode(), C.byref(ms), C.byref(cnt)) else 0


def paths(qb3, p, n):
    return [qb3.lib.qb3x_window_path(p, i) for i in range(n)]


def table_chunks(c):
    """[(offset of an "ix" chunk, its length)] and the offset of the first stream byte"""
    c = bytes(c)
    pos, out = 11, []
    while True:
        sig, ln = c[pos:pos + 2], c[pos + 2] | c[pos + 3] << 8
        if sig == b"DT":
            return out, pos + 2
        if sig == b"ix":
            out.append((pos, ln))
        pos += ln if sig in (b"ix", b"zz") else 4 + ln


def chunk_check(entries):
    """the 16-bit check of a version 3 table chunk over its entry bytes: sum of (byte + 1) * (i * K + 1) mod 2^32, folded
    (include/qb3x.h)"""
    e = np.frombuffer(bytes(entries), np.uint8).astype(np.uint64)
    i = np.arange(len(e), dtype=np.uint64)
    s = int((((e + 1) * ((i * 0x9e3779b1 + 1) & 0xffffffff)) & 0xffffffff).sum()) & 0xffffffff
    return (s ^ (s >> 16)) & 0xffff


# ---------------------------------------------------------------------------------------------------------------- one destination
def check_destination(buf, off, sbytes, rect, pix, want_rows, what, last=True):
    """the window `rect` written at byte `off` of the sentinel-filled uint8 tensor buf, rows sbytes apart: its payload is the crop of
    want_rows (the raster as rows of bytes; None: not compared), and -- unless further destinations of buf are still to be checked
    (last False) -- buf holds the sentinel everywhere else.  The payload is overwritten with the sentinel on the way"""
    import torch
    x0, y0, w, h = rect
    wline = w * pix
    rows = buf[off:off + h * sbytes].view(h, sbytes)
    if want_rows is not None:
        want = want_rows[y0:y0 + h, x0 * pix:(x0 + w) * pix]
        if not torch.equal(rows[:, :wline], want):
            bad = (rows[:, :wline] != want).nonzero()
            raise AssertionError("%s: %d bytes differ, the first at row %d byte %d" % (what, len(bad), int(bad[0][0]), int(bad[0][1])))
    rows[:, :wline] = SENTINEL
    if last:
        assert bool((buf == SENTINEL).all()), "%s: bytes outside the windows' rows were written" % what


def row_extra(k):
    """values a destination's rows are wider than the window's: none, an even number, an odd number"""
    return (0, 2 * (1 + k % 5), 1 + 2 * (k % 4))[k % 3]


def destination(rule, k, tsz, addr=None):
    """k chooses the destination of a single call: (its byte offset behind 16 sentinel bytes, the values its rows are wider than the
    window's).  u16: every halfword of four dwords; rows tight, an even number of values wider, an odd number.  cf8: every value of a
    dword; rows tight, a few values wider so that rows fall on every byte of a dword, whole dwords wider.  unit: every value of eight
    (or the byte offset handed in); rows as u16's"""
    if rule == "u16":
        return 16 + 2 * (k % 8), row_extra(k)
    if rule == "cf8":
        return 16 + tsz * (k % 4), (0, 1 + k % 7, 4 * (1 + k % 3))[k % 3]
    assert rule == "unit", rule
    return (16 + tsz * (k % 8) if addr is None else addr), row_extra(k)


def window_call(qb3, dec, d_c, win, want_rows, pix, tsz, addr, extra, index=None):
    """one qb3x_decode_window_device into a sentinel-filled buffer at byte offset `addr`, rows `extra` values apart beyond the
    window's own; returns the byte count after checking payload and sentinels.  want_rows: the raster as rows of bytes, or None
    when the call is expected to fail (a shortcut may have written the window before the whole decode failed)"""
    import torch
    x0, y0, w, h = win
    wline = w * pix
    sbytes = wline + extra * tsz
    buf = torch.full((addr + (h + 1) * sbytes + 64,), SENTINEL, dtype=torch.uint8, device=d_c.device)
    assert buf.data_ptr() % 16 == 0
    n = qb3.lib.qb3x_decode_window_device(dec.p, _vp(d_c.data_ptr()), _vp(index.data_ptr()) if index is not None else None, x0, y0, w, h,
                                          _vp(buf.data_ptr() + addr), sbytes // tsz if extra else 0, _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert n == (0 if want_rows is None else h * wline), (win, n, qb3.last_error())
    check_destination(buf, addr, sbytes, win, pix, want_rows, "window %r (address +%d, stride +%d)" % (win, addr, extra))
    return n


# ---------------------------------------------------------------------------------------------------------------- batches
class Layout:
    """the destinations of a batch packed into ONE buffer, sentinel bytes in front, between and behind them.  `rule` places window k:
    u8    behind 8 bytes; at a dword, for 8-bit values + (k + start) % 4 -- every alignment; rows tight (even k + start) or
          1 + (k * 7) % 29 values wider (odd); 5 bytes behind a window
    u16   behind 16 bytes; at a dword + destination("u16")'s offset and rows; 6 bytes behind a window
    cf8   behind 16 bytes; at a dword + destination("cf8")'s offset and rows; 3 bytes behind a window
    unit  behind 16 bytes; at a multiple of 8 + destination("unit")'s offset and rows; 3 values behind a window
    mosaic (not u8) = (width in values, [(column in values, row)] per window, rows): the windows side by side in one image behind 16
    bytes, through the stride"""

    def __init__(self, rects, pix, tsz, rule, mosaic=None, start=0):
        assert tsz == {"u16": 2, "cf8": 1}.get(rule, tsz)
        self.rects, self.pix, self.tsz = rects, pix, tsz
        self.offs, self.sbytes = [], []
        if mosaic:
            assert rule != "u8"
            width, places, height = mosaic
            for (col, row) in places:
                self.offs.append(16 + tsz * (row * width + col))
                self.sbytes.append(tsz * width)
            self.size = 16 + tsz * width * height + 64
            return
        at, align, gap = {"u8": (8, 4, 5), "u16": (16, 4, 6), "cf8": (16, 4, 3), "unit": (16, 8, 3 * tsz)}[rule]
        for k, (x0, y0, w, h) in enumerate(rects):
            if rule == "u8":
                shift, extra = ((k + start) % 4 if tsz == 1 else 0), (0 if (k + start) % 2 == 0 else 1 + (k * 7) % 29)
            else:
                addr, extra = destination(rule, k, tsz)
                shift = addr - 16
            at = (at + align - 1) // align * align + shift
            sb = w * pix + tsz * extra
            self.offs.append(at)
            self.sbytes.append(sb)
            at += h * sb + gap
        self.size = at + 64

    def buffer(self):
        import torch
        return torch.full((self.size,), SENTINEL, dtype=torch.uint8, device="cuda")

    def strides(self):
        return [0 if sb == r[2] * self.pix else sb // self.tsz for sb, r in zip(self.sbytes, self.rects)]

    def array(self, qb3, buf):
        return qb3.window_array(self.rects, [buf.data_ptr() + o for o in self.offs], self.strides())

    def check(self, buf, want_rows, skip=()):
        """every window (but those in `skip`) equals the crop of want_rows, and nothing else in the buffer was written"""
        buf = buf.clone()
        for k, (r, off, sb) in enumerate(zip(self.rects, self.offs, self.sbytes)):
            check_destination(buf, off, sb, r, self.pix, None if k in skip else want_rows, "window %d %r" % (k, r), k + 1 == len(self.rects))


def batch_call(qb3, dec, d_c, lay, host=None, index=None, buf=None):
    """one qb3x_decode_windows_device (host: qb3x_read_windows on that host handle) into a fresh sentinel buffer, or into buf; returns
    (windows written, the buffer as a device tensor)"""
    import torch
    if host is not None:
        hbuf = np.full(lay.size + 16, SENTINEL, np.uint8)
        base = (-hbuf.ctypes.data) % 16                     # the layout's offsets count from a 16-byte address
        wins = qb3.window_array(lay.rects, [hbuf.ctypes.data + base + o for o in lay.offs], lay.strides())
        n = qb3.lib.qb3x_read_windows(host, wins, len(lay.rects))
        return n, torch.from_numpy(hbuf[base:base + lay.size]).cuda()
    buf = lay.buffer() if buf is None else buf
    n = qb3.lib.qb3x_decode_windows_device(dec.p, _vp(d_c.data_ptr()), _vp(index.data_ptr()) if index is not None else None,
                                           lay.array(qb3, buf), len(lay.rects), _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return n, buf


def single_calls(qb3, dec, d_c, lay):
    """the same windows through n single calls into a second buffer of the same layout"""
    import torch
    buf = lay.buffer()
    st = _vp(torch.cuda.current_stream().cuda_stream)
    for (x0, y0, w, h), off, stride in zip(lay.rects, lay.offs, lay.strides()):
        assert qb3.lib.qb3x_decode_window_device(dec.p, _vp(d_c.data_ptr()), None, x0, y0, w, h, _vp(buf.data_ptr() + off), stride, st) == h * w * lay.pix
    torch.cuda.synchronize()
    return buf
