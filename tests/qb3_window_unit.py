"""What the tests of the lane-per-unit window kernels share (test_window_unit_plan.py, test_window_unit_decode.py): the (type, bands)
matrix, the shapes and band maps of a band count, the rungs of a raster's units restated in numpy for any value width, and the device
plumbing of the GPU tests (containers, sentinel-guarded destinations, batches).  Windows and the seal are qb3_window16's, the geometry
rule is qb3_window's."""
import ctypes as C

import numpy as np

import qb3_window as W
import qb3_window16 as W16

QB3X_WINK_U16, QB3X_WINK_CF8, QB3X_WINK_UNIT = 1, 2, 4
HILBERT = W16.HILBERT
U8, I8, U16, I16, U32, I32, U64, I64 = range(8)
TSZ = (1, 1, 2, 2, 4, 4, 8, 8)
FTL, BASE, BASE_Z, CF_H = 8, 4, 0, 5
SENTINEL = 0xc3
_vp = C.c_void_p

# (type, bands) of the device tests: every value size, the smallest and the largest band count of each, odd and even ones, signed and unsigned
MATRIX = ((U8, 2), (U8, 5), (I8, 7), (U8, 16),
          (U16, 5), (I16, 7), (U16, 9),
          (U32, 1), (I32, 2), (U32, 3),
          (U64, 1), (I64, 2), (U64, 5), (U64, 16))
BIG = ((U8, 5), (I16, 7), (I32, 2), (U64, 1))          # these take (1001, 259) as their fourth shape
GENERATORS = ("NOISY3", "DEM", "RANDOM")
# (type, bands) of the plan tests and the blocks a segment of each holds: 64 // bands
PLAN_MATRIX = ((U8, 2, 32), (U8, 5, 12), (U8, 7, 9), (U8, 16, 4), (U16, 5, 12), (U16, 9, 7), (I32, 1, 64), (I32, 3, 21), (I64, 2, 32))


def seg_blocks(bands):
    return 64 // bands


def shapes_of(dt, bands):
    """the smallest shapes at which each mechanism can fail, with NB = 64 // bands blocks a segment"""
    NB = seg_blocks(bands)
    return ((4 * (NB + 1), 37),                         # nbx = NB + 1: a segment is reached from two block rows
            (8 * NB, 24),                               # nbx = 2 NB: nbx % NB == 0
            (4 * max(2, NB // 2) - 1, 50),              # several block rows in a segment, a partial last segment, a shifted last column
            (1001, 259) if (dt, bands) in BIG else (201, 67))      # shifted last column and row


def maps_of(bands):
    """None: the encoder's default (R-G, G, B-G for three bands and more; the identity below)"""
    if bands < 3:
        return (None,)
    return (None, list(range(bands))) + (([0, 0, 2, 2, 4],) if bands == 5 else ())


def unit_rungs(band, bits):
    """the rung of every unit of ONE band (a 2-D array, sides multiples of 4, values of `bits` bits in any integer type) coded in
    Hilbert order with the identity band map, FTL: the top bit of the largest mag-sign delta of the block's sixteen values, the first
    against the last value of the block before (the stream's first against 0) -- W16.unit_rungs for any value width, in arithmetic
    modulo 2^64 so that 64-bit values need no wider type"""
    h, w = band.shape
    assert h % 4 == 0 and w % 4 == 0
    nib = [(HILBERT >> (60 - 4 * i)) & 15 for i in range(16)]              # (y << 2) | x of the i-th value visited
    mask = np.uint64((1 << bits) - 1)
    v = band.astype(np.int64).view(np.uint64) & mask
    blocks = v.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16)[:, nib].reshape(-1)
    d = (blocks - np.concatenate((np.zeros(1, np.uint64), blocks[:-1]))) & mask      # the difference as a `bits`-bit two's complement number
    neg = (d >> np.uint64(bits - 1)) & np.uint64(1)
    m = (((d << np.uint64(1)) & mask) ^ (np.uint64(0) - neg)) & mask           # mag-sign: 2 d, or -2 d - 1 for a negative d
    m = m.reshape(-1, 16).max(axis=1)
    rung = np.zeros(m.shape, np.int64)
    for k in range(1, bits):
        rung[(m >> np.uint64(k)) > 0] = k
    return rung


# ---------------------------------------------------------------------------------------------------------------- device plumbing
def make_container(qb3, img, dt, mode, level=2, cband=None, quanta=1, want_index=False):
    """a container in device memory, written by this library from a device raster (h, w, bands) with qb3x_set_encoder_index_chunk
    (p, level); returns (uint8 tensor, size, out-of-band index or None)"""
    import torch
    from qb3_amd import device as qdev
    h, w, b = img.shape
    enc = qdev.DeviceEncoder(w, h, b, dt, mode=mode, cband=cband, want_index=want_index, index_chunk=level)
    if quanta > 1:
        assert qb3.lib.qb3_set_encoder_quanta(enc.p, quanta, False)
    dst, n, index = enc.encode(img.reshape(-1))
    out = torch.zeros((n + 3) // 4 * 4 + 64, dtype=torch.uint8, device=img.device)
    out[:n] = dst[:n]
    index = index.clone() if index is not None else None
    enc.close()
    return out, n, index


def as_rows(t, h):
    import torch
    return t.contiguous().view(torch.uint8).reshape(h, -1)


def full_decode(qb3, d_c, n):
    """qb3x_decode_device on a handle of its own: the flat uint8 tensor, or None when the call fails"""
    import torch
    from qb3_amd import device as qdev
    dec = qdev.DeviceDecoder(d_c, n)
    out = torch.zeros(dec.out_bytes, dtype=torch.uint8, device=d_c.device)
    got = qb3.lib.qb3x_decode_device(dec.p, _vp(d_c.data_ptr()), _vp(out.data_ptr()), None, _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    dec.close()
    return out if got else None


def segment_size(qb3, dec):
    bps = C.c_size_t()
    qb3.lib.qb3x_window_segments(dec.p, 0, 0, dec.w, dec.h, C.byref(bps))
    return bps.value


def row_extra(k):
    """values a destination's rows are wider than the window's: none, an even number, an odd number"""
    return (0, 2 * (1 + k % 5), 1 + 2 * (k % 4))[k % 3]


def window_call(qb3, dec, d_c, win, want_rows, pix, tsz, k, index=None, addr=None):
    """one qb3x_decode_window_device into a sentinel-filled buffer.  k chooses the destination: it starts k % 8 VALUES behind a dword
    (behind 16 sentinel bytes; addr: this byte offset instead) and its rows are tight, an even number of values wider or an odd
    number (row_extra).  Checks payload and sentinels; want_rows None: the call is expected to fail.  Returns the bytes written"""
    import torch
    x0, y0, w, h = win
    wline = w * pix
    extra = row_extra(k)
    sbytes = wline + tsz * extra
    addr = 16 + tsz * (k % 8) if addr is None else addr
    buf = torch.full((addr + (h + 1) * sbytes + 64,), SENTINEL, dtype=torch.uint8, device=d_c.device)
    assert buf.data_ptr() % 16 == 0
    n = qb3.lib.qb3x_decode_window_device(dec.p, _vp(d_c.data_ptr()), _vp(index.data_ptr()) if index is not None else None, x0, y0, w, h,
                                          _vp(buf.data_ptr() + addr), sbytes // tsz if extra else 0, _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    rows = buf[addr:addr + h * sbytes].view(h, sbytes)
    if want_rows is None:
        rows[:, :wline] = SENTINEL
        assert n == 0 and bool((buf == SENTINEL).all())
        return 0
    assert n == h * wline, (win, n, qb3.last_error())
    want = want_rows[y0:y0 + h, x0 * pix:(x0 + w) * pix]
    if not torch.equal(rows[:, :wline], want):
        bad = (rows[:, :wline] != want).nonzero()
        raise AssertionError("window %r (destination %d): %d bytes differ, the first at row %d byte %d" % (win, k, len(bad), int(bad[0][0]), int(bad[0][1])))
    rows[:, :wline] = SENTINEL
    assert bool((buf == SENTINEL).all()), "window %r (destination %d): bytes outside the window were written" % (win, k)
    return n


class Layout:
    """the destinations of a batch in one buffer: window k starts k % 8 values behind a dword, rows tight, wide-even or wide-odd"""

    def __init__(self, rects, pix, tsz, mosaic=None):
        self.rects, self.pix, self.tsz = rects, pix, tsz
        self.offs, self.sbytes = [], []
        if mosaic:                          # the windows side by side in rows of one image `mosaic[0]` values wide: (column, row) each
            for (col, row) in mosaic[1]:
                self.offs.append(16 + tsz * (row * mosaic[0] + col))
                self.sbytes.append(tsz * mosaic[0])
            self.size = 16 + tsz * mosaic[0] * mosaic[2] + 64
            return
        at = 16
        for k, (x0, y0, w, h) in enumerate(rects):
            at = (at + 7) // 8 * 8 + tsz * (k % 8)
            sb = w * pix + tsz * row_extra(k)
            self.offs.append(at)
            self.sbytes.append(sb)
            at += h * sb + 3 * tsz
        self.size = at + 64

    def strides(self):
        return [0 if sb == r[2] * self.pix else sb // self.tsz for sb, r in zip(self.sbytes, self.rects)]

    def check(self, buf, want_rows):
        import torch
        buf = buf.clone()
        for k, ((x0, y0, w, h), off, sb) in enumerate(zip(self.rects, self.offs, self.sbytes)):
            rows = buf[off:off + h * sb].view(h, sb)
            assert torch.equal(rows[:, :w * self.pix], want_rows[y0:y0 + h, x0 * self.pix:(x0 + w) * self.pix]), (k, self.rects[k])
            rows[:, :w * self.pix] = SENTINEL
        assert bool((buf == SENTINEL).all()), "bytes outside the windows were written"


def batch_call(qb3, dec, d_c, lay, host=None):
    """qb3x_decode_windows_device (host: qb3x_read_windows over the container's host copy) into a fresh sentinel buffer"""
    import torch
    if host is not None:
        hbuf = np.full(lay.size + 16, SENTINEL, np.uint8)
        base = (-hbuf.ctypes.data) % 16                     # the layout's offsets count from a 16-byte address
        wins = qb3.window_array(lay.rects, [hbuf.ctypes.data + base + o for o in lay.offs], lay.strides())
        n = qb3.lib.qb3x_read_windows(host, wins, len(lay.rects))
        return n, torch.from_numpy(hbuf[base:base + lay.size]).cuda()
    buf = torch.full((lay.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    wins = qb3.window_array(lay.rects, [buf.data_ptr() + o for o in lay.offs], lay.strides())
    n = qb3.lib.qb3x_decode_windows_device(dec.p, _vp(d_c.data_ptr()), None, wins, len(lay.rects), _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return n, buf


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


def entry_bytes(bands, tsz):
    """a level-2 entry of these rasters: position, a rung byte and the entering value per band, twelve bits a unit"""
    return 6 + bands * (1 + tsz) + (seg_blocks(bands) * bands * 12 + 7) // 8
