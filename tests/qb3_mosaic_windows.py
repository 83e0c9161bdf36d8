"""Helpers of the mosaic-window tests (test_mosaic_windows_plan.py, test_mosaic_windows.py): the tiles and pieces of a rectangle by
enumeration, a mosaic coded on the device, and one call of qb3x_decode_mosaic_windows into a 0xA5 buffer that is compared whole."""
import ctypes as C

import numpy as np

from qb3_amd import Window
from qb3_mosaic import grid

_sz = C.c_size_t
_vp = C.c_void_p
GAP = 64                        # bytes of 0xA5 between the windows of a call


def brute_tiles(W, H, tw, th, x0, y0, w, h):
    """the (i, j) of every tile of the grid that holds a pixel of the rectangle, pixel by pixel along its two axes"""
    if not (W and H and tw and th) or w <= 0 or h <= 0 or x0 + w > W or y0 + h > H:
        return set()
    return {(x // tw, y // th) for y in range(y0, y0 + h) for x in range(x0, x0 + w)} if w * h <= 4096 else \
        {(i, j) for i in {x // tw for x in range(x0, x0 + w)} for j in {y // th for y in range(y0, y0 + h)}}


def pieces(W, H, tw, th, x0, y0, w, h):
    """[(k, x, y, w, h)]: the parts of the rectangle by tile, each in its tile's pixels"""
    tx, _ = grid(W, H, tw, th)
    out = []
    for (i, j) in sorted(brute_tiles(W, H, tw, th, x0, y0, w, h), key=lambda t: (t[1], t[0])):
        ax, bx = max(x0, i * tw), min(x0 + w, (i + 1) * tw)
        ay, by = max(y0, j * th), min(y0 + h, (j + 1) * th)
        out.append((j * tx + i, ax - i * tw, ay - j * th, bx - ax, by - ay))
    return out


class Mosaic:
    """a raster coded by qb3x_encode_mosaic: the containers stay on the device (dst, pitch, sizes)"""

    def __init__(self, qb3, torch, raster, tw, th, dt, mode, index_chunk=2, quanta=1):
        L = qb3.lib
        self.qb3, self.torch, self.raster = qb3, torch, raster
        self.H, self.W, self.b = raster.shape
        self.tw, self.th, self.dt, self.tsz = tw, th, dt, raster.itemsize
        self.tx, self.ty = grid(self.W, self.H, tw, th)
        self.n = self.tx * self.ty
        p = L.qb3_create_encoder(tw, th, self.b, dt)
        assert p
        try:
            L.qb3_set_encoder_mode(p, mode)
            if index_chunk:
                L.qb3x_set_encoder_index_chunk(p, index_chunk)
            if quanta > 1:
                assert L.qb3_set_encoder_quanta(p, quanta, False)
            self.pitch = (L.qb3_max_encoded_size(p) + 3) // 4 * 4
            src = torch.from_numpy(np.ascontiguousarray(raster).view(np.uint8).reshape(-1)).cuda()
            self.dst = torch.full((self.n * self.pitch,), 0x5A, dtype=torch.uint8, device="cuda")
            self.sizes = (_sz * self.n)()
            k = L.qb3x_encode_mosaic(p, _vp(src.data_ptr()), self.W, self.H, 0, _vp(self.dst.data_ptr()), self.pitch, None, self.sizes, None)
            assert k == self.n and L.qb3_get_encoder_state(p) == 0, (k, self.n, qb3.last_error())
        finally:
            L.qb3_destroy_encoder(p)

    def host(self, k):
        return self.dst[k * self.pitch:k * self.pitch + self.sizes[k]].cpu().numpy()

    def handle(self, compat=None):
        """a decoder parsed from tile 0 on the device; the caller destroys it"""
        dims = (_sz * 3)()
        d = self.qb3.lib.qb3x_read_start_device(_vp(self.dst.data_ptr()), int(self.sizes[0]), dims, None)
        assert d, self.qb3.last_error()
        if compat is not None:
            self.qb3.lib.qb3x_set_decoder_compat(d, compat)
        return d

    def whole(self, sizes=None, compat=None):
        """(raster, [tile ok]) of qb3x_decode_mosaic on a handle of its own, with these sizes and this compat word"""
        L = self.qb3.lib
        sizes = sizes or self.sizes
        out = self.torch.full((self.H * self.W * self.b * self.tsz,), 0xA5, dtype=self.torch.uint8, device="cuda")
        d = self.handle(compat)
        try:
            L.qb3x_decode_mosaic(d, _vp(self.dst.data_ptr()), self.pitch, sizes, self.W, self.H, _vp(out.data_ptr()), 0, None, None)
            ok = [L.qb3x_decode_tile_ok(d, k) for k in range(self.n)]
        finally:
            L.qb3_destroy_decoder(d)
        return out.cpu().numpy().view(self.raster.dtype).reshape(self.H, self.W, self.b), ok


class Result:
    pass


def decode_windows(m, d, rects, expect, pads=None, odd=None, sizes=None):
    """qb3x_decode_mosaic_windows of m on handle d.  Every window lies in one 0xA5-filled device buffer, GAP bytes apart, window i with
    pads[i] values between its rows (its stride is then given, else 0) and, for i in odd, one byte off the dword its neighbours start
    on.  expect: the (H, W, bands) raster the windows are crops of.  The buffer is compared WHOLE: the rows of the windows that are ok
    against the crops, every other byte against 0xA5; a window that is not ok may hold anything inside its own rows.  Returns the
    call's results."""
    L, torch = m.qb3.lib, m.torch
    pads = pads or [0] * len(rects)
    odd = odd or ()
    pix = m.b * m.tsz
    at, spans = GAP, []
    for i, (x0, y0, w, h) in enumerate(rects):
        at = (at + 3) // 4 * 4 + (1 if i in odd else 0)
        stride = w * m.b + pads[i]
        spans.append((at, stride))
        at += h * stride * m.tsz + GAP
    want = np.full(at, 0xA5, dtype=np.uint8)
    buf = torch.from_numpy(want.copy()).cuda()
    wins = (Window * len(rects))()
    for i, (x0, y0, w, h) in enumerate(rects):
        wins[i] = Window(x0, y0, w, h, buf.data_ptr() + spans[i][0], spans[i][1] if pads[i] else 0)
    r = Result()
    r.n = L.qb3x_decode_mosaic_windows(d, _vp(m.dst.data_ptr()), m.pitch, sizes or m.sizes, m.W, m.H, wins, len(rects), None)
    r.ok = [L.qb3x_window_ok(d, i) for i in range(len(rects))]
    r.paths = [L.qb3x_window_path(d, i) for i in range(len(rects))]
    r.last = L.qb3x_last_window_path(d)
    r.segments = L.qb3x_last_window_segments(d)
    r.whole = L.qb3x_last_mosaic_whole_tiles(d)
    r.error = m.qb3.last_error()
    got = buf.cpu().numpy()
    for i, (x0, y0, w, h) in enumerate(rects):
        a, stride = spans[i]
        crop = np.ascontiguousarray(expect[y0:y0 + h, x0:x0 + w]).view(np.uint8).reshape(h, w * pix)
        for y in range(h):
            s = a + y * stride * m.tsz
            want[s:s + w * pix] = crop[y] if r.ok[i] else got[s:s + w * pix]
    r.wrong = [i for i, (x0, y0, w, h) in enumerate(rects) if r.ok[i] and any(
        not np.array_equal(got[spans[i][0] + y * spans[i][1] * m.tsz:][:w * pix], want[spans[i][0] + y * spans[i][1] * m.tsz:][:w * pix]) for y in range(h))]
    r.clean = bool(np.array_equal(got, want))
    assert r.n == sum(r.ok) and r.last == r.paths[-1] and all((p != 0) == bool(o) for p, o in zip(r.paths, r.ok)), (r.n, r.ok, r.paths, r.last)
    return r
