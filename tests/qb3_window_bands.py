"""What the tests of the band-selected window calls share (test_window_bands_plan.py, test_window_bands_decode.py): the selections of a
band count, the expected bytes -- always the SOURCE raster (or a second handle's whole decode) with the bands picked, never a window
call's -- and the sentinel-guarded destinations, which are qb3_window_dev's "unit" layout with `nsel` values a pixel in place of the
band count."""
import ctypes as C

import numpy as np

import qb3_window_dev as D

SENTINEL = D.SENTINEL
_vp = C.c_void_p
NAMES = ("qb3x_decode_windows_bands_device", "qb3x_read_windows_bands", "qb3x_last_window_gathers")


def selections(bands):
    """the selections of the fused cases, none longer than the band count: one band that is not core under the default band map (bands 0
    and 2 take band 1 off; with fewer than three bands the map is the identity), so that its core band is not selected; the reversed
    full list; three bands out of order; one with a repeat; for sixteen bands a permutation of all sixteen"""
    out = [[0] if bands >= 3 else [bands - 1], list(range(bands))[::-1]]
    if bands >= 3:
        out.append([2, 0, 1] if bands == 3 else [bands - 1, 0, 2])
    if bands >= 2:
        out.append([1, 1, 0, 1][:min(4, bands)])
    if bands == 16:
        out.append([(7 * k + 3) % 16 for k in range(16)])
    return out


def select(rows, bands, tsz, sel):
    """rows: (H, W * bands * tsz) bytes of a raster, a torch tensor or a numpy array; the same of the raster that holds band sel[k] of
    every pixel as its k-th value"""
    H = rows.shape[0]
    px = rows.reshape(H, -1, bands, tsz)[:, :, list(sel), :].reshape(H, -1)
    return px.contiguous() if hasattr(px, "contiguous") else np.ascontiguousarray(px)


class Layout(D.Layout):
    """the "unit" layout with nsel values a pixel; shift: every destination that many BYTES further on (1: off value alignment)"""

    def __init__(self, rects, nsel, tsz, mosaic=None, shift=0):
        super().__init__(rects, nsel * tsz, tsz, "unit", mosaic)
        self.offs = [o + shift for o in self.offs]
        self.size += shift


def bands_call(qb3, dec, d_c, lay, sel, host=None, index=None):
    """qb3x_decode_windows_bands_device (host: qb3x_read_windows_bands over the container's host copy) into a fresh sentinel buffer;
    returns (windows written, the buffer as a device tensor)"""
    import torch
    arr = qb3.band_array(sel)
    if host is not None:
        hbuf = np.full(lay.size + 16, SENTINEL, np.uint8)
        base = (-hbuf.ctypes.data) % 16                     # the layout's offsets count from a 16-byte address
        wins = qb3.window_array(lay.rects, [hbuf.ctypes.data + base + o for o in lay.offs], lay.strides())
        n = qb3.lib.qb3x_read_windows_bands(host, wins, len(lay.rects), arr, len(sel))
        return n, torch.from_numpy(hbuf[base:base + lay.size]).cuda()
    buf = lay.buffer()
    assert buf.data_ptr() % 16 == 0
    n = qb3.lib.qb3x_decode_windows_bands_device(dec.p, _vp(d_c.data_ptr()), _vp(index.data_ptr()) if index is not None else None, lay.array(qb3, buf), len(lay.rects),
                                                 arr, len(sel), _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return n, buf
