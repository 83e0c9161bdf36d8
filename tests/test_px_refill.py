"""The bit refills of the 8-bit lane-per-block decoders (qb3_px.h: px_switch hands what is left of its 32 bits to px_group; a refill
every four codes, lanes at rung 7 once more before the fourth).  Two rasters built here from the curve constant:

  ladder  block (bx, by) has k = (bx + 3 by) mod 10 and its pixels are base + 7 band + (noise & amp), amp = 2^max(k-1, 0) - 1,
          base = (3 (x div 32) + 5 (y div 16)) mod 200; in the k = 1 blocks the pixel the curve visits last is one lower, which makes
          rung-0 units WITH bits.  The lanes of a wave (a segment of 64 blocks) sit at every rung.
  zigzag  in block (bx, by) of band c the pixel visited i-th is 64 + (2^r - 1 for even i, else 0), r = (bx + 3 by + (0 if c == 1
          else c)) mod 8: from r = 2 on all sixteen codes of the G band (of the one band) have the long form of r + 2 bits, so four
          codes at rung 6 fill the 32 bits of a refill, and three codes at rung 7 the 27 bits a five-bit switch leaves, exactly.

The first tests need no GPU: a numpy restatement of band difference, delta, mag-sign and rung says which rungs the lanes of each wave
take, and the CPU oracle codes and decodes the rasters.  The GPU tests decode every container every way the library has and compare
the WHOLE destination, 0xA5-filled before the call, stride padding included."""
import ctypes as C
import functools

import numpy as np
import pytest

HILBERT = 0x01548CD9AEFB7623            # reference QB3common.h:193: nibble i = (y << 2 | x) of the pixel visited i-th
FTL, BASE, CF, BEST, STORED = 8, 4, 1, 7, 255
SHAPES = [(256, 16), (260, 20), (64, 64), (258, 18)]     # (the last: a shifted last block column and row)
BANDS = [1, 3, 4]
FILL = 0xA5
_vp = C.c_void_p


def curve():
    return [((HILBERT >> (60 - 4 * i)) & 3, (HILBERT >> (62 - 4 * i)) & 3) for i in range(16)]


def visit_index():
    """[y][x] -> i: the pixel (x, y) of a block is the one the curve visits i-th"""
    v = np.zeros((4, 4), np.int64)
    for i, (x, y) in enumerate(curve()):
        v[y, x] = i
    return v


@functools.lru_cache(maxsize=None)
def raster(name, w, h, b):
    """(h, w, b) uint8, read-only"""
    y, x = np.mgrid[0:h, 0:w]
    s = x // 4 + 3 * (y // 4)
    if name == "ladder":
        noise = np.random.default_rng(20261019).integers(0, 256, (h, w, b), dtype=np.int64)
        k = s % 10
        amp = (1 << np.maximum(k - 1, 0)) - 1
        base = (3 * (x // 32) + 5 * (y // 16)) % 200
        img = base[..., None] + 7 * np.arange(b) + (noise & amp[..., None])
        lx, ly = curve()[15]
        img[(k == 1) & (x % 4 == lx) & (y % 4 == ly)] -= 1
    else:
        even = visit_index()[y % 4, x % 4] % 2 == 0
        r = (s[..., None] + np.array([0 if c == 1 else c for c in range(b)])) % 8
        img = 64 + np.where(even[..., None], (1 << r) - 1, 0)
    img = (img & 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def units_of(img, nbits=8):
    """mag-sign values [block, band, 16] in curve order and rungs [block, band] of a raster under the default band map (R-G, G, B-G
    (, A)), blocks in raster order, the last block column / row shifted (reference QB3encode.h:439-441, QB3common.h:127-130)"""
    h, w, b = img.shape
    v = img.astype(np.int64)
    if b >= 3:
        v = v.copy()
        v[..., 0] -= img[..., 1]
        v[..., 2] -= img[..., 1]
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    seq = np.zeros((nbx * nby, b, 16), np.int64)
    for by in range(nby):
        for bx in range(nbx):
            x0, y0 = min(4 * bx, w - 4), min(4 * by, h - 4)
            for i, (x, y) in enumerate(curve()):
                seq[by * nbx + bx, :, i] = v[y0 + y, x0 + x]
    flat = seq.transpose(1, 0, 2).reshape(b, -1)
    mask = (1 << nbits) - 1
    d = np.diff(flat, axis=1, prepend=0) & mask
    d = np.where(d > mask >> 1, d - mask - 1, d)
    m = (((d << 1) ^ (d >> (nbits - 1))) & mask).reshape(b, nbx * nby, 16).transpose(1, 0, 2)
    used = np.bitwise_or.reduce(m, axis=2)
    rung = np.floor(np.log2(np.maximum(used, 1))).astype(np.int64)
    return m, rung


def code_bits(m, r):
    """bits of the sixteen codes of a unit at rung r >= 1 without the step (QB3M_FTL; reference QB3encode.h:30-33, 132-141)"""
    top, half = 1 << r, 1 << (r - 1)
    n = 0
    for v in m:
        v = int(v)
        if v == top or v == top - 1:
            v ^= 2 * top - 1
        n += r + (v >= half) + (v >= top)
    return n


def test_rungs_of_a_wave():
    """every rung 0..7 shares a segment (a wave: 64 blocks of one band) with a rung-7 lane and with a lane at rung 2 or below, in
    every shape and band count of the ladder raster; rung 0 occurs with and without bits"""
    for (w, h) in SHAPES[:3]:
        for b in BANDS:
            m, rung = units_of(raster("ladder", w, h, b))
            met = set()
            for s0 in range(0, len(rung), 64):
                for c in range(b):
                    here = set(rung[s0:s0 + 64, c].tolist())
                    if 7 in here and min(here) <= 2:
                        met |= here
            assert met == set(range(8)), (w, h, b, sorted(met))
            zero = m[rung == 0]
            assert (zero.max(axis=1) == 0).any() and (zero.max(axis=1) == 1).any(), (w, h, b)


def test_zigzag_fills_the_buffers():
    """units whose sixteen codes are all r + 2 bits long, for r = 6 (four codes are the 32 bits of a refill) and r = 7 (three codes
    are the 27 bits behind a five-bit switch), in every shape and band count; and every rung occurs"""
    for (w, h) in SHAPES[:3]:
        for b in BANDS:
            m, rung = units_of(raster("zigzag", w, h, b))
            g = 1 if b >= 3 else 0
            assert set(rung[:, g].tolist()) == set(range(8)), (w, h, b)
            for r in (6, 7):
                full = [u for u in m[rung[:, g] == r, g] if code_bits(u, r) == 16 * (r + 2)]
                assert full, (w, h, b, r)
                top = 1 << r
                assert all(int(v) > top for u in full for v in u)          # every value in the long form, none of the swapped pair


@pytest.mark.parametrize("name", ["ladder", "zigzag"])
def test_oracle_codes_them(oracle, name):
    """the CPU oracle's containers of the rasters are not STORED and decode to the rasters"""
    for (w, h) in SHAPES:
        for b in BANDS:
            img = raster(name, w, h, b)
            for mode in (FTL, BASE) + ((CF, BEST) if name == "ladder" else ()):
                s = oracle.encode(img, 0, mode)
                assert s[10] != STORED and len(s) < img.size, (name, w, h, b, mode, len(s))
                out, dims, _, _ = oracle.decode(s)
                assert dims == (w, h, b) and np.array_equal(out, img.ravel()), (name, w, h, b, mode)


# ------------------------------------------------------------------------------------------------------------------ on the GPU
def stream():
    import torch
    return _vp(torch.cuda.current_stream().cuda_stream)


def window_of(w, h):
    """a window that cuts its first and its last segment: it starts and ends inside a block, a few blocks from the raster's edges"""
    return 9, 5, w - 19, h - 11


def check_whole(qb3, dec, d_c, index, img, extra):
    """qb3x_decode_device into 0xA5 bytes, rows `extra` values wider than the raster's: every byte of the destination"""
    import torch
    h, w, b = img.shape
    line, stride = w * b, w * b + extra
    qb3.lib.qb3_set_decoder_stride(dec.p, stride if extra else 0)
    buf = torch.full((h * stride + 64,), FILL, dtype=torch.uint8, device="cuda")
    n = qb3.lib.qb3x_decode_device(dec.p, _vp(d_c.data_ptr()), _vp(buf.data_ptr()), _vp(index.data_ptr()) if index is not None else None, stream())
    got = buf.cpu().numpy()
    assert n != 0, qb3.last_error()
    assert qb3.lib.qb3x_last_decode_status(dec.p) == 0
    want = np.full(h * stride + 64, FILL, np.uint8)
    want[:h * stride].reshape(h, stride)[:, :line] = img.reshape(h, line)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%d bytes differ, the first at row %d byte %d" % (len(bad), bad[0] // stride, bad[0] % stride))


def check_window(qb3, dec, d_c, index, img, path1):
    """one qb3x_decode_window_device into 0xA5 bytes, rows four values wider than the window's: every byte of the destination"""
    import torch
    h, w, b = img.shape
    x0, y0, ww, wh = window_of(w, h)
    line, stride = ww * b, ww * b + 4
    buf = torch.full((wh * stride + 64,), FILL, dtype=torch.uint8, device="cuda")
    n = qb3.lib.qb3x_decode_window_device(dec.p, _vp(d_c.data_ptr()), _vp(index.data_ptr()) if index is not None else None,
                                          x0, y0, ww, wh, _vp(buf.data_ptr()), stride, stream())
    got = buf.cpu().numpy()
    assert n == wh * line, qb3.last_error()
    assert qb3.lib.qb3x_last_decode_status(dec.p) == 0
    if path1:
        assert qb3.lib.qb3x_last_window_path(dec.p) == 1 and qb3.lib.qb3x_last_window_segments(dec.p) >= 2
    want = np.full(wh * stride + 64, FILL, np.uint8)
    want[:wh * stride].reshape(wh, stride)[:, :line] = img[y0:y0 + wh, x0:x0 + ww].reshape(wh, line)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("window: %d bytes differ, the first at row %d byte %d" % (len(bad), bad[0] // stride, bad[0] % stride))


def container(img, mode, level, want_index):
    """(device tensor with the container and zeros behind it, size, host copy, out-of-band index or None)"""
    import torch
    from qb3_amd import device as qdev
    h, w, b = img.shape
    enc = qdev.DeviceEncoder(w, h, b, 0, mode=mode, want_index=want_index, index_chunk=level)
    dst, n, index = enc.encode(torch.from_numpy(img.copy()).cuda().view(-1))
    d_c = torch.zeros((n + 3) // 4 * 4 + 64, dtype=torch.uint8, device="cuda")
    d_c[:n] = dst[:n]
    index = index.clone() if index is not None else None
    enc.close()
    return d_c, n, d_c[:n].cpu().numpy(), index


CASES = [(name, s, b, mode) for name in ("ladder", "zigzag") for s in SHAPES for b in BANDS for mode in (FTL, BASE)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-%d-m%d" % (c[0], c[1][0], c[1][1], c[2], c[3]))
def test_decode_every_route(qb3, oracle, case):
    """FTL and BASE: from the container alone at table level 2 (dec_px_kernel's table branch, the u8 window kernel) and at level 1 (the
    walk, then the index branch), and with the out-of-band index; the whole raster and a window each; the oracle reads the same
    container to the same bytes"""
    from qb3_amd import device as qdev
    name, (w, h), b, mode = case
    img = raster(name, w, h, b)
    extra = 4 if (w, h) == (260, 20) else 0
    for level in (2, 1):
        d_c, n, host, index = container(img, mode, level, level == 2)
        assert host[10] != STORED, "a STORED container decodes nothing"
        dec = qdev.DeviceDecoder(d_c, n)
        for ix in (None, index) if level == 2 else (None,):
            check_whole(qb3, dec, d_c, ix, img, extra)
            check_window(qb3, dec, d_c, ix, img, level == 2 and ix is None)
        dec.close()
        if level == 2:
            out, dims, _, _ = oracle.decode(host)
            assert out is not None and dims == (w, h, b) and np.array_equal(out, img.ravel())


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(s, b, mode) for s in SHAPES for b in BANDS for mode in (CF, BEST)], ids=lambda c: "%dx%d-%d-m%d" % (c[0][0], c[0][1], c[1], c[2]))
def test_decode_common_factor(qb3, oracle, case):
    """the ladder raster in QB3M_CF and QB3M_BEST: dec_px_best_kernel (plain units through px_group, the others parsed by the lane)
    and, with QB3X_WINK_CF8, the window kernel of these modes"""
    from qb3_amd import device as qdev
    (w, h), b, mode = case
    img = raster("ladder", w, h, b)
    extra = 4 if (w, h) == (260, 20) else 0
    d_c, n, host, _ = container(img, mode, 2, False)
    assert host[10] != STORED, "a STORED container decodes nothing"
    dec = qdev.DeviceDecoder(d_c, n)
    check_whole(qb3, dec, d_c, None, img, extra)
    dec.set_window_kernels(qb3.QB3X_WINK_CF8)
    check_window(qb3, dec, d_c, None, img, host[10] in (1, 5))      # (QB3M_CF, QB3M_CF_H: not the RLE modes QB3M_BEST may end in)
    dec.close()
    out, dims, _, _ = oracle.decode(host)
    assert out is not None and dims == (w, h, b) and np.array_equal(out, img.ravel())


@pytest.mark.gpu
@pytest.mark.parametrize("b", [1, 4])
def test_decode_16bit_below_rung_8(qb3, oracle, b):
    """dec_px16_kernel calls px_group with a position only, for units below rung 8: 256 x 16 uint16 values whose differences stay
    keep every unit below rung 8 (the ladder's amplitudes, capped; rung 7 occurs), from the container alone and with the index"""
    import torch
    from qb3_amd import device as qdev
    w, h = 256, 16
    img8 = raster("ladder", w, h, 4)[..., :b]
    y, x = np.mgrid[0:h, 0:w]
    amp = (1 << np.maximum((x // 4 + 3 * (y // 4)) % 10 - 1, 0)) - 1
    img = (7 * np.arange(b) + (img8.astype(np.int64) & np.minimum(amp, 127 if b == 1 else 63)[..., None])).astype(np.uint16)
    rungs = units_of(img, 16)[1]
    assert rungs.max() == 7 and rungs.min() == 0
    d_img = torch.from_numpy(img.view(np.int16)).cuda().view(-1)
    enc = qdev.DeviceEncoder(w, h, b, 2, mode=BASE, want_index=True, index_chunk=2)
    d_c, n, index = enc.encode(d_img)
    host = d_c[:n].cpu().numpy()
    assert host[10] != STORED, "a STORED container decodes nothing"
    dec = qdev.DeviceDecoder(d_c, n)
    for ix in (None, index):
        buf = torch.full((img.nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
        dec.decode(d_c, out=buf, index=ix)
        assert qb3.lib.qb3x_last_decode_status(dec.p) == 0
        got = buf.cpu().numpy()
        assert np.array_equal(got[:img.nbytes], img.view(np.uint8).ravel()) and (got[img.nbytes:] == FILL).all()
    out, dims, _, _ = oracle.decode(host)
    assert out is not None and np.array_equal(out, img.view(np.uint8).ravel())
