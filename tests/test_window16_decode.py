"""The 16-bit window kernels on the device (include/qb3x.h: qb3x_set_decoder_window_kernels, QB3X_WINK_U16; k_dec_win16.hip).
The invariant is the window calls': a window is the crop of what the whole decode writes, and no byte outside the window's rows is
written.  Expected bytes are the crop of the SOURCE raster (lossless containers) or of qb3x_decode_device on a second handle
(quanta, damaged or truncated streams), never of a window call.  Every destination lies in a sentinel-filled buffer with sentinel
bytes before, between (wide strides) and behind it.
With the bit set a call must go path 1, end with status 0 and count the window's segments; the same handle with the mask back at 0
must give the same bytes by path 2 and count the segments of the window's block rows.
Which value decoder a unit takes -- the code rule for rungs of 8 and above (px16_groups_hi), the 8-bit table below -- follows from
the generators: test_window16_plan.py::test_the_generators_reach_both_value_decoders restates the rungs of their rasters on the CPU
from the oracle's generator output and finds every raster of LANDSAT16 and DEM on both sides (NOISY3: the low amplitude)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
import qb3_window16 as W16  # noqa: E402
from qb3_window_dev import (FTL, BASE, BASE_Z, CF_H, SENTINEL, Layout, as_rows, batch_call, chunk_check, count, destination,  # noqa: E402
                            full_decode, make_container, segment_size, table_chunks, window_call)

pytestmark = pytest.mark.gpu

U16, I16 = W16.U16, W16.I16
BIT = W16.QB3X_WINK_U16


def check_windows(qb3, dec, d_c, rows, Wd, Ht, pix, wins, k0=0):
    """every window with the bit set (path 1, status 0, the window's segments) and with the mask back at 0 (path 2, the rows')"""
    L = qb3.lib
    bps = segment_size(qb3, dec)
    for i, win in enumerate(wins):
        dec.set_window_kernels(BIT)
        window_call(qb3, dec, d_c, win, rows, pix, 2, *destination("u16", k0 + i, 2))
        assert L.qb3x_last_window_path(dec.p) == 1 and L.qb3x_last_decode_status(dec.p) == 0, win
        assert L.qb3x_last_window_segments(dec.p) == L.qb3x_window_segments(dec.p, *win, None) == W.brute_segments(Wd, Ht, *win, bps=bps), win
        dec.set_window_kernels(0)
        window_call(qb3, dec, d_c, win, rows, pix, 2, *destination("u16", k0 + i, 2))
        assert L.qb3x_last_window_path(dec.p) == 2, win
        assert L.qb3x_last_window_segments(dec.p) == W.row_segments(Wd, Ht, win[1], win[3], bps), win


CASES = [(b, s, m) for b in (1, 2, 3, 4, 6, 8) for s in W16.shapes_of(b) for m in (FTL, BASE, BASE_Z)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-%dx%d-m%d" % (c[0], c[1][0], c[1][1], c[2]))
def test_window16_kernel(qb3, case):
    """uint16 (and int16 for 1 and 4 bands) x 1, 2, 3, 4, 6, 8 bands x FTL, BASE, BASE_Z x the default band map and the identity
    (3 bands and more) x LANDSAT16, DEM, NOISY3 (each container takes the next generator: every (bands, mode) sees all three over
    its four shapes and maps), windows of W16.windows, destinations at every halfword offset 0..7 with tight, wide-even and wide-odd rows"""
    from qb3_amd import device as qdev, synth
    bands, (Wd, Ht), mode = case
    maps = (None,) if bands < 3 else (None, list(range(bands)))
    types = (U16, I16) if bands in (1, 4) else (U16,)
    g = CASES.index(case)
    for cband in maps:
        for dt in types:
            gen = W16.GENERATORS[g % 3]
            g += 1
            img = synth.generate(Wd, Ht, bands, dt, gen, 31 * bands + Wd)
            d_c, n, _ = make_container(qb3, img, dt, mode, 2, cband)
            dec = qdev.DeviceDecoder(d_c, n)
            assert qb3.lib.qb3_get_mode(dec.p) == mode
            wins = W16.windows(Wd, Ht, 5 * Wd + bands + mode, segment_size(qb3, dec), 24 if dt == U16 and cband is None else 8)
            check_windows(qb3, dec, d_c, as_rows(img, Ht), Wd, Ht, 2 * bands, wins, g)
            dec.close()


@pytest.mark.parametrize("case", ((4, 1001, 259, BASE, "DEM"), (8, 1001, 259, FTL, "LANDSAT16"), (6, 132, 37, BASE_Z, "DEM"), (1, 260, 37, FTL, "LANDSAT16")),
                         ids=lambda c: "%d-%dx%d-m%d" % c[:4])
def test_window16_batch(qb3, case):
    """n = 1, 2 and 65 rectangles of one raster in one call, overlapping ones among them, and a mosaic laid out in one buffer; the
    host flavour (qb3x_read_windows) on the 4- and the 8-band case"""
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    bands, Wd, Ht, mode, gen = case
    pix = 2 * bands
    img = synth.generate(Wd, Ht, bands, U16, gen, 77)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, U16, mode, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    bps = segment_size(qb3, dec)
    wins = W16.windows(Wd, Ht, 9, bps, 65)
    host = d_c[:n].cpu().numpy() if bands in (4, 8) else None
    for nwin in (1, 2, 65):
        rects = wins[5:5 + nwin] if nwin < 65 else wins[3:68]          # (random ones overlap each other and the fixed ones)
        lay = Layout(rects, pix, 2, "u16")
        total = sum(W.brute_segments(Wd, Ht, *r, bps=bps) for r in rects)
        dec.set_window_kernels(BIT)
        got, buf = batch_call(qb3, dec, d_c, lay)
        assert got == nwin, qb3.last_error()
        lay.check(buf, rows)
        assert all(L.qb3x_window_ok(dec.p, i) == 1 and L.qb3x_window_path(dec.p, i) == 1 for i in range(nwin))
        assert L.qb3x_last_window_segments(dec.p) == total and L.qb3x_last_decode_status(dec.p) == 0
        dec.set_window_kernels(0)
        got, buf = batch_call(qb3, dec, d_c, lay)
        assert got == nwin
        lay.check(buf, rows)
        assert all(L.qb3x_window_path(dec.p, i) == 2 for i in range(nwin))
        if host is not None and nwin != 2:
            p, _ = W.open_handle(L, host)
            L.qb3x_set_decoder_window_kernels(p, BIT)
            got, buf = batch_call(qb3, None, None, lay, host=p)
            assert got == nwin, qb3.last_error()
            lay.check(buf, rows)
            assert all(L.qb3x_window_path(p, i) == 1 for i in range(nwin)) and L.qb3x_last_window_segments(p) == total
            out = np.full(7 * 9 * pix + 8, SENTINEL, np.uint8)             # ... and the single host call
            assert L.qb3x_read_window(p, Wd - 9, Ht - 7, 9, 7, out.ctypes.data, 0) == 7 * 9 * pix and L.qb3x_last_window_path(p) == 1
            assert np.array_equal(out[:7 * 9 * pix].reshape(7, -1), rows[Ht - 7:, (Wd - 9) * pix:].cpu().numpy()) and (out[7 * 9 * pix:] == SENTINEL).all()
            L.qb3_destroy_decoder(p)
    # a mosaic: 3 x 2 tiles of 40 x 20 pixels from six places of the raster, side by side in one image of 120 x 40 pixels
    tw, th = min(40, Wd // 3), min(20, Ht // 2)
    rects = [((7 + 31 * i) % (Wd - tw), (5 + 13 * i) % (Ht - th), tw, th) for i in range(6)]
    lay = Layout(rects, pix, 2, "u16", mosaic=(3 * tw * bands, [((i % 3) * tw * bands, (i // 3) * th) for i in range(6)], 2 * th))
    dec.set_window_kernels(BIT)
    got, buf = batch_call(qb3, dec, d_c, lay)
    assert got == 6 and all(L.qb3x_window_path(dec.p, i) == 1 for i in range(6))
    mosaic = buf[16:16 + 2 * 3 * tw * bands * 2 * th].view(2 * th, -1)
    for i, (x0, y0, w, h) in enumerate(rects):
        import torch
        assert torch.equal(mosaic[(i // 3) * th:(i // 3 + 1) * th, (i % 3) * tw * pix:(i % 3 + 1) * tw * pix], rows[y0:y0 + h, x0 * pix:(x0 + w) * pix]), i
    assert bool((buf[:16] == SENTINEL).all()) and bool((buf[16 + mosaic.numel():] == SENTINEL).all())
    dec.close()


def test_window16_dequantises_the_window(qb3):
    """quanta 3 on a BASE container: path 1, then the WINDOW is multiplied back; expected: the second handle's whole decode, cropped"""
    import torch
    from qb3_amd import device as qdev, synth
    Wd, Ht, b = 260, 37, 4
    img = synth.generate(Wd, Ht, b, U16, "LANDSAT16", 11)
    d_c, n, _ = make_container(qb3, img, U16, BASE, 2, quanta=3)
    want = full_decode(qb3, d_c, n)[0]
    assert want is not None and not torch.equal(want, img.reshape(-1).view(torch.uint8))
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(BIT)
    for i, win in enumerate(W16.windows(Wd, Ht, 3, 64, 8)):
        window_call(qb3, dec, d_c, win, want.view(Ht, -1), 2 * b, 2, *destination("u16", i, 2))
        assert qb3.lib.qb3x_last_window_path(dec.p) == 1
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- trust
@pytest.mark.parametrize("bands", (4, 8, 1))
def test_damaged_tables_and_short_streams_cost_time_not_pixels(qb3, bands):
    """a flipped entry byte (the chunk's check), a changed lane length under a re-sealed check (the kernel's own test of where a
    lane's units end), a stream cut inside the window's last segment and one cut behind the window's segments (the table's end):
    path 3 and the whole decode's bytes every time -- or, where the whole decode refuses the stream, a refused window"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    Wd, Ht = 1001, 259
    img = synth.generate(Wd, Ht, bands, U16, "DEM", 5)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, U16, FTL, 2)
    host = d_c[:n].cpu().numpy()
    chunks, data_off = table_chunks(host)
    E = 6 + 3 * bands + (80 if bands == 1 else 160)
    dec = qdev.DeviceDecoder(d_c, n)
    bps = segment_size(qb3, dec)
    nbx, nby = W.blocks_of(Wd, Ht)
    nseg = (nbx * nby + bps - 1) // bps
    assert L.qb3x_decoder_table_entries(dec.p) == nseg and sum(ln - 12 for _, ln in chunks) == nseg * E
    dec.close()
    per_chunk = (chunks[0][1] - 12) // E
    win = (40, 24, 300, 40)                                     # block rows 6..15, block columns 10..84
    first, last = (6 * nbx + 10) // bps, (15 * nbx + 84) // bps
    seg = first + 1

    def entry_at(k):
        return chunks[k // per_chunk][0] + 12 + (k % per_chunk) * E

    def expect_path3(bad, size, what):
        want = full_decode(qb3, bad, size)[0]
        dec = qdev.DeviceDecoder(bad, size)
        dec.set_window_kernels(BIT)
        window_call(qb3, dec, bad, win, None if want is None else want.view(Ht, -1), 2 * bands, 2, *destination("u16", 3, 2))
        if want is not None:
            assert L.qb3x_last_window_path(dec.p) == 3, what
        dec.close()
        return want

    # the sound container first: path 1
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(BIT)
    window_call(qb3, dec, d_c, win, rows, 2 * bands, 2, *destination("u16", 3, 2))
    assert L.qb3x_last_window_path(dec.p) == 1
    dec.close()
    e0 = entry_at(seg)
    bad = d_c.clone()
    bad[e0 + 7] ^= 0x10
    want = expect_path3(bad, n, "entry")
    assert want is not None and torch.equal(want.view(Ht, -1), rows)
    # lane 5's first length field + 1, the chunk's check sealed again: only the kernel's own test can tell
    bad = host.copy()
    fields = e0 + 6 + 3 * bands
    nf = E - 6 - 3 * bands
    v = int.from_bytes(bytes(bad[fields:fields + nf]), "little")
    bit = (10 if bands == 1 else 20) * 5
    f = (v >> bit) & 1023
    v = (v & ~(1023 << bit)) | (((f + 1) & 1023) << bit)
    bad[fields:fields + nf] = np.frombuffer(v.to_bytes(nf, "little"), np.uint8)
    c0, cl = chunks[seg // per_chunk]
    s16 = chunk_check(bad[c0 + 12:c0 + cl])
    assert chunk_check(host[c0 + 12:c0 + cl]) == int(host[c0 + 6]) | int(host[c0 + 7]) << 8      # (the formula is the encoder's)
    bad[c0 + 6], bad[c0 + 7] = s16 & 255, s16 >> 8
    d_bad = torch.zeros_like(d_c)
    d_bad[:n] = torch.from_numpy(bad).cuda()
    want = expect_path3(d_bad, n, "lengths")
    assert want is not None and torch.equal(want.view(Ht, -1), rows)
    # the stream ends in the middle of the window's last segment / behind the window's segments
    pos_last = int.from_bytes(bytes(host[entry_at(last):entry_at(last) + 6]), "little")
    pos_next = int.from_bytes(bytes(host[entry_at(last + 1):entry_at(last + 1) + 6]), "little")
    pos_far = int.from_bytes(bytes(host[entry_at(nseg - 2):entry_at(nseg - 2) + 6]), "little")
    for what, cut in (("cut inside", data_off + (pos_last + pos_next) // 16), ("cut behind", data_off + pos_far // 8)):
        assert data_off + pos_last // 8 < cut < n
        short = torch.zeros_like(d_c)
        short[:cut] = d_c[:cut]
        expect_path3(short, cut, what)


def test_not_taken_with_the_bit_set(qb3):
    """what the bit does not change: 8-bit RGB still goes through the old kernel (dec_window counted, dec_window16 not); uint16 x 5
    and uint16 x 4 in QB3M_CF_H go path 2; a level-1 table and an out-of-band index go path 3"""
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    win = (13, 9, 101, 21)

    def one(img, dt, mode, level, path, pix, want_index=False):
        d_c, n, index = make_container(qb3, img, dt, mode, level, want_index=want_index)
        dec = qdev.DeviceDecoder(d_c, n)
        dec.set_window_kernels(BIT)
        tsz = 1 if dt == 0 else 2
        window_call(qb3, dec, d_c, win, as_rows(img, img.shape[0]), pix, tsz, *destination("u16", 1, tsz), index)
        assert L.qb3x_last_window_path(dec.p) == path, (dt, mode, level)
        dec.close()

    L.qb3x_profile_enable(1)
    L.qb3x_profile_reset()
    try:
        one(synth.generate(260, 37, 3, 0, "NOISY3", 1), 0, FTL, 2, 1, 3)
        assert count(qb3, "dec_window") == 1 and count(qb3, "dec_window16") == 0
        one(synth.generate(260, 37, 4, U16, "LANDSAT16", 1), U16, FTL, 2, 1, 8)
        assert count(qb3, "dec_window") == 1 and count(qb3, "dec_window16") == 1
    finally:
        L.qb3x_profile_enable(0)
    one(synth.generate(260, 37, 5, U16, "LANDSAT16", 1), U16, FTL, 2, 2, 10)
    one(synth.generate(260, 37, 4, U16, "LANDSAT16", 1), U16, CF_H, 2, 2, 8)
    one(synth.generate(260, 37, 4, U16, "LANDSAT16", 1), U16, FTL, 1, 3, 8)
    one(synth.generate(260, 37, 4, U16, "LANDSAT16", 1), U16, FTL, 2, 3, 8, want_index=True)
