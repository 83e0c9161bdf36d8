"""The window kernels for 8-bit common-factor rasters on the device (include/qb3x.h: qb3x_set_decoder_window_kernels, QB3X_WINK_CF8;
k_dec_win_best.hip).  The invariant is the window calls': a window is the crop of what the whole decode writes, and no byte outside the
window's rows is written.  Expected bytes are the crop of the SOURCE raster (lossless containers) or of qb3x_decode_device on a second
handle (quanta, damaged or truncated containers), never of a window call.  Every destination lies in a sentinel-filled buffer with
sentinel bytes before, between (wide strides) and behind it.
With the bit set a call must go path 1, end with status 0 and count the window's segments; the same handle with the mask back at 0 must
give the same bytes by path 2.  The rasters (qb3_window_best.py) reach the index form, common-factor units with their own factor and
with the one in force (across segment boundaries: the entry's), and the fast path beside them; test_window_best_plan.py shows on the CPU
that every one of them is a coded common-factor container at every shape, band count and mode used here, so the mode byte is ASSERTED."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
import qb3_window16 as W16  # noqa: E402
import qb3_window_best as WB  # noqa: E402
from qb3_window_best import device_raster  # noqa: E402
from qb3_window_dev import (FTL, SENTINEL, Layout, as_rows, batch_call, chunk_check, count, destination, full_decode,  # noqa: E402
                            make_container, segments_of, single_calls, table_chunks, window_call)

pytestmark = pytest.mark.gpu

CF, CF_H, BEST = WB.CF, WB.CF_H, WB.BEST
BIT = WB.QB3X_WINK_CF8

CASES = [(b, s) for b in WB.BANDS for s in WB.SHAPES]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-%dx%d" % (c[0], c[1][0], c[1][1]))
def test_window_best_kernel(qb3, oracle, case):
    """1, 3, 4 bands x the four shapes; inside: QB3M_CF (Z order), QB3M_CF_H, QB3M_BEST x table levels 1 and 2 x the six rasters x the
    default band map and the identity (3 and 4 bands), the windows of W16.windows, destinations 0..3 bytes behind a dword with tight
    and wide rows: the source's crop, sentinels intact, path 1, the window's segments, status 0"""
    from qb3_amd import device as qdev
    L = qb3.lib
    bands, (Wd, Ht) = case
    maps = (None,) if bands < 3 else (None, list(range(bands)))
    k = 0
    for name in WB.NAMES:
        img = device_raster(oracle, name, Wd, Ht, bands, 7 * Wd + bands)
        rows = as_rows(img, Ht)
        for mode in WB.MODES:
            for level in (1, 2):
                for cband in maps:
                    d_c, n, _ = make_container(qb3, img, 0, mode, level, cband)
                    dec = qdev.DeviceDecoder(d_c, n)
                    assert L.qb3_get_mode(dec.p) == (1 if mode == CF else 5), (name, mode)
                    dec.set_window_kernels(BIT)
                    for win in W16.windows(Wd, Ht, 5 * Wd + bands + mode + level, 64, 6 if cband is None else 2):
                        k += 1
                        window_call(qb3, dec, d_c, win, rows, bands, 1, *destination("cf8", k, 1))
                        what = (name, mode, level, cband, win)
                        assert L.qb3x_last_window_path(dec.p) == 1 and L.qb3x_last_decode_status(dec.p) == 0, what
                        assert L.qb3x_last_window_segments(dec.p) == L.qb3x_window_segments(dec.p, *win, None) == W.brute_segments(Wd, Ht, *win), what
                    dec.close()


@pytest.mark.parametrize("case", ((3, 260, 37, CF_H, 2, "mixed"), (4, 1001, 259, BEST, 1, "FEW"), (1, 100, 100, CF, 2, "TERRACE")),
                         ids=lambda c: "%d-%dx%d-m%d-l%d" % c[:5])
def test_the_bit_only_chooses_the_way(qb3, oracle, case):
    """the same container and handle: with the bit path 1 and one dec_window_best launch a call, without it path 2 (the segments of
    the window's block rows), no such launch, the same bytes"""
    from qb3_amd import device as qdev
    L = qb3.lib
    bands, Wd, Ht, mode, level, name = case
    img = device_raster(oracle, name, Wd, Ht, bands, 3)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, 0, mode, level)
    dec = qdev.DeviceDecoder(d_c, n)
    assert L.qb3_get_mode(dec.p) == (1 if mode == CF else 5)
    L.qb3x_profile_enable(1)
    L.qb3x_profile_reset()
    try:
        for i, win in enumerate(W16.windows(Wd, Ht, 17, 64, 6)):
            dec.set_window_kernels(BIT)
            before = count(qb3, "dec_window_best")
            window_call(qb3, dec, d_c, win, rows, bands, 1, *destination("cf8", i, 1))
            assert L.qb3x_last_window_path(dec.p) == 1 and count(qb3, "dec_window_best") == before + 1, win
            assert L.qb3x_last_window_segments(dec.p) == W.brute_segments(Wd, Ht, *win), win
            dec.set_window_kernels(0)
            window_call(qb3, dec, d_c, win, rows, bands, 1, *destination("cf8", i, 1))
            assert L.qb3x_last_window_path(dec.p) == 2 and count(qb3, "dec_window_best") == before + 1, win
            assert L.qb3x_last_window_segments(dec.p) == W.row_segments(Wd, Ht, win[1], win[3], 64), win
        assert count(qb3, "dec_window") == 0 and count(qb3, "dec_window16") == 0
    finally:
        L.qb3x_profile_enable(0)
    dec.close()


@pytest.mark.parametrize("case", ((3, 1001, 259, BEST, 2, "mixed"), (4, 260, 37, CF_H, 1, "scaled16"), (1, 100, 100, CF, 2, "PALETTE")),
                         ids=lambda c: "%d-%dx%d-m%d-l%d" % c[:5])
def test_window_best_batch(qb3, oracle, case):
    """n = 1, 7 and 200 rectangles of one raster in one call, overlapping ones among them, in one buffer at mixed alignments, and a
    mosaic through dst_stride: the bytes of n single calls (and the source's crop), ONE dec_window_best launch a call, every window
    ok by path 1, the segment total the sum over the windows"""
    import torch
    from qb3_amd import device as qdev
    L = qb3.lib
    bands, Wd, Ht, mode, level, name = case
    img = device_raster(oracle, name, Wd, Ht, bands, 77)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, 0, mode, level)
    dec = qdev.DeviceDecoder(d_c, n)
    assert L.qb3_get_mode(dec.p) == (1 if mode == CF else 5)
    dec.set_window_kernels(BIT)
    wins = W16.windows(Wd, Ht, 9, 64, 200)
    wins = wins[1:] if Wd > 1000 else wins                                 # (the whole large raster once is enough: the mosaic's loop below)
    L.qb3x_profile_enable(1)
    L.qb3x_profile_reset()
    try:
        for nwin in (1, 7, 200):
            rects = wins[5:5 + nwin] if nwin < 200 else wins[3:203]        # (random ones overlap each other and the fixed ones)
            lay = Layout(rects, bands, 1, "cf8")
            total = sum(W.brute_segments(Wd, Ht, *r) for r in rects)
            before = count(qb3, "dec_window_best")
            got, buf = batch_call(qb3, dec, d_c, lay)
            assert got == nwin, qb3.last_error()
            assert count(qb3, "dec_window_best") == before + 1
            lay.check(buf, rows)
            assert all(L.qb3x_window_ok(dec.p, i) == 1 and L.qb3x_window_path(dec.p, i) == 1 for i in range(nwin))
            assert L.qb3x_last_window_segments(dec.p) == total and L.qb3x_last_decode_status(dec.p) == 0
            assert torch.equal(buf, single_calls(qb3, dec, d_c, lay))
    finally:
        L.qb3x_profile_enable(0)
    # a mosaic: 3 x 2 tiles from six places of the raster, side by side in one image
    tw, th = min(40, Wd // 3), min(20, Ht // 2)
    rects = [((7 + 31 * i) % (Wd - tw), (5 + 13 * i) % (Ht - th), tw, th) for i in range(6)]
    line = 3 * tw * bands
    lay = Layout(rects, bands, 1, "cf8", mosaic=(line, [((i % 3) * tw * bands, (i // 3) * th) for i in range(6)], 2 * th))
    got, buf = batch_call(qb3, dec, d_c, lay)
    assert got == 6 and all(L.qb3x_window_path(dec.p, i) == 1 for i in range(6))
    mosaic = buf[16:16 + line * 2 * th].view(2 * th, -1)
    for i, (x0, y0, w, h) in enumerate(rects):
        assert torch.equal(mosaic[(i // 3) * th:(i // 3 + 1) * th, (i % 3) * tw * bands:(i % 3 + 1) * tw * bands], rows[y0:y0 + h, x0 * bands:(x0 + w) * bands]), i
    assert bool((buf[:16] == SENTINEL).all()) and bool((buf[16 + mosaic.numel():] == SENTINEL).all())
    dec.close()


def test_window_best_dequantises_the_window(qb3, oracle):
    """quanta 3 on a QB3M_CF_H container: path 1, then the WINDOW is multiplied back; expected: the second handle's whole decode, cropped"""
    import torch
    from qb3_amd import device as qdev
    Wd, Ht, b = 260, 37, 3
    img = device_raster(oracle, "mixed", Wd, Ht, b, 11)
    d_c, n, _ = make_container(qb3, img, 0, CF_H, 2, quanta=3)
    want = full_decode(qb3, d_c, n)[0]
    assert want is not None and not torch.equal(want, img.reshape(-1))
    dec = qdev.DeviceDecoder(d_c, n)
    assert qb3.lib.qb3_get_mode(dec.p) == 5
    dec.set_window_kernels(BIT)
    for i, win in enumerate(W16.windows(Wd, Ht, 3, 64, 8)):
        window_call(qb3, dec, d_c, win, want.view(Ht, -1), b, 1, *destination("cf8", i, 1))
        assert qb3.lib.qb3x_last_window_path(dec.p) == 1
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- trust
@pytest.mark.parametrize("bands", WB.BANDS)
def test_damage_costs_time_not_pixels(qb3, oracle, bands):
    """a flipped entry bit under the old check (the chunk's check: status bit 5); a block's length, a block's entering rung and an
    entry's position changed under a RE-SEALED check (the kernel's own tests: where a block's units end, the rung they leave, the
    bits they are read from); in a batch only the windows that hold the damaged segment fall back; a stream cut in front of the
    window's segments, inside its last segment and behind them.  Path 3, a nonzero status and the bytes of a second handle's whole
    decode of the same damaged container every time; every one of these containers must have a whole decode"""
    import torch
    from qb3_amd import device as qdev
    L = qb3.lib
    Wd, Ht = 1001, 259
    img = device_raster(oracle, "mixed", Wd, Ht, bands, 5)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, 0, CF_H, 2)
    host = d_c[:n].cpu().numpy()
    chunks, data_off = table_chunks(host)
    E = WB.entry_bytes(bands)
    nbx, nby = W.blocks_of(Wd, Ht)
    nseg = (nbx * nby + 63) // 64
    dec = qdev.DeviceDecoder(d_c, n)
    assert L.qb3_get_mode(dec.p) == 5
    assert L.qb3x_decoder_table_entries(dec.p) == nseg and sum(ln - 12 for _, ln in chunks) == nseg * E
    dec.close()
    per_chunk = (chunks[0][1] - 12) // E
    win = (40, 24, 300, 40)                                     # block rows 6..15, block columns 10..84
    first, last = (6 * nbx + 10) // 64, (15 * nbx + 84) // 64
    seg = first + 1
    assert seg in segments_of(Wd, Ht, win)

    def entry_at(k):
        return chunks[k // per_chunk][0] + 12 + (k % per_chunk) * E

    def resealed(change):
        """the container with change(bytes, offset of entry seg) applied and the chunk's 16-bit check made again, on the device"""
        bad = host.copy()
        change(bad, entry_at(seg))
        assert not np.array_equal(bad, host)
        c0, cl = chunks[seg // per_chunk]
        s16 = chunk_check(bad[c0 + 12:c0 + cl])
        bad[c0 + 6], bad[c0 + 7] = s16 & 255, s16 >> 8
        d_bad = torch.zeros_like(d_c)
        d_bad[:n] = torch.from_numpy(bad).cuda()
        return d_bad

    def expect_path3(bad, size, what, bit=0):
        want = full_decode(qb3, bad, size)[0]
        dec = qdev.DeviceDecoder(bad, size)
        dec.set_window_kernels(BIT)
        window_call(qb3, dec, bad, win, None if want is None else want.view(Ht, -1), bands, 1, *destination("cf8", 3, 1))
        if want is not None:
            assert L.qb3x_last_window_path(dec.p) == 3 and L.qb3x_last_decode_status(dec.p) != 0, what
            assert L.qb3x_last_decode_status(dec.p) & bit == bit, what
        dec.close()
        return want

    c0, cl = chunks[seg // per_chunk]
    assert chunk_check(host[c0 + 12:c0 + cl]) == int(host[c0 + 6]) | int(host[c0 + 7]) << 8      # (the formula is the encoder's)
    # the sound container first: path 1
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(BIT)
    window_call(qb3, dec, d_c, win, rows, bands, 1, *destination("cf8", 3, 1))
    assert L.qb3x_last_window_path(dec.p) == 1
    dec.close()
    # a flipped bit in the entry, the check left as it was
    bad = d_c.clone()
    bad[entry_at(seg) + WB.field_at(bands, 9)] ^= 0x10
    want = expect_path3(bad, n, "entry", bit=32)
    assert want is not None and torch.equal(want.view(Ht, -1), rows)

    # re-sealed: only the kernel's own tests can tell
    def longer(b, e0):                      # block 5's length + 1
        at = e0 + WB.field_at(bands, 5)
        f = int(b[at]) | int(b[at + 1]) << 8
        f = (f & 0xf000) | ((f + 1) & 0xfff)
        b[at], b[at + 1] = f & 255, f >> 8

    def other_rung(b, e0):                  # block 5 entered one rung higher in band 0
        at = e0 + WB.field_at(bands, 5) + 1
        b[at] = (int(b[at]) & 0x8f) | ((((int(b[at]) >> 4) & 7) + 1) & 7) << 4

    def moved(b, e0):                       # the segment starts 512 bits from where it does
        b[e0 + 1] ^= 2

    for what, change in (("length", longer), ("rung", other_rung), ("position", moved)):
        want = expect_path3(resealed(change), n, what)
        assert want is not None and torch.equal(want.view(Ht, -1), rows), what
    # a batch over the container with the longer block: the windows that hold segment `seg` fall back, the others keep path 1
    d_bad = resealed(longer)
    dec = qdev.DeviceDecoder(d_bad, n)
    dec.set_window_kernels(BIT)
    rects = [win] + W16.windows(Wd, Ht, 21, 64, 30)[1:]
    lay = Layout(rects, bands, 1, "cf8")
    got, buf = batch_call(qb3, dec, d_bad, lay)
    assert got == len(rects), qb3.last_error()
    lay.check(buf, rows)
    paths = [L.qb3x_window_path(dec.p, i) for i in range(len(rects))]
    assert paths == [3 if seg in segments_of(Wd, Ht, r) else 1 for r in rects] and 1 in paths and 3 in paths
    dec.close()
    # the stream ends in front of the window's first segment (the window lies wholly behind the cut), in the middle of its last
    # segment, and behind all its segments (the window lies wholly in front of the cut).  The whole decode reads zeros behind a
    # stream's end, as the reference's reader does, and must give a raster every time -- a refusal would leave path 3 unasserted
    def pos_of(k):
        return int.from_bytes(bytes(host[entry_at(k):entry_at(k) + 6]), "little")

    assert 0 < first and last + 1 < nseg - 2
    x0, y0, w, h = win
    crop = (slice(y0, y0 + h), slice(x0 * bands, (x0 + w) * bands))
    for what, cut, sound in (("cut in front", data_off + (pos_of(first - 1) + pos_of(first)) // 16, False),
                             ("cut inside", data_off + (pos_of(last) + pos_of(last + 1)) // 16, None),
                             ("cut behind", data_off + pos_of(nseg - 2) // 8, True)):
        assert data_off < cut < n
        assert (cut < data_off + pos_of(first) // 8) if what == "cut in front" else (data_off + pos_of(last) // 8 < cut)
        short = torch.zeros_like(d_c)
        short[:cut] = d_c[:cut]
        want = expect_path3(short, cut, what)
        assert want is not None, what
        # (behind all of the window's segments the cut leaves its pixels the source's, in front of them it cannot; a cut inside
        # the last segment may lie behind the window's own blocks)
        assert sound is None or torch.equal(want.view(Ht, -1)[crop], rows[crop]) == sound, what


def test_host_flavour_and_python(qb3, oracle):
    """qb3x_read_window and qb3x_read_windows on a host handle with the bit; DeviceDecoder.set_window_kernels with decode_window and
    decode_windows"""
    import torch
    from qb3_amd import device as qdev
    L = qb3.lib
    Wd, Ht, b = 260, 37, 3
    img = device_raster(oracle, "FEW", Wd, Ht, b, 2)
    rows = as_rows(img, Ht)
    d_c, n, _ = make_container(qb3, img, 0, BEST, 2)
    host = d_c[:n].cpu().numpy()
    p, _ = W.open_handle(L, host)
    assert L.qb3_get_mode(p) == 5
    L.qb3x_set_decoder_window_kernels(p, BIT)
    rects = W16.windows(Wd, Ht, 4, 64, 7)
    lay = Layout(rects, b, 1, "cf8")
    got, buf = batch_call(qb3, None, None, lay, host=p)
    assert got == len(rects), qb3.last_error()
    lay.check(buf, rows)
    assert all(L.qb3x_window_path(p, i) == 1 for i in range(len(rects)))
    assert L.qb3x_last_window_segments(p) == sum(W.brute_segments(Wd, Ht, *r) for r in rects)
    out = np.full(7 * 9 * b + 8, SENTINEL, np.uint8)                       # ... and the single host call
    assert L.qb3x_read_window(p, Wd - 9, Ht - 7, 9, 7, out.ctypes.data, 0) == 7 * 9 * b and L.qb3x_last_window_path(p) == 1
    assert np.array_equal(out[:7 * 9 * b].reshape(7, -1), rows[Ht - 7:, (Wd - 9) * b:].cpu().numpy()) and (out[7 * 9 * b:] == SENTINEL).all()
    L.qb3_destroy_decoder(p)
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(qb3.QB3X_WINK_CF8)
    one = dec.decode_window(d_c, 33, 5, 100, 20)
    assert torch.equal(one, img[5:25, 33:133]) and L.qb3x_last_window_path(dec.p) == 1
    many = dec.decode_windows(d_c, rects)
    assert all(torch.equal(t, img[y0:y0 + h, x0:x0 + w]) for t, (x0, y0, w, h) in zip(many, rects))
    assert all(L.qb3x_window_path(dec.p, i) == 1 for i in range(len(rects)))
    dec.close()


def test_not_taken_with_the_bit_set(qb3, oracle):
    """what the bit does not change: 8-bit RGB FTL still goes through the old kernel; 8-bit x 2 and x 5 and uint16 x 4 in QB3M_CF_H go
    path 2; a container whose RLE0 pass won and an out-of-band index go path 3; with both bits a uint16 x 4 FTL raster goes through
    dec_window16"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    win = (13, 9, 101, 21)

    def one(img, dt, mode, path, want_index=False, mask=BIT, mode_byte=None):
        d_c, n, index = make_container(qb3, img, dt, mode, 2, want_index=want_index)
        dec = qdev.DeviceDecoder(d_c, n)
        assert L.qb3_get_mode(dec.p) == (mode if mode_byte is None else mode_byte)
        dec.set_window_kernels(mask)
        tsz = 1 if dt == 0 else 2
        window_call(qb3, dec, d_c, win, as_rows(img, img.shape[0]), img.shape[2] * tsz, tsz, *destination("cf8", 1, tsz), index)
        assert L.qb3x_last_window_path(dec.p) == path, (dt, mode, img.shape)
        dec.close()

    L.qb3x_profile_enable(1)
    L.qb3x_profile_reset()
    try:
        one(device_raster(oracle, "NOISY3", 260, 37, 3, 1), 0, FTL, 1)
        assert count(qb3, "dec_window") == 1 and count(qb3, "dec_window_best") == 0
        one(synth.generate(260, 37, 4, W16.U16, "LANDSAT16", 1), W16.U16, FTL, 1, mask=BIT | W16.QB3X_WINK_U16)
        assert count(qb3, "dec_window16") == 1 and count(qb3, "dec_window_best") == 0
        one(device_raster(oracle, "mixed", 260, 37, 2, 1), 0, CF_H, 2)
        one(device_raster(oracle, "mixed", 260, 37, 5, 1), 0, CF_H, 2)
        one(synth.generate(260, 37, 4, W16.U16, "LANDSAT16", 1), W16.U16, CF_H, 2)
        one(torch.from_numpy(oracle.generate(260, 37, 3, 0, "CONST", 1)).cuda(), 0, BEST, 3, mode_byte=7)
        one(device_raster(oracle, "mixed", 260, 37, 3, 1), 0, CF_H, 3, want_index=True)
        assert count(qb3, "dec_window_best") == 0
        one(device_raster(oracle, "mixed", 260, 37, 3, 1), 0, CF_H, 1)     # (the same raster without the out-of-band index: taken)
        assert count(qb3, "dec_window_best") == 1
    finally:
        L.qb3x_profile_enable(0)


def test_a_window_repeats(qb3, oracle):
    """the same window twenty times on one handle: identical bytes (nothing of a call is left for the next)"""
    import torch
    from qb3_amd import device as qdev
    Wd, Ht, b = 1001, 259, 3
    img = device_raster(oracle, "mixed", Wd, Ht, b, 9)
    d_c, n, _ = make_container(qb3, img, 0, BEST, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(BIT)
    first = None
    for i in range(20):
        out = dec.decode_window(d_c, 501, 117, 256, 100).clone()
        assert qb3.lib.qb3x_last_window_path(dec.p) == 1
        first = out if first is None else first
        assert torch.equal(out, first)
    assert torch.equal(first, img[117:217, 501:757])
    dec.close()
