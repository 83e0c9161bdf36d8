"""The window kernels of the remaining common-factor rasters on the device (include/qb3x.h: qb3x_set_decoder_window_kernels,
QB3X_WINK_CFU; k_dec_win_best_unit.hip): the common-factor streams of 8-bit rasters of 2 or 5 to 16 bands, of 16/32/64-bit rasters of
several bands and of one-band 16/32/64-bit rasters.  The invariant is the window calls': a window is the crop of what the whole decode
writes, and no byte outside the window's rows is written.  Expected bytes are the crop of the SOURCE raster, which the whole decode of
a second handle must reproduce (lossless containers), or of that decode (quanta, damaged or truncated streams), never of a window call.
Every destination lies in a sentinel-filled buffer with sentinel bytes before, between (wide strides) and behind it.
With the bit set a call must go path 1, end with status 0 and count the window's segments.
test_window_best_unit_plan.py shows on the CPU that the scaled, few and mixed rasters are coded QB3M_CF / QB3M_CF_H containers smaller
than their QB3M_BASE ones at every shape: those cases are never skipped.  Only a QB3M_BEST container whose mode byte says that the RLE0
pass won is, and every case checks that it decoded at least one container."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
import qb3_window16 as W16  # noqa: E402
import qb3_window_dev as D  # noqa: E402
import qb3_window_unit as WU  # noqa: E402
import qb3_window_best_unit as WBU  # noqa: E402

pytestmark = pytest.mark.gpu

CF, CF_H, BEST, FTL = WBU.CF, WBU.CF_H, WBU.BEST, WBU.FTL
BIT = WBU.QB3X_WINK_CFU
TSZ = WU.TSZ
_vp = C.c_void_p


def check_path1(qb3, dec, d_c, rows, Wd, Ht, pix, tsz, wins, k0=0):
    """every window with the bit set: path 1, status 0, the window's segments"""
    L = qb3.lib
    bps = D.segment_size(qb3, dec)
    dec.set_window_kernels(BIT)
    for i, win in enumerate(wins):
        D.window_call(qb3, dec, d_c, win, rows, pix, tsz, *D.destination("unit", k0 + i, tsz))
        assert L.qb3x_last_window_path(dec.p) == 1 and L.qb3x_last_decode_status(dec.p) == 0, win
        assert L.qb3x_last_window_segments(dec.p) == L.qb3x_window_segments(dec.p, *win, None) == W.brute_segments(Wd, Ht, *win, bps=bps), win


CASES = [(dt, b, si) for (dt, b) in WBU.MATRIX for si in range(4)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "t%d-b%d-s%d" % c)
def test_window_best_unit_kernel(qb3, case):
    """every (type, bands) of WBU.MATRIX x its four shapes; inside a case QB3M_CF and QB3M_CF_H (and QB3M_BEST for WBU.WITH_BEST) x the
    band maps of the band count (the default, the identity, [0, 0, 2, 2, 4] for five bands), each container taking the next of the
    rasters scaled, few, mixed, noisy and the next of the table levels 2, 1; windows of W16.windows over the segment size;
    destinations at every value offset 0..7 behind a dword with tight, wide-even and wide-odd rows"""
    import torch
    from qb3_amd import device as qdev
    dt, bands, si = case
    Wd, Ht = WU.shapes_of(dt, bands)[si]
    tsz, pix = TSZ[dt], TSZ[dt] * bands
    g = CASES.index(case)
    decoded = 0
    for mode in (CF, CF_H) + ((BEST,) if (dt, bands) in WBU.WITH_BEST else ()):
        for mi, cband in enumerate(WU.maps_of(bands)):
            name, level = WBU.NAMES[g % 4], 2 - (g // 4 + mi) % 2
            g += 1
            img = WBU.device_raster(name, Wd, Ht, bands, dt, 31 * bands + Wd)
            d_c, n, _ = D.make_container(qb3, img, dt, mode, level, cband)
            dec = qdev.DeviceDecoder(d_c, n)
            got_mode = qb3.lib.qb3_get_mode(dec.p)
            if (mode == BEST and got_mode == 7) or (name == "noisy" and got_mode == 255):      # the RLE0 pass won; noise that did not compress
                dec.close()
                continue
            assert got_mode == (CF_H if mode == BEST else mode), (name, mode, got_mode)
            bps = D.segment_size(qb3, dec)
            assert bps == WU.seg_blocks(bands)
            rows = D.as_rows(img, Ht)
            whole = D.full_decode(qb3, d_c, n)[0]
            assert whole is not None and torch.equal(whole.view(Ht, -1), rows)
            wins = W16.windows(Wd, Ht, 5 * Wd + bands + mode, bps, 12 if mi == 0 else 4)
            check_path1(qb3, dec, d_c, rows, Wd, Ht, pix, tsz, wins, g)
            decoded += 1
            dec.close()
    assert decoded >= 1, "every container of the case was skipped"


@pytest.mark.parametrize("case", ((WBU.U8, 5, 1001, 259, BEST, 2, "scaled"), (WBU.U16, 8, 132, 37, CF_H, 1, "mixed"), (WBU.I32, 1, 260, 37, CF, 2, "few")),
                         ids=lambda c: "t%d-b%d-%dx%d-m%d" % c[:5])
def test_window_best_unit_batch(qb3, case):
    """n = 1, 2 and 65 rectangles of one raster in one call, overlapping ones among them -- ONE launch of the kernel each -- and a
    mosaic laid out in one buffer; the host flavours (qb3x_read_windows, qb3x_read_window) on the int32 and the uint8 case"""
    import torch
    from qb3_amd import device as qdev
    L = qb3.lib
    dt, bands, Wd, Ht, mode, level, name = case
    tsz, pix = TSZ[dt], TSZ[dt] * bands
    img = WBU.device_raster(name, Wd, Ht, bands, dt, 77)
    rows = D.as_rows(img, Ht)
    d_c, n, _ = D.make_container(qb3, img, dt, mode, level)
    dec = qdev.DeviceDecoder(d_c, n)
    assert L.qb3_get_mode(dec.p) == (CF_H if mode == BEST else mode)
    bps = D.segment_size(qb3, dec)
    wins = W16.windows(Wd, Ht, 9, bps, 65)
    host = d_c[:n].cpu().numpy() if dt in (WBU.I32, WBU.U8) else None
    dec.set_window_kernels(BIT)
    for nwin in (1, 2, 65):
        rects = wins[5:5 + nwin] if nwin < 65 else wins[3:68]          # (random ones overlap each other and the fixed ones)
        lay = D.Layout(rects, pix, tsz, "unit")
        total = sum(W.brute_segments(Wd, Ht, *r, bps=bps) for r in rects)
        L.qb3x_profile_enable(1)
        L.qb3x_profile_reset()
        try:
            got, buf = D.batch_call(qb3, dec, d_c, lay)
            assert D.count(qb3, "dec_window_best_unit") == 1
        finally:
            L.qb3x_profile_enable(0)
        assert got == nwin, qb3.last_error()
        lay.check(buf, rows)
        assert all(L.qb3x_window_ok(dec.p, i) == 1 and L.qb3x_window_path(dec.p, i) == 1 for i in range(nwin))
        assert L.qb3x_last_window_segments(dec.p) == total and L.qb3x_last_decode_status(dec.p) == 0
        if host is not None and nwin != 2:
            p, _ = W.open_handle(L, host)
            L.qb3x_set_decoder_window_kernels(p, BIT)
            got, buf = D.batch_call(qb3, None, None, lay, host=p)
            assert got == nwin, qb3.last_error()
            lay.check(buf, rows)
            assert all(L.qb3x_window_path(p, i) == 1 for i in range(nwin)) and L.qb3x_last_window_segments(p) == total
            out = np.full(7 * 9 * pix + 8, D.SENTINEL, np.uint8)             # ... and the single host call
            assert L.qb3x_read_window(p, Wd - 9, Ht - 7, 9, 7, out.ctypes.data, 0) == 7 * 9 * pix and L.qb3x_last_window_path(p) == 1
            assert np.array_equal(out[:7 * 9 * pix].reshape(7, -1), rows[Ht - 7:, (Wd - 9) * pix:].cpu().numpy()) and (out[7 * 9 * pix:] == D.SENTINEL).all()
            L.qb3_destroy_decoder(p)
    # a mosaic: 3 x 2 tiles from six places of the raster, side by side in one image
    tw, th = min(40, Wd // 3), min(20, Ht // 2)
    rects = [((7 + 31 * i) % (Wd - tw), (5 + 13 * i) % (Ht - th), tw, th) for i in range(6)]
    lay = D.Layout(rects, pix, tsz, "unit", mosaic=(3 * tw * bands, [((i % 3) * tw * bands, (i // 3) * th) for i in range(6)], 2 * th))
    got, buf = D.batch_call(qb3, dec, d_c, lay)
    assert got == 6 and all(L.qb3x_window_path(dec.p, i) == 1 for i in range(6))
    mosaic = buf[16:16 + tsz * 3 * tw * bands * 2 * th].view(2 * th, -1)
    for i, (x0, y0, w, h) in enumerate(rects):
        assert torch.equal(mosaic[(i // 3) * th:(i // 3 + 1) * th, (i % 3) * tw * pix:(i % 3 + 1) * tw * pix], rows[y0:y0 + h, x0 * pix:(x0 + w) * pix]), i
    assert bool((buf[:16] == D.SENTINEL).all()) and bool((buf[16 + mosaic.numel():] == D.SENTINEL).all())
    dec.close()


@pytest.mark.parametrize("case", ((WBU.I8, 7, 201, 67, CF_H, 2, "mixed"), (WBU.U16, 1, 260, 37, CF, 1, "few"), (WBU.U64, 5, 1001, 259, CF_H, 2, "scaled")),
                         ids=lambda c: "t%d-b%d-%dx%d-m%d" % c[:5])
def test_the_bit_only_chooses_the_way(qb3, case):
    """the same windows on the same handle with the bit (path 1, the window's segments) and with the mask at 0 (path 2, the segments of
    the window's block rows): identical bytes, the source raster's"""
    from qb3_amd import device as qdev
    L = qb3.lib
    dt, bands, Wd, Ht, mode, level, name = case
    tsz, pix = TSZ[dt], TSZ[dt] * bands
    img = WBU.device_raster(name, Wd, Ht, bands, dt, 3)
    rows = D.as_rows(img, Ht)
    d_c, n, _ = D.make_container(qb3, img, dt, mode, level)
    dec = qdev.DeviceDecoder(d_c, n)
    assert L.qb3_get_mode(dec.p) == mode
    bps = D.segment_size(qb3, dec)
    for i, win in enumerate(W16.windows(Wd, Ht, 41, bps, 8)):
        dec.set_window_kernels(BIT)
        D.window_call(qb3, dec, d_c, win, rows, pix, tsz, *D.destination("unit", i, tsz))
        assert L.qb3x_last_window_path(dec.p) == 1 and L.qb3x_last_window_segments(dec.p) == W.brute_segments(Wd, Ht, *win, bps=bps), win
        dec.set_window_kernels(0)
        D.window_call(qb3, dec, d_c, win, rows, pix, tsz, *D.destination("unit", i, tsz))
        assert L.qb3x_last_window_path(dec.p) == 2 and L.qb3x_last_window_segments(dec.p) == W.row_segments(Wd, Ht, win[1], win[3], bps), win
    dec.close()


@pytest.mark.parametrize("case", ((WBU.U8, 5), (WBU.I32, 2)), ids=lambda c: "t%d-b%d" % c)
def test_window_best_unit_dequantises_the_window(qb3, case):
    """quanta 3 on a QB3M_CF_H container: path 1, then the WINDOW is multiplied back; expected: the second handle's whole decode, cropped"""
    import torch
    from qb3_amd import device as qdev
    dt, b = case
    Wd, Ht, tsz = 260, 37, TSZ[dt]
    img = WBU.device_raster("mixed", Wd, Ht, b, dt, 11)
    d_c, n, _ = D.make_container(qb3, img, dt, CF_H, 2, quanta=3)
    want = D.full_decode(qb3, d_c, n)[0]
    assert want is not None and not torch.equal(want, img.reshape(-1).view(torch.uint8))
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(BIT)
    for i, win in enumerate(W16.windows(Wd, Ht, 3, WU.seg_blocks(b), 8)):
        D.window_call(qb3, dec, d_c, win, want.view(Ht, -1), tsz * b, tsz, *D.destination("unit", i, tsz))
        assert qb3.lib.qb3x_last_window_path(dec.p) == 1
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- trust
@pytest.mark.parametrize("case", ((WBU.U8, 5), (WBU.U32, 1), (WBU.I64, 2)), ids=lambda c: "t%d-b%d" % c)
def test_damage_costs_time_not_pixels(qb3, case):
    """a flipped field bit under the old check (the chunk's check: status bit 5); a unit's length and a unit's entering rung changed
    under a RE-SEALED check (the kernel's own tests: where a unit ends, the rung the unit before leaves its band at); a stream cut
    inside the window's last segment and behind the window's segments: path 3 and the bytes of a second handle's whole decode of the
    same damaged container every time.  A shape whose sides are multiples of 4: no block repeats a neighbour's pixels"""
    import torch
    from qb3_amd import device as qdev
    L = qb3.lib
    dt, bands = case
    tsz, pix = TSZ[dt], TSZ[dt] * bands
    Wd, Ht = 1000, 260
    img = WBU.device_raster("mixed", Wd, Ht, bands, dt, 5)
    rows = D.as_rows(img, Ht)
    d_c, n, _ = D.make_container(qb3, img, dt, CF_H, 2)
    host = d_c[:n].cpu().numpy()
    chunks, data_off = D.table_chunks(host)
    E = WBU.entry_bytes(bands, tsz)
    dec = qdev.DeviceDecoder(d_c, n)
    assert L.qb3_get_mode(dec.p) == CF_H
    bps = D.segment_size(qb3, dec)
    nbx, nby = W.blocks_of(Wd, Ht)
    nseg = (nbx * nby + bps - 1) // bps
    assert L.qb3x_decoder_table_entries(dec.p) == nseg and sum(ln - 12 for _, ln in chunks) == nseg * E
    dec.close()
    per_chunk = (chunks[0][1] - 12) // E
    win = (40, 24, 300, 40)                                     # block rows 6..15, block columns 10..84
    first, last = (6 * nbx + 10) // bps, (15 * nbx + 84) // bps
    seg = first + 1
    lane = 2 * bands + bands - 1                                # the last band's unit of the segment's third block

    def entry_at(k):
        return chunks[k // per_chunk][0] + 12 + (k % per_chunk) * E

    def upload(a):
        t = torch.zeros_like(d_c)
        t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t

    def resealed(change):
        bad = host.copy()
        change(bad, entry_at(seg) + WBU.field_at(bands, tsz, lane))
        assert not np.array_equal(bad, host)
        c0, cl = chunks[seg // per_chunk]
        s16 = D.chunk_check(bad[c0 + 12:c0 + cl])
        bad[c0 + 6], bad[c0 + 7] = s16 & 255, s16 >> 8
        return upload(bad)

    def expect_path3(bad, size, what, bit=0, may_refuse=False):
        want = D.full_decode(qb3, bad, size)[0]
        assert want is not None or may_refuse, what
        dec = qdev.DeviceDecoder(bad, size)
        dec.set_window_kernels(BIT)
        D.window_call(qb3, dec, bad, win, None if want is None else want.view(Ht, -1), pix, tsz, *D.destination("unit", 3, tsz))
        if want is not None:
            assert L.qb3x_last_window_path(dec.p) == 3 and L.qb3x_last_decode_status(dec.p) & bit == bit, what
        dec.close()
        return want

    c0, cl = chunks[seg // per_chunk]
    assert D.chunk_check(host[c0 + 12:c0 + cl]) == int(host[c0 + 6]) | int(host[c0 + 7]) << 8      # (the formula is the encoder's)
    # the sound container first: path 1
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(BIT)
    D.window_call(qb3, dec, d_c, win, rows, pix, tsz, *D.destination("unit", 3, tsz))
    assert L.qb3x_last_window_path(dec.p) == 1
    dec.close()
    # a flipped bit in a field, the check left as it was
    bad = host.copy()
    bad[entry_at(seg) + WBU.field_at(bands, tsz, lane)] ^= 0x10
    want = expect_path3(upload(bad), n, "entry", bit=32)
    assert torch.equal(want.view(Ht, -1), rows)

    # re-sealed: only the kernel's own tests can tell
    def longer(b, at):                      # the unit's length + 1
        f = int(b[at]) | int(b[at + 1]) << 8
        f = (f & 0xf000) | ((f + 1) & 0xfff)
        b[at], b[at + 1] = f & 255, f >> 8

    def other_rung(b, at):                  # the unit entered one rung higher (the rung starts at bit 12 of the field)
        b[at + 1] = (int(b[at + 1]) & 0x0f) | (((int(b[at + 1]) >> 4) + 1) & 0xf) << 4

    for what, change in (("length", longer), ("rung", other_rung)):
        want = expect_path3(resealed(change), n, what)
        assert torch.equal(want.view(Ht, -1), rows), what
    # the stream ends in the middle of the window's last segment / behind the window's segments
    def pos_of(k):
        return int.from_bytes(bytes(host[entry_at(k):entry_at(k) + 6]), "little")

    assert last + 1 < nseg - 2
    for what, cut in (("cut inside", data_off + (pos_of(last) + pos_of(last + 1)) // 16), ("cut behind", data_off + pos_of(nseg - 2) // 8)):
        assert data_off + pos_of(last) // 8 < cut < n
        expect_path3(upload(host[:cut]), cut, what, may_refuse=True)      # (the same bytes as the whole decode, or its refusal)


def test_not_taken_with_the_bit_set(qb3, oracle):
    """what the bit does not change: with this bit alone an FTL raster of the same shape goes path 2 and 8-bit RGB in QB3M_CF_H goes
    path 2; an out-of-band index and a level-0 container (no table) go path 3; a container whose RLE0 pass won goes its usual path 3;
    a destination off the value size goes path 2, with the right bytes (the int64 raster is the scaled one, whose segments are of one
    length: path 2 stages for the stream's average segment and leaves a stream with longer ones to path 3); the kernel is counted only
    where it is taken"""
    import torch
    from qb3_amd import device as qdev
    L = qb3.lib
    win = (13, 9, 101, 21)

    def one(img, dt, mode, level, path, want_index=False, addr=None, mode_byte=None):
        d_c, n, index = D.make_container(qb3, img, dt, mode, level, want_index=want_index)
        dec = qdev.DeviceDecoder(d_c, n)
        assert L.qb3_get_mode(dec.p) == (mode if mode_byte is None else mode_byte)
        dec.set_window_kernels(BIT)
        D.window_call(qb3, dec, d_c, win, D.as_rows(img, img.shape[0]), TSZ[dt] * img.shape[2], TSZ[dt], *D.destination("unit", 0, TSZ[dt], addr), index)
        assert L.qb3x_last_window_path(dec.p) == path, (dt, mode, level, addr)
        dec.close()

    L.qb3x_profile_enable(1)
    L.qb3x_profile_reset()
    try:
        one(WBU.device_raster("noisy", 260, 37, 5, WBU.U8, 1), WBU.U8, FTL, 2, 2)
        one(WBU.device_raster("mixed", 260, 37, 3, WBU.U8, 1), WBU.U8, CF_H, 2, 2)
        one(WBU.device_raster("mixed", 260, 37, 5, WBU.U8, 1), WBU.U8, CF_H, 2, 3, want_index=True)
        one(WBU.device_raster("mixed", 260, 37, 5, WBU.U8, 1), WBU.U8, CF_H, 0, 3)
        one(torch.from_numpy(oracle.generate(260, 37, 5, 0, "CONST", 1)).cuda(), WBU.U8, BEST, 2, 3, mode_byte=7)
        one(WBU.device_raster("mixed", 260, 37, 2, WBU.I16, 1), WBU.I16, CF_H, 2, 2, addr=17)
        one(WBU.device_raster("scaled", 260, 37, 2, WBU.I64, 1), WBU.I64, CF, 2, 2, addr=20)
        assert D.count(qb3, "dec_window_best_unit") == 0
        one(WBU.device_raster("mixed", 260, 37, 5, WBU.U8, 1), WBU.U8, CF_H, 2, 1)
        one(WBU.device_raster("mixed", 260, 37, 2, WBU.I16, 1), WBU.I16, CF_H, 2, 1, addr=18)
        one(WBU.device_raster("scaled", 260, 37, 2, WBU.I64, 1), WBU.I64, CF, 2, 1, addr=24)
        assert D.count(qb3, "dec_window_best_unit") == 3
    finally:
        L.qb3x_profile_enable(0)


def test_a_ranged_handle_reads_the_container_whole_and_takes_the_kernel(qb3):
    """the bit adds no ranged shortcut: uint16 x 3 in QB3M_CF_H on a handle of open_ranged is read whole, once (qb3x_ranged_bytes = the
    container's size), after which its windows take path 1 from the uploaded container; bytes: the crop of the source raster"""
    import qb3_amd
    Wd, Ht, b = 201, 67, 3
    img = WBU.device_raster("mixed", Wd, Ht, b, WBU.U16, 3)
    d_c, n, _ = D.make_container(qb3, img, WBU.U16, CF_H, 2)
    host = d_c[:n].cpu().numpy()
    src = WBU.raster("mixed", Wd, Ht, b, WBU.U16, 3)
    rects = W16.windows(Wd, Ht, 17, WU.seg_blocks(b), 6)
    with qb3_amd.open_ranged(lambda off, size: host[off:off + size].tobytes(), size=n, window_kernels=BIT) as rd:
        outs = rd.read_windows(rects)
        assert rd.last_bytes == n and rd.last_windows == [1] * len(rects)
        for (x0, y0, w, h), o in zip(rects, outs):
            assert np.array_equal(o, src[y0:y0 + h, x0:x0 + w]), (x0, y0, w, h)


def test_python_decode_window(qb3):
    """DeviceDecoder.set_window_kernels(QB3X_WINK_CFU) with decode_window and decode_windows"""
    import torch
    from qb3_amd import device as qdev
    Wd, Ht, b = 260, 37, 2
    img = WBU.device_raster("few", Wd, Ht, b, WBU.I32, 2)
    d_c, n, _ = D.make_container(qb3, img, WBU.I32, CF_H, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(qb3.QB3X_WINK_CFU)
    one = dec.decode_window(d_c, 33, 5, 100, 20)
    assert torch.equal(one, img[5:25, 33:133]) and qb3.lib.qb3x_last_window_path(dec.p) == 1
    rects = W16.windows(Wd, Ht, 4, 32, 5)
    many = dec.decode_windows(d_c, rects)
    assert all(torch.equal(t, img[y0:y0 + h, x0:x0 + w]) for t, (x0, y0, w, h) in zip(many, rects))
    assert all(qb3.lib.qb3x_window_path(dec.p, i) == 1 for i in range(len(rects)))
    dec.close()
