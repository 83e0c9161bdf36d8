"""The window kernels of the lane-per-unit and one-band 32/64-bit rasters on the device (include/qb3x.h:
qb3x_set_decoder_window_kernels, QB3X_WINK_UNIT; k_dec_win_unit.hip).  The invariant is the window calls': a window is the crop of what
the whole decode writes, and no byte outside the window's rows is written.  Expected bytes are the crop of the SOURCE raster (lossless
containers) or of qb3x_decode_device on a second handle (quanta, damaged or truncated streams), never of a window call.  Every
destination lies in a sentinel-filled buffer with sentinel bytes before, between (wide strides) and behind it.
With the bit set a call must go path 1, end with status 0 and count the window's segments; the same handle with the mask back at 0
must give the same bytes by path 2 and count the segments of the window's block rows.
Which value decoder a unit takes -- the code table below rung 8, the code rule from there -- follows from the generators:
test_window_unit_plan.py restates the rungs of their rasters on the CPU.  RANDOM rasters do not compress and come out STORED: those
containers are skipped, and every case checks that it decoded at least one."""
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

pytestmark = pytest.mark.gpu

FTL, BASE, BASE_Z, CF_H = WU.FTL, WU.BASE, WU.BASE_Z, WU.CF_H
BIT = WU.QB3X_WINK_UNIT
TSZ = WU.TSZ
_vp = C.c_void_p


def check_windows(qb3, dec, d_c, rows, Wd, Ht, pix, tsz, wins, k0=0):
    """every window with the bit set (path 1, status 0, the window's segments) and with the mask back at 0 (path 2, the rows')"""
    L = qb3.lib
    bps = D.segment_size(qb3, dec)
    for i, win in enumerate(wins):
        dec.set_window_kernels(BIT)
        D.window_call(qb3, dec, d_c, win, rows, pix, tsz, *D.destination("unit", k0 + i, tsz))
        assert L.qb3x_last_window_path(dec.p) == 1 and L.qb3x_last_decode_status(dec.p) == 0, win
        assert L.qb3x_last_window_segments(dec.p) == L.qb3x_window_segments(dec.p, *win, None) == W.brute_segments(Wd, Ht, *win, bps=bps), win
        dec.set_window_kernels(0)
        D.window_call(qb3, dec, d_c, win, rows, pix, tsz, *D.destination("unit", k0 + i, tsz))
        assert L.qb3x_last_window_path(dec.p) == 2, win
        assert L.qb3x_last_window_segments(dec.p) == W.row_segments(Wd, Ht, win[1], win[3], bps), win


CASES = [(dt, b, si) for (dt, b) in WU.MATRIX for si in range(4)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "t%d-b%d-s%d" % c)
def test_window_unit_kernel(qb3, case):
    """every (type, bands) of WU.MATRIX x its four shapes; inside a case FTL, BASE, BASE_Z x the band maps of the band count (the
    default, the identity, [0, 0, 2, 2, 4] for five bands), each container taking the next of NOISY3, DEM, RANDOM; windows of
    W16.windows; destinations at every value offset 0..7 behind a dword with tight, wide-even and wide-odd rows.  The case with the
    (1001, 259) raster of uint8 x 5 must read its entries from more than one table chunk"""
    from qb3_amd import device as qdev, synth
    dt, bands, si = case
    Wd, Ht = WU.shapes_of(dt, bands)[si]
    tsz, pix = TSZ[dt], TSZ[dt] * bands
    g = CASES.index(case)
    decoded = 0
    for mode in (FTL, BASE, BASE_Z):
        for mi, cband in enumerate(WU.maps_of(bands)):
            gen = WU.GENERATORS[g % 3]
            g += 1
            img = synth.generate(Wd, Ht, bands, dt, gen, 31 * bands + Wd)
            d_c, n, _ = D.make_container(qb3, img, dt, mode, 2, cband)
            dec = qdev.DeviceDecoder(d_c, n)
            if qb3.lib.qb3_get_mode(dec.p) == 255:          # STORED: the raster did not compress
                dec.close()
                continue
            assert qb3.lib.qb3_get_mode(dec.p) == mode
            bps = D.segment_size(qb3, dec)
            assert bps == WU.seg_blocks(bands)
            wins = W16.windows(Wd, Ht, 5 * Wd + bands + mode, bps, 24 if mi == 0 else 8)
            if (dt, bands, Wd) == (WU.U8, 5, 1001):         # the whole raster (wins[0]): its first and last segment lie in different chunks
                chunks, _ = D.table_chunks(d_c[:n].cpu().numpy())
                E = WU.entry_bytes(bands, tsz)
                nseg = W.brute_segments(Wd, Ht, 0, 0, Wd, Ht, bps=bps)
                assert len(chunks) >= 2 and sum(ln - 12 for _, ln in chunks) == nseg * E and wins[0] == (0, 0, Wd, Ht)
                assert (nseg - 1) // ((chunks[0][1] - 12) // E) >= 1
            check_windows(qb3, dec, d_c, D.as_rows(img, Ht), Wd, Ht, pix, tsz, wins, g)
            decoded += 1
            dec.close()
    assert decoded >= 1, "every container of the case came out STORED"


@pytest.mark.parametrize("case", ((WU.U8, 5, 1001, 259, BASE, "DEM"), (WU.I16, 7, 1001, 259, FTL, "DEM"), (WU.I32, 1, 260, 37, BASE_Z, "DEM"),
                                  (WU.U64, 2, 132, 37, FTL, "NOISY3")), ids=lambda c: "t%d-b%d-%dx%d-m%d" % c[:5])
def test_window_unit_batch(qb3, case):
    """n = 1, 2 and 65 rectangles of one raster in one call, overlapping ones among them, and a mosaic laid out in one buffer; the
    host flavours (qb3x_read_windows, qb3x_read_window) on the int32 and the uint8 case"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    dt, bands, Wd, Ht, mode, gen = case
    tsz, pix = TSZ[dt], TSZ[dt] * bands
    img = synth.generate(Wd, Ht, bands, dt, gen, 77)
    rows = D.as_rows(img, Ht)
    d_c, n, _ = D.make_container(qb3, img, dt, mode, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    assert L.qb3_get_mode(dec.p) == mode
    bps = D.segment_size(qb3, dec)
    wins = W16.windows(Wd, Ht, 9, bps, 65)
    host = d_c[:n].cpu().numpy() if dt in (WU.I32, WU.U8) else None
    for nwin in (1, 2, 65):
        rects = wins[5:5 + nwin] if nwin < 65 else wins[3:68]          # (random ones overlap each other and the fixed ones)
        lay = D.Layout(rects, pix, tsz, "unit")
        total = sum(W.brute_segments(Wd, Ht, *r, bps=bps) for r in rects)
        dec.set_window_kernels(BIT)
        got, buf = D.batch_call(qb3, dec, d_c, lay)
        assert got == nwin, qb3.last_error()
        lay.check(buf, rows)
        assert all(L.qb3x_window_ok(dec.p, i) == 1 and L.qb3x_window_path(dec.p, i) == 1 for i in range(nwin))
        assert L.qb3x_last_window_segments(dec.p) == total and L.qb3x_last_decode_status(dec.p) == 0
        dec.set_window_kernels(0)
        got, buf = D.batch_call(qb3, dec, d_c, lay)
        assert got == nwin
        lay.check(buf, rows)
        assert all(L.qb3x_window_path(dec.p, i) == 2 for i in range(nwin))
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
    # a mosaic: 3 x 2 tiles of 40 x 20 pixels from six places of the raster, side by side in one image of 120 x 40 pixels
    tw, th = min(40, Wd // 3), min(20, Ht // 2)
    rects = [((7 + 31 * i) % (Wd - tw), (5 + 13 * i) % (Ht - th), tw, th) for i in range(6)]
    lay = D.Layout(rects, pix, tsz, "unit", mosaic=(3 * tw * bands, [((i % 3) * tw * bands, (i // 3) * th) for i in range(6)], 2 * th))
    dec.set_window_kernels(BIT)
    got, buf = D.batch_call(qb3, dec, d_c, lay)
    assert got == 6 and all(L.qb3x_window_path(dec.p, i) == 1 for i in range(6))
    mosaic = buf[16:16 + tsz * 3 * tw * bands * 2 * th].view(2 * th, -1)
    for i, (x0, y0, w, h) in enumerate(rects):
        assert torch.equal(mosaic[(i // 3) * th:(i // 3 + 1) * th, (i % 3) * tw * pix:(i % 3 + 1) * tw * pix], rows[y0:y0 + h, x0 * pix:(x0 + w) * pix]), i
    assert bool((buf[:16] == D.SENTINEL).all()) and bool((buf[16 + mosaic.numel():] == D.SENTINEL).all())
    dec.close()


@pytest.mark.parametrize("case", ((WU.U8, 5), (WU.I32, 1)), ids=lambda c: "t%d-b%d" % c)
def test_window_unit_dequantises_the_window(qb3, case):
    """quanta 3 on a BASE container: path 1, then the WINDOW is multiplied back; expected: the second handle's whole decode, cropped"""
    import torch
    from qb3_amd import device as qdev, synth
    dt, b = case
    Wd, Ht, tsz = 260, 37, TSZ[dt]
    img = synth.generate(Wd, Ht, b, dt, "NOISY3", 11)
    d_c, n, _ = D.make_container(qb3, img, dt, BASE, 2, quanta=3)
    want = D.full_decode(qb3, d_c, n)[0]
    assert want is not None and not torch.equal(want, img.reshape(-1).view(torch.uint8))
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(BIT)
    for i, win in enumerate(W16.windows(Wd, Ht, 3, WU.seg_blocks(b), 8)):
        D.window_call(qb3, dec, d_c, win, want.view(Ht, -1), tsz * b, tsz, *D.destination("unit", i, tsz))
        assert qb3.lib.qb3x_last_window_path(dec.p) == 1
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- trust
@pytest.mark.parametrize("case", ((WU.U8, 5), (WU.I32, 1), (WU.U64, 2)), ids=lambda c: "t%d-b%d" % c)
def test_damaged_tables_and_short_streams_cost_time_not_pixels(qb3, case):
    """a flipped entry byte (the chunk's check), one lane's twelve-bit length + 1 under a re-sealed check (the kernel's own test of
    where a unit ends), a stream cut inside the window's last segment and one cut behind the window's segments (the table's end):
    path 3 and the whole decode's bytes every time -- or, where the whole decode refuses the stream, a refused window.  The bytes are
    changed on the host and uploaded; every damaged container is decoded once"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    dt, bands = case
    tsz, pix = TSZ[dt], TSZ[dt] * bands
    Wd, Ht = 1001, 259
    img = synth.generate(Wd, Ht, bands, dt, "DEM", 5)
    rows = D.as_rows(img, Ht)
    d_c, n, _ = D.make_container(qb3, img, dt, FTL, 2)
    host = d_c[:n].cpu().numpy()
    chunks, data_off = D.table_chunks(host)
    E = WU.entry_bytes(bands, tsz)
    dec = qdev.DeviceDecoder(d_c, n)
    bps = D.segment_size(qb3, dec)
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

    def upload(a):
        t = torch.zeros_like(d_c)
        t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t

    def expect_path3(bad, size, what):
        want = D.full_decode(qb3, bad, size)[0]
        dec = qdev.DeviceDecoder(bad, size)
        dec.set_window_kernels(BIT)
        D.window_call(qb3, dec, bad, win, None if want is None else want.view(Ht, -1), pix, tsz, *D.destination("unit", 3, tsz))
        if want is not None:
            assert L.qb3x_last_window_path(dec.p) == 3, what
        dec.close()
        return want

    # the sound container first: path 1
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(BIT)
    D.window_call(qb3, dec, d_c, win, rows, pix, tsz, *D.destination("unit", 3, tsz))
    assert L.qb3x_last_window_path(dec.p) == 1
    dec.close()
    e0 = entry_at(seg)
    bad = host.copy()
    bad[e0 + 7] ^= 0x10
    want = expect_path3(upload(bad), n, "entry")
    assert want is not None and torch.equal(want.view(Ht, -1), rows)
    # lane 5's length field + 1, the chunk's check sealed again: only the kernel's own test can tell
    bad = host.copy()
    fields = e0 + 6 + bands * (1 + tsz)
    nf = E - 6 - bands * (1 + tsz)
    v = int.from_bytes(bytes(bad[fields:fields + nf]), "little")
    bit = 12 * 5
    f = (v >> bit) & 4095
    v = (v & ~(4095 << bit)) | (((f + 1) & 4095) << bit)
    bad[fields:fields + nf] = np.frombuffer(v.to_bytes(nf, "little"), np.uint8)
    c0, cl = chunks[seg // per_chunk]
    s16 = D.chunk_check(bad[c0 + 12:c0 + cl])
    assert D.chunk_check(host[c0 + 12:c0 + cl]) == int(host[c0 + 6]) | int(host[c0 + 7]) << 8      # (the formula is the encoder's)
    bad[c0 + 6], bad[c0 + 7] = s16 & 255, s16 >> 8
    want = expect_path3(upload(bad), n, "lengths")
    assert want is not None and torch.equal(want.view(Ht, -1), rows)
    # the stream ends in the middle of the window's last segment / behind the window's segments
    pos_last = int.from_bytes(bytes(host[entry_at(last):entry_at(last) + 6]), "little")
    pos_next = int.from_bytes(bytes(host[entry_at(last + 1):entry_at(last + 1) + 6]), "little")
    pos_far = int.from_bytes(bytes(host[entry_at(nseg - 2):entry_at(nseg - 2) + 6]), "little")
    for what, cut in (("cut inside", data_off + (pos_last + pos_next) // 16), ("cut behind", data_off + pos_far // 8)):
        assert data_off + pos_last // 8 < cut < n
        expect_path3(upload(host[:cut]), cut, what)


def test_not_taken_with_the_bit_set(qb3):
    """what the bit does not change: 8-bit RGB still goes through the old kernel (dec_window counted, dec_window_unit not); uint16 x 4
    goes path 2 with this bit alone, uint16 x 5 in QB3M_CF_H goes path 2; a level-1 table and an out-of-band index go path 3; a
    destination on an odd address (16-bit raster) or on address % 8 == 4 (64-bit raster) goes path 2, with the right bytes"""
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    win = (13, 9, 101, 21)

    def one(img, dt, mode, level, path, want_index=False, addr=None):
        d_c, n, index = D.make_container(qb3, img, dt, mode, level, want_index=want_index)
        dec = qdev.DeviceDecoder(d_c, n)
        dec.set_window_kernels(BIT)
        D.window_call(qb3, dec, d_c, win, D.as_rows(img, img.shape[0]), TSZ[dt] * img.shape[2], TSZ[dt], *D.destination("unit", 0, TSZ[dt], addr), index)
        assert L.qb3x_last_window_path(dec.p) == path, (dt, mode, level, addr)
        dec.close()

    L.qb3x_profile_enable(1)
    L.qb3x_profile_reset()
    try:
        one(synth.generate(260, 37, 3, WU.U8, "NOISY3", 1), WU.U8, FTL, 2, 1)
        assert D.count(qb3, "dec_window") == 1 and D.count(qb3, "dec_window_unit") == 0
        one(synth.generate(260, 37, 5, WU.U8, "NOISY3", 1), WU.U8, FTL, 2, 1)
        assert D.count(qb3, "dec_window") == 1 and D.count(qb3, "dec_window_unit") == 1
    finally:
        L.qb3x_profile_enable(0)
    one(synth.generate(260, 37, 4, WU.U16, "LANDSAT16", 1), WU.U16, FTL, 2, 2)
    one(synth.generate(260, 37, 5, WU.U16, "LANDSAT16", 1), WU.U16, CF_H, 2, 2)
    one(synth.generate(260, 37, 5, WU.U8, "NOISY3", 1), WU.U8, FTL, 1, 3)
    one(synth.generate(260, 37, 5, WU.U8, "NOISY3", 1), WU.U8, FTL, 2, 3, want_index=True)
    one(synth.generate(260, 37, 5, WU.U16, "LANDSAT16", 1), WU.U16, FTL, 2, 1, addr=18)
    one(synth.generate(260, 37, 5, WU.U16, "LANDSAT16", 1), WU.U16, FTL, 2, 2, addr=17)
    one(synth.generate(260, 37, 2, WU.I64, "DEM", 1), WU.I64, FTL, 2, 1, addr=24)
    one(synth.generate(260, 37, 2, WU.I64, "DEM", 1), WU.I64, FTL, 2, 2, addr=20)


def test_a_ranged_handle_reads_the_container_whole_and_takes_the_kernel(qb3):
    """the bit adds no ranged shortcut: uint8 x 5 on a handle of open_ranged is read whole, once (qb3x_ranged_bytes = the container's
    size), after which its windows take path 1 from the uploaded container; bytes: the crop of the source raster"""
    import qb3_amd
    from qb3_amd import synth
    Wd, Ht, b = 201, 67, 5
    img = synth.generate(Wd, Ht, b, WU.U8, "NOISY3", 3)
    d_c, n, _ = D.make_container(qb3, img, WU.U8, BASE, 2)
    host = d_c[:n].cpu().numpy()
    src = img.cpu().numpy()
    rects = W16.windows(Wd, Ht, 17, WU.seg_blocks(b), 6)
    with qb3_amd.open_ranged(lambda off, size: host[off:off + size].tobytes(), size=n, window_kernels=BIT) as rd:
        outs = rd.read_windows(rects)
        assert rd.last_bytes == n and rd.last_windows == [1] * len(rects)
        for (x0, y0, w, h), o in zip(rects, outs):
            assert np.array_equal(o, src[y0:y0 + h, x0:x0 + w]), (x0, y0, w, h)
