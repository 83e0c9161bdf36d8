"""Band-selected windows on the device (include/qb3x.h: qb3x_decode_windows_bands_device, qb3x_read_windows_bands).  The invariant:
value k of a window's pixel is band sel[k] of that pixel of the whole decode, and no byte outside the window's h runs of w * nsel values
is written.  Expected bytes are the SOURCE raster with the bands picked (WB.select) -- for lossy or damaged containers
qb3x_decode_device on a second handle -- never a window call's.  Every destination lies in a sentinel-filled buffer (WB.Layout: windows
at every value offset 0..7 behind a dword, rows tight, wide-even and wide-odd).
qb3x_last_window_gathers tells the two routes apart: 0 where the lane-per-unit window kernels wrote the selection themselves (the fused
route), 1 where full-band pixels were produced first and one launch of the gather picked the bands.
RANDOM rasters do not compress and come out STORED: those containers are skipped, and every case checks that it decoded at least one."""
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
import qb3_window_best as WBEST  # noqa: E402
import qb3_window_best_unit as WBU  # noqa: E402
import qb3_window_bands as WB  # noqa: E402

pytestmark = pytest.mark.gpu

FTL, BASE, BASE_Z, CF_H, BEST = WU.FTL, WU.BASE, WU.BASE_Z, WU.CF_H, WBU.BEST
UNIT, CFU, U16BIT, CF8 = WU.QB3X_WINK_UNIT, WBU.QB3X_WINK_CFU, WU.QB3X_WINK_U16, WU.QB3X_WINK_CF8
TSZ = WU.TSZ
_vp = C.c_void_p


def shapes_of(dt, bands):
    s = WU.shapes_of(dt, bands)
    return (s[0], s[2], (201, 67))


def call_and_check(qb3, dec, d_c, rows, bands, tsz, rects, sel, path, gathers, segs=None, shift=0, index=None, mosaic=None):
    """one band-selected call into a fresh sentinel buffer: every window written by `path` (a list: per window), the gather launches,
    the segments (None: not asserted), the bytes and the sentinels"""
    L = qb3.lib
    lay = WB.Layout(rects, len(sel), tsz, mosaic=mosaic, shift=shift)
    got, buf = WB.bands_call(qb3, dec, d_c, lay, sel, index=index)
    assert got == len(rects), qb3.last_error()
    paths = path if isinstance(path, list) else [path] * len(rects)
    assert [L.qb3x_window_path(dec.p, i) for i in range(len(rects))] == paths and all(L.qb3x_window_ok(dec.p, i) == 1 for i in range(len(rects)))
    assert L.qb3x_last_window_path(dec.p) == paths[-1]
    assert L.qb3x_last_window_gathers(dec.p) == gathers, (L.qb3x_last_window_gathers(dec.p), gathers)
    if segs is not None:
        assert L.qb3x_last_window_segments(dec.p) == segs
    if mosaic is None:
        lay.check(buf, WB.select(rows, bands, tsz, sel))
    return lay, buf


# ---------------------------------------------------------------------------------------------------------------- 1. fused, FTL / BASE
FUSED = ((WU.U8, 5), (WU.I8, 7), (WU.U8, 16), (WU.I16, 7), (WU.U16, 9), (WU.I32, 2), (WU.U32, 3), (WU.U64, 5))
FUSED_CASES = [(dt, b, si) for (dt, b) in FUSED for si in range(3)]


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "t%d-b%d-s%d" % c)
def test_fused_route_unit(qb3, case):
    """QB3X_WINK_UNIT: FTL, BASE, BASE_Z x the default and the identity band map x WB.selections: path 1, status 0, no gather, the
    windows' segments"""
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    dt, bands, si = case
    Wd, Ht = shapes_of(dt, bands)[si]
    tsz = TSZ[dt]
    g = FUSED_CASES.index(case)
    decoded = 0
    for mode in (FTL, BASE, BASE_Z):
        for cband in (None, list(range(bands))) if bands >= 3 else (None,):
            gen = WU.GENERATORS[g % 3]
            g += 1
            img = synth.generate(Wd, Ht, bands, dt, gen, 31 * bands + Wd)
            d_c, n, _ = D.make_container(qb3, img, dt, mode, 2, cband)
            dec = qdev.DeviceDecoder(d_c, n)
            if L.qb3_get_mode(dec.p) == 255:
                dec.close()
                continue
            dec.set_window_kernels(UNIT)
            bps = D.segment_size(qb3, dec)
            assert bps == WU.seg_blocks(bands)
            rects = W16.windows(Wd, Ht, 5 * Wd + bands + mode, bps, 1)
            assert 8 <= len(rects) <= 12
            total = sum(W.brute_segments(Wd, Ht, *r, bps=bps) for r in rects)
            rows = D.as_rows(img, Ht)
            for sel in WB.selections(bands):
                call_and_check(qb3, dec, d_c, rows, bands, tsz, rects, sel, 1, 0, segs=total)
                assert L.qb3x_last_decode_status(dec.p) == 0
            decoded += 1
            dec.close()
    assert decoded >= 1, "every container of the case came out STORED"


# ---------------------------------------------------------------------------------------------------------------- 2. fused, common factor
@pytest.mark.parametrize("case", ((WBU.U16, 2), (WBU.U8, 5), (WBU.I64, 2)), ids=lambda c: "t%d-b%d" % c)
def test_fused_route_common_factor(qb3, case):
    """QB3X_WINK_CFU, QB3M_CF_H and QB3M_BEST, the rasters of qb3_window_best_unit: the same assertions.  A QB3M_BEST container whose RLE0
    pass won is no common-factor stream (as in test_window_best_unit_decode.py): skipped, and at least one of each mode must be left"""
    from qb3_amd import device as qdev
    L = qb3.lib
    dt, bands = case
    tsz = TSZ[dt]
    decoded, k = {CF_H: 0, BEST: 0}, 0
    for (Wd, Ht) in shapes_of(dt, bands):
        for mode in (CF_H, BEST):
            name = WBU.SIGNAL[k % 3]
            k += 1
            img = WBU.device_raster(name, Wd, Ht, bands, dt, 31 * bands + Wd)
            d_c, n, _ = D.make_container(qb3, img, dt, mode, 2)
            dec = qdev.DeviceDecoder(d_c, n)
            if L.qb3_get_mode(dec.p) == 255 or (mode == BEST and L.qb3_get_mode(dec.p) == 7):
                dec.close()
                continue
            assert L.qb3_get_mode(dec.p) == CF_H
            dec.set_window_kernels(CFU)
            bps = D.segment_size(qb3, dec)
            rects = W16.windows(Wd, Ht, 5 * Wd + bands + mode, bps, 1)
            total = sum(W.brute_segments(Wd, Ht, *r, bps=bps) for r in rects)
            rows = D.as_rows(img, Ht)
            for sel in WB.selections(bands):
                call_and_check(qb3, dec, d_c, rows, bands, tsz, rects, sel, 1, 0, segs=total)
                assert L.qb3x_last_decode_status(dec.p) == 0
            decoded[mode] += 1
            dec.close()
    assert decoded[CF_H] >= 1 and decoded[BEST] >= 1, "every container of a mode was skipped"


# ---------------------------------------------------------------------------------------------------------------- 3. gather, path 1
def _synth(gen):
    def make(Wd, Ht, b, dt):
        from qb3_amd import synth
        return synth.generate(Wd, Ht, b, dt, gen, 7)
    return make


def _mixed(Wd, Ht, b, dt):
    import torch
    return torch.from_numpy(WBEST.mixed(Wd, Ht, b, 7)).cuda()     # (the 8-bit patchwork that QB3M_BEST codes as QB3M_CF_H)


# name: type, bands, raster, mode, the handle's switches, selections, byte shift of every destination
GATHER1 = {
    "u8-rgb": (WU.U8, 3, _synth("NOISY3"), FTL, 0, ([2, 1, 0], [1]), 0),
    "u8-rgba": (WU.U8, 4, _synth("NOISY3"), BASE, 0, ([0, 1, 2],), 0),
    "u16x8": (WU.U16, 8, _synth("LANDSAT16"), FTL, U16BIT, ([3, 2, 1],), 0),
    "u8-rgb-best": (WU.U8, 3, _mixed, BEST, CF8, ([0],), 0),
    "u8x2-five-slots": (WU.U8, 2, _synth("NOISY3"), FTL, UNIT, ([1, 0, 1, 1, 0],), 0),         # 32 blocks a segment x 5 slots > 64
    "i16x7-odd-address": (WU.I16, 7, _synth("DEM"), FTL, UNIT, ([6, 0, 3],), 1),
}


@pytest.mark.parametrize("name", list(GATHER1), ids=list(GATHER1))
def test_gather_route_on_path_1(qb3, name):
    """the lane-per-block families, a selection too wide for the wave's tile, destinations off value alignment: the family's kernel
    writes full-band windows into the handle's memory, ONE gather launch picks the bands"""
    from qb3_amd import device as qdev
    L = qb3.lib
    dt, bands, make, mode, bits, sels, shift = GATHER1[name]
    tsz = TSZ[dt]
    for (Wd, Ht) in ((260, 37), (201, 67)):
        img = make(Wd, Ht, bands, dt)
        d_c, n, _ = D.make_container(qb3, img, dt, mode, 2)
        dec = qdev.DeviceDecoder(d_c, n)
        assert L.qb3_get_mode(dec.p) != 255
        dec.set_window_kernels(bits)
        bps = D.segment_size(qb3, dec)
        rects = W16.windows(Wd, Ht, Wd + bands, bps, 1)
        total = sum(W.brute_segments(Wd, Ht, *r, bps=bps) for r in rects)
        rows = D.as_rows(img, Ht)
        for sel in sels:
            call_and_check(qb3, dec, d_c, rows, bands, tsz, rects, sel, 1, 1, segs=total, shift=shift)
            assert L.qb3x_last_decode_status(dec.p) == 0
        dec.close()


# ---------------------------------------------------------------------------------------------------------------- 4. gather, paths 2 and 3
def test_gather_route_on_paths_2_and_3(qb3):
    """int16 x 7: the mask at 0 (strips into the scratch raster), a level-1 table and an out-of-band index (the whole decode)"""
    from qb3_amd import device as qdev, synth
    dt, bands, Wd, Ht = WU.I16, 7, 201, 67
    tsz = TSZ[dt]
    img = synth.generate(Wd, Ht, bands, dt, "DEM", 3)
    rows = D.as_rows(img, Ht)
    rects = W16.windows(Wd, Ht, 11, WU.seg_blocks(bands), 1)
    for level, want_index, path in ((2, False, 2), (1, False, 3), (2, True, 3)):
        d_c, n, index = D.make_container(qb3, img, dt, FTL, level, want_index=want_index)
        dec = qdev.DeviceDecoder(d_c, n)
        dec.set_window_kernels(UNIT if path == 3 else 0)
        for k, sel in enumerate(([5], [6, 3, 0], [2, 2, 4, 2, 1, 0, 6, 5, 3])):
            call_and_check(qb3, dec, d_c, rows, bands, tsz, rects, sel, path, 1, index=index, shift=k % 2)
        dec.close()


# ---------------------------------------------------------------------------------------------------------------- 5. batch
@pytest.mark.parametrize("case", ((WU.U8, 5, UNIT, [3, 2, 1], 0), (WU.U8, 3, 0, [2, 0], 1)), ids=("u8x5-fused", "u8-rgb-gathered"))
def test_batches_and_a_mosaic(qb3, case):
    """n = 1, 2 and 65 overlapping rectangles and a mosaic of six tiles in one buffer; 65 fused windows count the sum of their
    segments; the host call (qb3x_read_windows_bands) on the uint8 x 5 raster"""
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    dt, bands, bits, sel, gathers = case
    Wd, Ht, tsz, nsel = 201, 67, TSZ[dt], len(sel)
    img = synth.generate(Wd, Ht, bands, dt, "NOISY3", 77)
    rows = D.as_rows(img, Ht)
    want = WB.select(rows, bands, tsz, sel)
    d_c, n, _ = D.make_container(qb3, img, dt, BASE, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(bits)
    bps = D.segment_size(qb3, dec)
    wins = W16.windows(Wd, Ht, 9, bps, 65)
    host = d_c[:n].cpu().numpy()
    for nwin in (1, 2, 65):
        rects = wins[5:5 + nwin] if nwin < 65 else wins[3:68]
        total = sum(W.brute_segments(Wd, Ht, *r, bps=bps) for r in rects)
        lay, _ = call_and_check(qb3, dec, d_c, rows, bands, tsz, rects, sel, 1, gathers, segs=total)
        if bands == 5 and nwin != 2:
            p, _ = W.open_handle(L, host)
            L.qb3x_set_decoder_window_kernels(p, bits)
            got, buf = WB.bands_call(qb3, None, None, lay, sel, host=p)
            assert got == nwin, qb3.last_error()
            lay.check(buf, want)
            assert all(L.qb3x_window_path(p, i) == 1 for i in range(nwin)) and L.qb3x_last_window_segments(p) == total
            assert L.qb3x_last_window_gathers(p) == gathers
            L.qb3_destroy_decoder(p)
    tw, th = 40, 20
    rects = [((7 + 31 * i) % (Wd - tw), (5 + 13 * i) % (Ht - th), tw, th) for i in range(6)]
    _, buf = call_and_check(qb3, dec, d_c, rows, bands, tsz, rects, sel, 1, gathers,
                            mosaic=(3 * tw * nsel, [((i % 3) * tw * nsel, (i // 3) * th) for i in range(6)], 2 * th))
    mosaic = buf[16:16 + tsz * 3 * tw * nsel * 2 * th].view(2 * th, -1)
    px = nsel * tsz
    for i, (x0, y0, w, h) in enumerate(rects):
        assert torch.equal(mosaic[(i // 3) * th:(i // 3 + 1) * th, (i % 3) * tw * px:(i % 3 + 1) * tw * px], want[y0:y0 + h, x0 * px:(x0 + w) * px]), i
    assert bool((buf[:16] == WB.SENTINEL).all()) and bool((buf[16 + mosaic.numel():] == WB.SENTINEL).all())
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 6. quanta
@pytest.mark.parametrize("case", ((WU.I16, 7, UNIT, 2, 1, 0), (WU.I16, 7, 0, 2, 2, 1), (WU.I16, 7, UNIT, 1, 3, 1), (WU.U8, 3, 0, 2, 1, 1)),
                         ids=("i16x7-fused", "i16x7-strips", "i16x7-whole", "u8-rgb"))
def test_quanta_commute_with_the_selection(qb3, case):
    """quanta 3 on a BASE container, a signed type among them: the fused route multiplies the window back as a raster of nsel bands,
    the gather multiplies while it picks; expected: the second handle's whole decode with the bands picked"""
    import torch
    from qb3_amd import device as qdev, synth
    dt, bands, bits, level, path, gathers = case
    Wd, Ht, tsz = 201, 67, TSZ[dt]
    img = synth.generate(Wd, Ht, bands, dt, "NOISY3", 11)
    d_c, n, _ = D.make_container(qb3, img, dt, BASE, level, quanta=3)
    want = D.full_decode(qb3, d_c, n)[0]
    assert want is not None and not torch.equal(want, img.reshape(-1).view(torch.uint8))
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(bits)
    rects = W16.windows(Wd, Ht, 3, D.segment_size(qb3, dec), 1)
    for sel in ([bands - 1, 0], [1, 1, 0]):
        call_and_check(qb3, dec, d_c, want.view(Ht, -1), bands, tsz, rects, sel, path, gathers)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 7. damage
def test_a_damaged_table_costs_time_not_pixels(qb3):
    """uint8 x 5 with the bit set.  A flipped entry byte fails its chunk's check: every window goes path 3.  One lane's twelve-bit
    length + 1 under a re-sealed check, in a segment only the first of two windows touches: that window goes path 3, the other stays
    on path 1.  Expected bytes: the second handle's whole decode of the damaged container, which is the source raster"""
    import torch
    from qb3_amd import device as qdev, synth
    dt, bands, Wd, Ht = WU.U8, 5, 1001, 259
    tsz = TSZ[dt]
    img = synth.generate(Wd, Ht, bands, dt, "DEM", 5)
    rows = D.as_rows(img, Ht)
    d_c, n, _ = D.make_container(qb3, img, dt, FTL, 2)
    host = d_c[:n].cpu().numpy()
    chunks, _ = D.table_chunks(host)
    E = WU.entry_bytes(bands, tsz)
    per_chunk = (chunks[0][1] - 12) // E
    bps = WU.seg_blocks(bands)
    nbx, _ = W.blocks_of(Wd, Ht)
    wins = [(40, 24, 300, 40), (40, 200, 100, 20)]              # block rows 6..15 and 50..54: no segment in common
    seg = (6 * nbx + 10) // bps + 1
    assert seg < (50 * nbx) // bps
    e0 = chunks[seg // per_chunk][0] + 12 + (seg % per_chunk) * E
    sel = [4, 0, 2]

    def upload(a):
        t = torch.zeros_like(d_c)
        t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t

    def run(bad, paths, gathers):
        d_bad = upload(bad)
        want = D.full_decode(qb3, d_bad, n)[0]
        assert want is not None and torch.equal(want.view(Ht, -1), rows)
        dec = qdev.DeviceDecoder(d_bad, n)
        dec.set_window_kernels(UNIT)
        call_and_check(qb3, dec, d_bad, want.view(Ht, -1), bands, tsz, wins, sel, paths, gathers)
        dec.close()

    run(host, [1, 1], 0)                                        # the sound container first
    bad = host.copy()
    bad[e0 + 7] ^= 0x10
    run(bad, [3, 3], 1)
    bad = host.copy()
    fields = e0 + 6 + bands * (1 + tsz)
    nf = E - 6 - bands * (1 + tsz)
    v = int.from_bytes(bytes(bad[fields:fields + nf]), "little")
    f = (v >> 60) & 4095                                        # lane 5's field
    v = (v & ~(4095 << 60)) | (((f + 1) & 4095) << 60)
    bad[fields:fields + nf] = np.frombuffer(v.to_bytes(nf, "little"), np.uint8)
    c0, cl = chunks[seg // per_chunk]
    s16 = D.chunk_check(bad[c0 + 12:c0 + cl])
    bad[c0 + 6], bad[c0 + 7] = s16 & 255, s16 >> 8
    run(bad, [3, 1], 1)


# ---------------------------------------------------------------------------------------------------------------- 8. identity
@pytest.mark.parametrize("case", ((WU.U8, 5, UNIT), (WU.U8, 3, 0)), ids=("u8x5", "u8-rgb"))
def test_the_identity_selection_is_the_full_band_call(qb3, case):
    import torch
    from qb3_amd import device as qdev, synth
    L = qb3.lib
    dt, bands, bits = case
    Wd, Ht, tsz = 201, 67, TSZ[dt]
    img = synth.generate(Wd, Ht, bands, dt, "NOISY3", 4)
    d_c, n, _ = D.make_container(qb3, img, dt, FTL, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    dec.set_window_kernels(bits)
    rects = W16.windows(Wd, Ht, 21, D.segment_size(qb3, dec), 1)
    lay = D.Layout(rects, bands * tsz, tsz, "unit")
    got, full = D.batch_call(qb3, dec, d_c, lay)
    assert got == len(rects)
    segs = L.qb3x_last_window_segments(dec.p)
    lay2, buf = call_and_check(qb3, dec, d_c, D.as_rows(img, Ht), bands, tsz, rects, list(range(bands)), 1, 0, segs=segs)
    assert lay2.offs == lay.offs and torch.equal(buf, full)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 9. Python
def test_python_device_decoder_takes_bands(qb3):
    import torch
    from qb3_amd import device as qdev, synth
    Wd, Ht, bands = 201, 67, 7
    img = synth.generate(Wd, Ht, bands, WU.I16, "DEM", 2)
    d_c, n, _ = D.make_container(qb3, img, WU.I16, FTL, 2)
    dec = qdev.DeviceDecoder(d_c, n)
    rects = [(3, 5, 50, 20), (100, 40, 101, 27), (0, 0, Wd, Ht)]
    for bits, gathers in ((UNIT, 0), (0, 1)):
        dec.set_window_kernels(bits)
        outs = dec.decode_windows(d_c, rects, bands=[6, 2, 0])
        assert dec.last_window_gathers() == gathers
        for o, (x0, y0, w, h) in zip(outs, rects):
            assert o.shape == (h, w, 3) and o.dtype == torch.int16 and torch.equal(o, img[y0:y0 + h, x0:x0 + w][:, :, [6, 2, 0]])
        one = dec.decode_window(d_c, 3, 5, 50, 20, bands=[1])
        assert one.shape == (20, 50, 1) and torch.equal(one, img[5:25, 3:53, 1:2])
        outs = dec.decode_windows(d_c, rects)                   # bands=None: as before
        for o, (x0, y0, w, h) in zip(outs, rects):
            assert o.shape == (h, w, bands) and torch.equal(o, img[y0:y0 + h, x0:x0 + w])
    dec.close()
