"""The window kernels of the remaining common-factor rasters (include/qb3x.h: qb3x_set_decoder_window_kernels, QB3X_WINK_CFU), the part
that needs no GPU: the bit exists and is harmless where the kernels do not apply, the header still compiles as C and C++, the entry size
the kernels read by is what a restatement gives, and the rasters of test_window_best_unit_decode.py are coded common-factor containers
whose streams hold signal units."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
import qb3_window_unit as WU  # noqa: E402
import qb3_window_best_unit as WBU  # noqa: E402

BIT = WBU.QB3X_WINK_CFU
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_bit_is_declared_and_bound(qb3):
    text = open(os.path.join(ROOT, "include", "qb3x.h")).read()
    assert "#define QB3X_WINK_CFU 8u" in text and qb3.QB3X_WINK_CFU == BIT == 8
    assert BIT & (qb3.QB3X_WINK_U16 | qb3.QB3X_WINK_CF8 | qb3.QB3X_WINK_UNIT) == 0
    names = text[text.index("Kernel names:"):]
    names = names[:names.index("level: 0 off")]
    assert "dec_window_best_unit" in names
    qb3.lib.qb3x_set_decoder_window_kernels(None, BIT)                      # a NULL handle: no-op
    from qb3_amd import device as qdev
    assert "QB3X_WINK_CFU" in qdev.DeviceDecoder.set_window_kernels.__doc__ and "QB3X_WINK_CFU" in qb3.RangedReader.set_window_kernels.__doc__


@pytest.mark.parametrize("lang", ("c", "c++"))
def test_the_header_compiles_as_c_and_cxx(tmp_path, lang):
    src = tmp_path / ("use." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "qb3x.h"\nint main(void) { return (int)(QB3X_WINK_CFU | QB3X_WINK_UNIT | QB3X_WINK_CF8 | QB3X_WINK_U16) == 15 ? 0 : 1; }\n')
    exe = tmp_path / "use"
    subprocess.run(["gcc" if lang == "c" else "g++", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_the_bit_is_harmless_where_the_kernels_do_not_apply(qb3, oracle):
    """an oracle-made container (no table), a STORED one, a narrow one: the setter takes the bit, the handle stays good,
    qb3x_window_segments says what it said, and qb3x_read_window on the STORED container still crops on the host with the bit set"""
    L = qb3.lib
    for (w, h, b, dt, gen, mode, stored) in ((64, 48, 5, 0, "NOISY3", WBU.CF_H, False), (64, 48, 3, 4, "RANDOM", WBU.CF, True), (3, 400, 1, 4, "DEM", WBU.BEST, False)):
        img = oracle.generate(w, h, b, dt, gen, 5)
        s = oracle.encode(img, dt, mode)
        p, dims = W.open_handle(L, s)
        assert dims == (w, h, b) and (L.qb3_get_mode(p) == 255) == stored
        bps0 = C.c_size_t()
        before = L.qb3x_window_segments(p, 0, 0, w, h, C.byref(bps0))
        for mask in (BIT, BIT | 7, 0xffffffff, 0, BIT):
            L.qb3x_set_decoder_window_kernels(p, mask)
            bps = C.c_size_t()
            assert W.handle_error(p) == W.QB3E_OK and L.qb3x_window_segments(p, 0, 0, w, h, C.byref(bps)) == before and bps.value == bps0.value
        if stored:
            win = (5, 7, 11, 13)
            nb = 13 * 11 * b * WU.TSZ[dt]
            out = np.full(nb + 16, 0x5a, np.uint8)
            assert L.qb3x_read_window(p, *win, out.ctypes.data, 0) == nb
            assert L.qb3x_last_window_path(p) == 3 and L.qb3x_last_window_segments(p) == 0
            assert np.array_equal(out[:nb].view(img.dtype).reshape(13, 11, b), img[7:20, 5:16]) and (out[nb:] == 0x5a).all()
        L.qb3_destroy_decoder(p)


def test_the_entry_size_restated():
    """6 position bytes, per band a rung byte, an entering value and a factor, three bytes a unit of the 64 // bands blocks: with one
    band that is dec_pxw_best_kernel's entry (7 + 2 * tsz + 192), and the fields start where both whole-raster kernels read them"""
    for dt, bands in WBU.MATRIX:
        tsz, nb = WU.TSZ[dt], 64 // bands
        assert WBU.entry_bytes(bands, tsz) == 6 + bands * (1 + 2 * tsz) + 3 * nb * bands
        assert WBU.field_at(bands, tsz, nb * bands - 1) + 3 == WBU.entry_bytes(bands, tsz)
        if bands == 1:
            assert WBU.entry_bytes(1, tsz) == 7 + 2 * tsz + 192 and WBU.field_at(1, tsz, 0) == 7 + 2 * tsz
        assert nb * bands <= 64 and nb >= 4


@pytest.mark.parametrize("pair", WBU.MATRIX, ids=lambda c: "t%d-b%d" % c)
def test_the_rasters_are_coded_common_factor_containers(oracle, pair):
    """every raster of the GPU tests with signal by construction (scaled, few, mixed) x QB3M_CF, QB3M_CF_H at every shape: the oracle's
    container is not STORED -- its mode byte is 1 or 5 -- and smaller than the same raster's in QB3M_BASE: the stream really holds
    signal units.  So none of those GPU cases may be skipped"""
    dt, bands = pair
    for si, (w, h) in enumerate(WU.shapes_of(dt, bands)):
        for name in WBU.SIGNAL:
            img = WBU.raster(name, w, h, bands, dt, 7 * w + bands)
            assert img.shape == (h, w, bands) and img.dtype == WBU.np_type(dt)
            base = len(oracle.encode(img, dt, WBU.BASE))
            for mode in (WBU.CF, WBU.CF_H):
                s = oracle.encode(img, dt, mode)
                assert int(s[10]) == mode, (name, w, h, mode, int(s[10]))
                assert len(s) < base, (name, w, h, mode, len(s), base)
