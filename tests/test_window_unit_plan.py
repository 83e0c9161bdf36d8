"""The window kernels of the lane-per-unit and one-band 32/64-bit rasters (include/qb3x.h: qb3x_set_decoder_window_kernels,
QB3X_WINK_UNIT), the part that needs no GPU: the bit exists and is harmless where the kernels do not apply, qb3x_window_segments counts
what an enumeration counts for the segment sizes of these rasters (64 // bands blocks), window_unit_geometry_ok (qb3_dev.h) draws the
line a launch's size draws, and the generators of test_window_unit_decode.py reach the value decoders on both sides of rung 8."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window as W  # noqa: E402
import qb3_window16 as W16  # noqa: E402
import qb3_window_unit as WU  # noqa: E402

FTL, BASE = WU.FTL, WU.BASE
BIT = WU.QB3X_WINK_UNIT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_bit_is_declared_and_bound(qb3):
    text = open(os.path.join(ROOT, "include", "qb3x.h")).read()
    assert "#define QB3X_WINK_UNIT 4u" in text and qb3.QB3X_WINK_UNIT == BIT == 4
    assert BIT & (qb3.QB3X_WINK_U16 | qb3.QB3X_WINK_CF8) == 0 and qb3.QB3X_WINK_U16 | qb3.QB3X_WINK_CF8 | BIT == 7
    names = text[text.index("Kernel names:"):]
    names = names[:names.index("level: 0 off")]
    assert "dec_window_unit" in names
    qb3.lib.qb3x_set_decoder_window_kernels(None, BIT)                      # a NULL handle: no-op
    from qb3_amd import device as qdev
    assert "QB3X_WINK_UNIT" in qdev.DeviceDecoder.set_window_kernels.__doc__


def test_the_bit_is_harmless_where_the_kernels_do_not_apply(qb3, oracle):
    """an oracle-made container (no table), a STORED one, a narrow one: the setter takes the bit, the handle stays good,
    qb3x_window_segments says what it said, and qb3x_read_window on the STORED container still crops on the host with the bit set"""
    L = qb3.lib
    for (w, h, b, dt, gen, stored) in ((64, 48, 5, 0, "NOISY3", False), (64, 48, 3, 4, "RANDOM", True), (3, 400, 1, 4, "DEM", False)):
        img = oracle.generate(w, h, b, dt, gen, 5)
        s = oracle.encode(img, dt, FTL)
        p, dims = W.open_handle(L, s)
        assert dims == (w, h, b) and (L.qb3_get_mode(p) == 255) == stored
        bps0 = C.c_size_t()
        before = L.qb3x_window_segments(p, 0, 0, w, h, C.byref(bps0))
        for mask in (BIT, BIT | 3, 0xffffffff, 0, BIT):
            L.qb3x_set_decoder_window_kernels(p, mask)
            bps = C.c_size_t()
            assert W.handle_error(p) == W.QB3E_OK and L.qb3x_window_segments(p, 0, 0, w, h, C.byref(bps)) == before and bps.value == bps0.value
        if stored:
            win = (5, 7, 11, 13)
            tsz = WU.TSZ[dt]
            nb = 13 * 11 * b * tsz
            out = np.full(nb + 16, 0x5a, np.uint8)
            assert L.qb3x_read_window(p, *win, out.ctypes.data, 0) == nb
            assert L.qb3x_last_window_path(p) == 3 and L.qb3x_last_window_segments(p) == 0
            assert np.array_equal(out[:nb].view(img.dtype).reshape(13, 11, b), img[7:20, 5:16]) and (out[nb:] == 0x5a).all()
        L.qb3_destroy_decoder(p)


@pytest.mark.parametrize("case", WU.PLAN_MATRIX, ids=lambda c: "t%d-b%d" % c[:2])
def test_segment_count_of_the_lane_per_unit_rasters(qb3, oracle, case):
    """64 // bands blocks a segment (64 for one band), whatever the value size; the count is the enumeration's for 100 windows a
    shape, with and without the bit"""
    L = qb3.lib
    dt, bands, want_bps = case
    assert want_bps == WU.seg_blocks(bands)
    for (Wd, Ht) in WU.shapes_of(dt, bands)[:3] + ((201, 67),):
        s = oracle.encode(oracle.generate(Wd, Ht, bands, dt, "NOISY3", 7), dt, BASE)
        p, dims = W.open_handle(L, s)
        assert dims == (Wd, Ht, bands)
        bps = C.c_size_t()
        L.qb3x_window_segments(p, 0, 0, Wd, Ht, C.byref(bps))
        assert bps.value == want_bps
        wins = W16.windows(Wd, Ht, 100 * bands + Wd, want_bps, 100)
        counts = {}
        for mask in (0, BIT):
            L.qb3x_set_decoder_window_kernels(p, mask)
            counts[mask] = [L.qb3x_window_segments(p, *win, None) for win in wins]
        assert counts[0] == counts[BIT] == [W.brute_segments(Wd, Ht, *win, bps=want_bps) for win in wins], (Wd, Ht)
        L.qb3_destroy_decoder(p)


GEOMETRY_MAIN = r"""
#include "qb3_dev.h"
#include <stdio.h>
#include <stdlib.h>
// argv: width height seg_blocks [nblocks]; prints 1 or 0
int main(int argc, char **argv) {
    if (argc < 4) return 2;
    qb3dev::Geometry g = {};
    g.w = (uint32_t)strtoull(argv[1], nullptr, 10); g.h = (uint32_t)strtoull(argv[2], nullptr, 10);
    g.seg_blocks = (uint32_t)strtoull(argv[3], nullptr, 10);
    g.nbx = (g.w + 3) / 4; g.nby = (g.h + 3) / 4;
    g.nblocks = argc > 4 ? strtoull(argv[4], nullptr, 10) : (uint64_t)g.nbx * g.nby;
    printf("%d\n", qb3dev::window_unit_geometry_ok(g) ? 1 : 0);
    return 0;
}
"""


def test_one_window_fits_one_launch(tmp_path):
    """window_unit_geometry_ok: nby * (nbx / seg_blocks + 2) waves at most against WIN_LAUNCH_WAVES = 2^24, and nblocks below 2^31.
    65536 x 65536 (16384 x 16384 blocks): 16384 * (16384 / NB + 2) is 2^23 + 2^15 at NB = 32 and below 2^24 at 21, 2^24 + 2^15 at 16
    and more below; 16384 x 16384 at NB = 4: 4096 * 1026 < 2^24.  A program of its own from a source that includes qb3_dev.h alone"""
    src = tmp_path / "geometry_main.cpp"
    src.write_text(GEOMETRY_MAIN)
    exe = tmp_path / "geometry_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "qb3_amd", "csrc"), "-o", str(exe), str(src)], check=True)

    def ok(*args):
        return subprocess.run([str(exe)] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.strip() == "1"

    assert ok(65536, 65536, 32) and ok(65536, 65536, 21) and ok(65536, 65536, 64)
    assert not ok(65536, 65536, 16) and not ok(65536, 65536, 12) and not ok(65536, 65536, 4)
    assert ok(16384, 16384, 4)
    assert ok(4096, 4096, 64, 2 ** 31 - 1) and not ok(4096, 4096, 64, 2 ** 31) and not ok(4096, 4096, 64, 2 ** 33)


def test_the_generators_reach_the_value_decoders_on_both_sides_of_rung_8(oracle):
    """The kernels decode a unit of rung 1..7 through the 2 KB code table and one of rung 8 and above by the code rule (32/64-bit data:
    wide_values_lds).  The rungs of a raster's units, restated in numpy from the oracle's generator output (WU.unit_rungs: one band,
    Hilbert order, FTL): NOISY3 (a gradient of slope 1 with three bits of noise) stays below rung 8 inside a block row (only the unit
    that starts a row sits about w = 256 below the end of the row before, and 8-bit data has no rung above 7); RANDOM in 32/64-bit
    data has deltas that fill the value (the largest of sixteen uniform mag-sign numbers misses the top two bits with probability
    2^-32); DEM (slope 37, six bits of noise, a block row starts about 37 w below the end of the row before) has units at rung 7 and below inside a row and at rung 9 and above where a row starts, for 16-, 32- and 64-bit data.
    BASE's step moves a unit by at most one rung: the margins hold for it too"""
    for dt, bits in ((0, 8), (2, 16)):
        r = WU.unit_rungs(oracle.generate(256, 24, 1, dt, "NOISY3", 11)[:, :, 0], bits)
        assert (r < 8).mean() > 0.9 and (bits > 8 or r.max() <= 7), bits
    for dt, bits in ((4, 32), (6, 64)):
        r = WU.unit_rungs(oracle.generate(256, 24, 1, dt, "RANDOM", 11)[:, :, 0], bits)
        assert r.max() <= bits - 1 and (r >= bits - 3).all(), bits
    for dt, bits in ((2, 16), (4, 32), (6, 64)):
        r = WU.unit_rungs(oracle.generate(256, 24, 1, dt, "DEM", 11)[:, :, 0], bits)
        assert (r >= 9).sum() >= 5 and (r < 8).sum() >= 5, bits
