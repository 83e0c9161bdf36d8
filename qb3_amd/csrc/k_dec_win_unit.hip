// qb3_amd/csrc/k_dec_win_unit.hip -- the window kernels of the lane-per-unit rasters and of one-band 32/64-bit rasters, single and batch:
// the shells of qb3_win.h over winu_decode_wave (qb3_win_unit.h), and the family's record.
#include "qb3_win_unit.h"

namespace qb3dev {

static void win_unit_one(const Geometry &g, const DecPlan &plan, const WinArgs &wa, const WinLaunch &l) {
    win_unit_pick(g, plan, [&](auto f) { win_launch(f, wa, l); });
}
static void win_unit_batch(const Geometry &g, const DecPlan &plan, const WinBatchArgs &ba, const WinLaunch &l) {
    win_unit_pick(g, plan, [&](auto f) { win_launch(f, ba, l); });
}
// the band-selected batch: the same wave routine with winu_store_tile's SEL (ba.d.sel_nibs, ba.d.nsel)
static void win_unit_batch_sel(const Geometry &g, const DecPlan &plan, const WinBatchArgs &ba, const WinLaunch &l) {
    win_unit_pick<true>(g, plan, [&](auto f) { win_launch(f, ba, l); });
}

static bool decode_window_unit_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    const DecKernel k = aligned_dec_kernel(g, plan);
    return decode_strips_ok(g, plan, ix) && (k == DecKernel::pxu || k == DecKernel::pxw) && g.seg_blocks * g.bands <= 64 &&
           ix.block_lens && ix.version >= 3 && window_unit_geometry_ok(g);
}

// The rasters of the lane-per-unit decoder (8-bit rasters of 2 or more than 4 bands, 16-bit rasters of an odd band count above 4,
// 32/64-bit rasters of several bands) and one-band 32/64-bit rasters, FTL / BASE, whose level-2 table (version 3) carries the
// twelve-bit unit lengths dec_pxu_kernel's BL branch (k_dec_pxu.hip) decodes a segment from alone, on a geometry one launch holds
// (window_unit_geometry_ok): a wave per segment of 64 / bands blocks, a lane per unit.  The one-band 32/64-bit entry (dec_pxw_kernel's,
// k_dec_pxw.hip) has the lane-per-unit layout with one band, so the same routine takes it.  Mapping, de-duplication, trust and status
// are described at the head of k_dec_win.hip and hold here with the raster's blocks per segment in place of 64.  What differs from
// the 8-bit family:
//   * STAGING  The launch brings LDS for the worst-case segment (the plan's px_cap_dw), so there is no "sized for this stream's average,
//     run again" status: a segment that does not fit is not this stream's.
//   * STORES  The lanes write their values into the wave's LDS tile, laid out like the image ([row][block][x][band]), once every lane
//     holds its sixteen values.  A block whose four columns are its own and the window's stores its rows -- those that are its own and
//     the window's -- in pieces of 16, 8 or 4 bytes at value-aligned addresses; an edge block stores value by value under its column
//     mask -- so every destination must be value aligned.  A lane finds the numbers of the block it stores for (offset in the window,
//     row and column masks) by a shuffle from the lane of that block's number.
const WinKernels &win_unit() {      // (in a function: host data, not for the device side of this file)
    static const WinKernels k = { decode_window_unit_ok, QB3X_WINK_UNIT, window_align_value, window_unit_dec_args, window_unit_lds_bytes, "lane-per-unit ", "dec_window_unit", nullptr, win_unit_one, win_unit_batch, nullptr, win_unit_batch_sel };
    return k;
}

}  // namespace qb3dev
