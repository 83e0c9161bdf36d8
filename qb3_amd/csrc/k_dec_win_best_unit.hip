// qb3_amd/csrc/k_dec_win_best_unit.hip -- the window kernels of the common-factor rasters that decode a lane per unit and of one-band
// 16/32/64-bit common-factor rasters, single and batch: the shells of qb3_win.h over winu_best_decode_wave (qb3_win_best_unit.h), and
// the family's record.
#include "qb3_win_best_unit.h"

namespace qb3dev {

static void win_cfu_one(const Geometry &g, const DecPlan &plan, const WinArgs &wa, const WinLaunch &l) {
    win_cfu_pick(g, plan, [&](auto f) { win_launch(f, wa, l); });
}
static void win_cfu_batch(const Geometry &g, const DecPlan &plan, const WinBatchArgs &ba, const WinLaunch &l) {
    win_cfu_pick(g, plan, [&](auto f) { win_launch(f, ba, l); });
}
// the band-selected batch: the same wave routine with winu_store_tile's SEL (ba.d.sel_nibs, ba.d.nsel)
static void win_cfu_batch_sel(const Geometry &g, const DecPlan &plan, const WinBatchArgs &ba, const WinLaunch &l) {
    win_cfu_pick<true>(g, plan, [&](auto f) { win_launch(f, ba, l); });
}

static bool decode_window_best_unit_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    const DecKernel k = aligned_dec_kernel(g, plan);
    return decode_strips_ok(g, plan, ix) && (k == DecKernel::pxu_best || k == DecKernel::pxw_best) && g.seg_blocks * g.bands <= 64 &&
           ix.block_lens && ix.version >= 3 && window_unit_geometry_ok(g);
}

// The common-factor rasters (QB3M_CF, QB3M_CF_H; QB3M_BEST / QB3M_CF_RLE where the RLE0 pass did not win) that the whole-raster decoders
// dec_pxu_best_kernel and dec_pxw_best_kernel take -- 8-bit rasters of 2 or more than 4 bands, 16/32/64-bit rasters of several bands,
// and one-band 16/32/64-bit rasters -- whose table (level 1 or 2, version 3: the common-factor entries carry a three-byte field per
// unit at either) those kernels decode a segment from alone, on a geometry one launch holds: dec_pxu_best_kernel's BL branch
// (k_dec_pxu.hip), a wave per segment of 64 / bands blocks, a lane per unit.  The one-band entry (dec_pxw_best_kernel's, k_dec_pxw.hip)
// has the lane-per-unit layout with one band, so the same routine takes it.  Mapping, de-duplication, trust and status are described
// at the head of k_dec_win.hip and hold here with the raster's blocks per segment in place of 64.  What differs from win_unit:
//   * THE ENTRY  carries, besides position and entering values, the FACTOR each band is entered with, and per unit its bits | the rung it
//     is entered with << 12: a common-factor unit leaves its band at the rung of the multiplied values, so rungs are not a scan of the
//     switch codes.  Inside the segment the factor in force is the band's nearest writer among the lanes below, found by a ballot; before
//     the first writer it is the entry's.
//   * NO CODE TABLE, NO BARRIER  The common-factor parser reads the stream with the branchy reader and no table in LDS: the launch brings
//     four waves' worst-case staging and nothing else, and the waves share nothing.
//   * TRUST  Every consistency test of dec_pxu_best_kernel stays: a unit's leaving rung against the band's next unit's entering rung, the
//     end of a unit against its length, a malformed unit.  An entry's entering VALUE or FACTOR that was changed under a re-sealed check is
//     detected by neither this kernel nor the whole decode from the table: both give the same wrong pixels.
// Destinations must be value aligned: the stores are winu_store_tile's.
const WinKernels &win_cfu() {      // (in a function: host data, not for the device side of this file)
    static const WinKernels k = { decode_window_best_unit_ok, QB3X_WINK_CFU, window_align_value, window_unit_dec_args, window_best_unit_lds_bytes, "common-factor lane-per-unit ", "dec_window_best_unit", nullptr, win_cfu_one, win_cfu_batch, nullptr, win_cfu_batch_sel };
    return k;
}

}  // namespace qb3dev
