// qb3_amd/csrc/k_dec_win_best.hip -- the window kernels of 8-bit rasters in the common-factor modes, single and batch: the shells of
// qb3_win.h over win_best_decode_wave (qb3_win_best.h), and the family's record.
#include "qb3_win_best.h"

namespace qb3dev {

static void win_cf8_one(const Geometry &g, const DecPlan &plan, const WinArgs &wa, const WinLaunch &l) {
    win_cf8_pick(g, plan, [&](auto f) { win_launch(f, wa, l); });
}
static void win_cf8_batch(const Geometry &g, const DecPlan &plan, const WinBatchArgs &ba, const WinLaunch &l) {
    win_cf8_pick(g, plan, [&](auto f) { win_launch(f, ba, l); });
}

static bool decode_window_best_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    return decode_strips_ok(g, plan, ix) && aligned_dec_kernel(g, plan) == DecKernel::px_best && g.seg_blocks == 64 && g.nblocks < (1ull << 31);
}

// 8-bit grey / RGB / RGBA rasters in the common-factor modes (QB3M_CF, QB3M_CF_H; QB3M_BEST / QB3M_CF_RLE where the RLE0 pass did not
// win) whose table (level 1 or 2) carries the block fields dec_px_best_kernel's BL branch (k_dec_px_best.hip) decodes a segment from
// alone.  Mapping, de-duplication, clipping, trust and status are described at the head of k_dec_win.hip and hold here.  What differs
// from the 8-bit FTL / BASE family:
//   * THE ENTRY  carries, besides position, rungs and entering values, the FACTOR each band is entered with, and a 3-byte field per
//     block (its bits | the rungs its units are entered with << 12): a common-factor unit leaves its band at the rung of the multiplied
//     values, so rungs are not a scan of the switch codes.  Inside the segment the factor in force is the nearest writer among the lanes
//     below, found by a ballot; before the first writer it is the entry's.  Nothing a segment needs lies outside its entry and its bits.
//   * ALL LANES DECODE  A lane's entering value and factor come from the lanes below it, so the 64 blocks of a segment are decoded
//     whether the window holds them or not; the lanes whose block is the window's store.
//   * TRUST  Every consistency test of dec_px_best_kernel stays: a unit's leaving rung against the next block's entering rung, the end of
//     a block's units against its length, a factor above the multiplied values, a malformed unit.  An entry's entering VALUE or FACTOR
//     that was changed under a re-sealed check is detected by neither this kernel nor the whole decode from the table: both give the
//     same wrong pixels.
// Destinations need no alignment: the stores are win_decode_wave's.
const WinKernels &win_cf8() {      // (in a function: host data, not for the device side of this file)
    static const WinKernels k = { decode_window_best_ok, QB3X_WINK_CF8, window_align_any, nullptr, window_lds_px, "common-factor ", "dec_window_best", "dec_window_best_ranged", win_cf8_one, win_cf8_batch, win_cf8_ranged };
    return k;
}

}  // namespace qb3dev
