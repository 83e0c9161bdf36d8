// qb3_amd/csrc/k_dec_win16.hip -- the window kernels of 16-bit rasters, single and batch: the shells of qb3_win.h over win16_decode_wave
// (qb3_win16.h), and the family's record.
#include "qb3_win16.h"

namespace qb3dev {

static void win16_one(const Geometry &g, const DecPlan &plan, const WinArgs &wa, const WinLaunch &l) {
    win16_pick(g, plan, [&](auto f) { win_launch(f, wa, l); });
}
static void win16_batch(const Geometry &g, const DecPlan &plan, const WinBatchArgs &ba, const WinLaunch &l) {
    win16_pick(g, plan, [&](auto f) { win_launch(f, ba, l); });
}

static bool decode_window16_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    return decode_strips_ok(g, plan, ix) && aligned_dec_kernel(g, plan) == DecKernel::px16 && ix.block_lens && ix.version >= 3 && g.nblocks < (1ull << 31);
}
static uint32_t window16_align(const Geometry &) { return 2; }

// 16-bit rasters of 1, 2, 3, 4, 6 or 8 bands (FTL / BASE) whose level-2 table (version 3) carries the lane fields dec_px16_kernel's
// BL branch (k_dec_px16.hip) decodes a segment from alone: a wave per segment of 64 / band groups blocks, a lane per block and band
// group.  Mapping, de-duplication, clipping, trust and status are described at the head of k_dec_win.hip and hold here with the
// raster's blocks per segment in place of 64.  What differs from the 8-bit family:
//   * STAGING  The launch brings LDS for the worst-case segment (the plan's px_cap_dw), so there is no "sized for this stream's average,
//     run again" status: a segment that does not fit is not this stream's.
//   * STORES  A lane holds BG bands of its block's pixels.  A block wholly inside the window's columns stores dwords, the form chosen
//     row by row from the address (a row on a dword; a row off by a halfword: head halfword, aligned dwords, tail halfword); the two
//     lanes of an eight-band block swap halves and store 32 contiguous bytes each where the row lies on a 16-byte address.  An edge
//     block stores halfwords one by one under the column mask -- so every destination must be halfword aligned.
const WinKernels &win_u16() {      // (in a function: host data, not for the device side of this file)
    static const WinKernels k = { decode_window16_ok, QB3X_WINK_U16, window16_align, window16_dec_args, window_lds_px, "16-bit ", "dec_window16", "dec_window16_ranged", win16_one, win16_batch, win16_ranged };
    return k;
}

}  // namespace qb3dev
