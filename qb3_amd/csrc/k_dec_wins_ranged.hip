// qb3_amd/csrc/k_dec_wins_ranged.hip -- a batch of windows of one raster decoded from PIECES of its container: the batch kernel's work
// (k_dec_wins.hip) for a caller who holds a file or an object, not the container, and has fetched only the byte ranges of the
// segments the windows need (api_ranged.cpp).  The wave's work is win_decode_wave's (qb3_win.h) with the ranged source policy:
//   * PIECES  The host packs the fetched ranges back to back, copies the table entries their segments use into a compact array and
//     lists the pieces (runs of consecutive segments) sorted by first segment.  After finding its window as the batch kernel does, a
//     wave finds its piece by a wave-uniform binary search of that list -- scalar loads -- and takes its two entries and its stream
//     words from there.
//   * TRUST  The table's chunks are verified on the host before a byte of the stream is asked for, so the launch has no check
//     workgroups.  A 16-bit check can collide: the kernel reads no word outside its piece and no entry outside the compact array,
//     whatever the entries say.  A segment that is not wholly inside its piece stages zeros and raises status bit 3, as one that
//     exceeds the staging area does; a wave whose segment has no piece raises it and leaves.
//   * STATUS  A word per window, as in the batch kernel; the host takes any nonzero word as "this window from the whole decode".
#include "qb3_win.h"

namespace qb3dev {

void win_u8_ranged(const Geometry &g, const DecPlan &plan, const WinRangedArgs &ra, const WinLaunch &l) {
    win_u8_pick(g, plan, [&](auto f) { win_launch(f, ra, l); });
}

}  // namespace qb3dev
