// qb3_amd/csrc/k_dec_wins16_ranged.hip -- a batch of windows of one 16-bit raster decoded from PIECES of its container: what
// k_dec_wins_ranged.hip does for 8-bit rasters, with the wave's work of the 16-bit window kernels (win16_decode_wave, qb3_win16.h)
// under the ranged source policy (WinSrcPieces, qb3_win.h).  PIECES, TRUST and STATUS are described at the head of
// k_dec_wins_ranged.hip and hold here with the raster's blocks per segment (64 / band groups) in place of 64.  What the policy
// guarantees under win16_decode_wave, read off its code:
//   * a wave that is not live asks find(0, false) and entry(a, 0), entry(a, 1): the compact array's first entries (every piece has
//     two at least), of which nothing is taken;
//   * every lane reads its two length fields (one for a single band) whether it holds a block or not: lane 63's last byte is byte
//     159 of the 160 field bytes (79 of 80), inside the entry's E bytes; of entry seg + 1 only the six position bytes are read;
//   * holds(w0, ndw) is the only gate to word(): a segment that is not wholly inside its piece stages zeros (status bit 3), and the
//     16 zero words px16_groups_hi reads ahead are the staging loop's own, never the source's.
#include "qb3_win16.h"

namespace qb3dev {

void win16_ranged(const Geometry &g, const DecPlan &plan, const WinRangedArgs &ra, const WinLaunch &l) {
    win16_pick(g, plan, [&](auto f) { win_launch(f, ra, l); });
}

}  // namespace qb3dev
