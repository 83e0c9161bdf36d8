// qb3_amd/csrc/k_dec_wins_best_ranged.hip -- a batch of windows of one 8-bit common-factor raster decoded from PIECES of its container:
// what k_dec_wins_ranged.hip does for FTL / BASE rasters, with the wave's work of the common-factor window kernels
// (win_best_decode_wave, qb3_win_best.h) under the ranged source policy (WinSrcPieces, qb3_win.h).  PIECES, TRUST and STATUS are
// described at the head of k_dec_wins_ranged.hip and hold here; the entry is k_dec_win_best.hip's (E = 6 + 3 * bands + 192 bytes: position,
// rungs, entering values, entering factors, a 3-byte field per block).  What the policy guarantees under win_best_decode_wave, read off
// its code:
//   * a wave that is not live asks find(0, false), entry(a, 0) and, if the raster has more than one segment, entry(a, 1).  find() then
//     either finds segment 0 in the first piece or falls to pieces[0] with nwords = 0; either way entry() answers with the compact
//     array's first entries (the first piece's ent0 is 0; k - seg0 is 0 or 1, or wraps above nseg and is taken as 0), and every piece has two at least.  Of them
//     the six position bytes and the pv0 / cf0 bytes are loaded -- the field is not: act is false -- and the wave leaves behind the
//     barrier without using any of it;
//   * a live wave's lanes all form the field's address; lanes without a block (act false) do not load it.  The farthest byte a lane
//     reads from entry seg is lane 63's third field byte, 6 + 3B + 3 * 63 + 2 = E - 1, the entry's last.  Of entry seg + 1 only the six
//     position bytes are read; for the raster's last segment that entry is not read at all (the stream's length ends it), so the
//     zeros the host puts there are never seen;
//   * holds(w0, ndw) is the only gate to word(): ndw is zero unless it said yes, and word() is asked for i < ndw only.  A segment that
//     is not wholly inside its piece stages zeros and raises status bit 3, as one that exceeds the staging area does;
//   * the eight zero words behind a segment are the staging loop's own (i in [ndw, ndw + 8) stores 0 without asking the source): what
//     best_slow_unit and px_group read ahead of `limit` is LDS of this wave, never the packed words;
//   * the host clamps a piece's nwords to what was packed behind word0 (api_ranged.cpp), so holds() yes means word0 + (w - sw0) lies
//     inside the uploaded words whatever the entries' positions say.
// No check workgroups: the host verified the chunks (chunk_sound, api_ranged.cpp) before a byte of the stream was asked for.  As in
// k_dec_win_best.hip an entry's entering VALUE or FACTOR changed under a re-sealed check is detected by nobody; here only the host's
// 16-bit chunk check stands in front of it.
#include "qb3_win_best.h"

namespace qb3dev {

void win_cf8_ranged(const Geometry &g, const DecPlan &plan, const WinRangedArgs &ra, const WinLaunch &l) {
    win_cf8_pick(g, plan, [&](auto f) { win_launch(f, ra, l); });
}

}  // namespace qb3dev
