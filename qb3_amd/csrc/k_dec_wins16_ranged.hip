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

template <int BG, bool RGB, uint64_t ORDER, bool STEP>
__global__ void __launch_bounds__(256, 4) dec_wins16_ranged_kernel(const WinRangedArgs ra) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t gw = blockIdx.x * 4 + wave;          // (wave uniform, as are both searches)
    uint32_t lo = 0, hi = ra.nwin;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ra.wins[mid].wave0 <= gw) lo = mid; else hi = mid;
    }
    lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    const WinDesc w = ra.wins[lo];
    win16_decode_wave<BG, RGB, ORDER, STEP, WinSrcPieces>(ra.d, w, ra.wstatus + lo, smem, wave, gw - w.wave0, ra.src);
}

int launch_decode_windows16_ranged(const Geometry &g, const DecPlan &plan, uint32_t in_bit0, uint64_t in_bits, const void *h_descs, const void *d_descs,
                                   size_t n, const void *d_pieces, size_t npieces, const void *d_entries, const uint32_t *d_words,
                                   uint32_t *d_status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window16_ok(g, plan, ix) || !n || !npieces || npieces > 0xffffffffull) { set_error("16-bit ranged window batch: not for this raster", 0); return -1; }
    WinRangedArgs ra = {};
    IxTable none = ix;
    none.base = nullptr;            // (the table is not in device memory)
    window_dec_args(ra.d, g, plan, nullptr, in_bit0, in_bits, d_status, none);
    window16_dec_args(ra.d, plan);
    ra.src.pieces = (const WinPiece *)d_pieces; ra.src.npieces = (uint32_t)npieces;
    ra.src.ents = (const uint8_t *)d_entries; ra.src.words = d_words;
    window_ranged_launches(ra, h_descs, d_descs, n, d_status, [&](const WinRangedArgs &args, dim3 grid) {
        ProfScope ps("dec_window16_ranged", st);
        QB3_WIN16_DISPATCH(dec_wins16_ranged_kernel, args);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
