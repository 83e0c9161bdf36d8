// qb3_amd/csrc/k_dec_wins_ranged.hip -- a batch of windows of one raster decoded from PIECES of its container: dec_wins_kernel's work
// (k_dec_wins.hip) for a caller who holds a file or an object, not the container, and has fetched only the byte ranges of the
// segments the windows need (api_ranged.cpp).  The wave's work is win_decode_wave's (qb3_win.h) with the ranged source policy:
//   * PIECES  The host packs the fetched ranges back to back, copies the table entries their segments use into a compact array and
//     lists the pieces (runs of consecutive segments) sorted by first segment.  After finding its window as dec_wins_kernel does, a
//     wave finds its piece by a wave-uniform binary search of that list -- scalar loads -- and takes its two entries and its stream
//     words from there.
//   * TRUST  The table's chunks are verified on the host before a byte of the stream is asked for, so the launch has no check
//     workgroups.  A 16-bit check can collide: the kernel reads no word outside its piece and no entry outside the compact array,
//     whatever the entries say.  A segment that is not wholly inside its piece stages zeros and raises status bit 3, as one that
//     exceeds the staging area does; a wave whose segment has no piece raises it and leaves.
//   * STATUS  A word per window, as in dec_wins_kernel; the host takes any nonzero word as "this window from the whole decode".
#include "qb3_win.h"

namespace qb3dev {

template <int B, bool RGB, uint64_t ORDER, bool STEP>
__global__ void __launch_bounds__(256) dec_wins_ranged_kernel(const WinRangedArgs ra) {
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
    win_decode_wave<B, RGB, ORDER, STEP, WinSrcPieces>(ra.d, w, ra.wstatus + lo, smem, wave, gw - w.wave0, ra.src);
}

template <int B, bool RGB>
static void launch_dec_wins_ranged_b(const WinRangedArgs &ra, dim3 grid, size_t lds, hipStream_t st) {
    const bool step = ra.d.g.mode != CM_FTL, z = ra.d.g.order == ZCURVE;
    const dim3 block(256);
    if (!z && !step) hipLaunchKernelGGL((dec_wins_ranged_kernel<B, RGB, HILBERT, false>), grid, block, lds, st, ra);
    else if (!z && step) hipLaunchKernelGGL((dec_wins_ranged_kernel<B, RGB, HILBERT, true>), grid, block, lds, st, ra);
    else if (z && !step) hipLaunchKernelGGL((dec_wins_ranged_kernel<B, RGB, ZCURVE, false>), grid, block, lds, st, ra);
    else hipLaunchKernelGGL((dec_wins_ranged_kernel<B, RGB, ZCURVE, true>), grid, block, lds, st, ra);
}

int launch_decode_windows_ranged(const Geometry &g, const DecPlan &plan, uint32_t in_bit0, uint64_t in_bits, const void *h_descs, const void *d_descs,
                                 size_t n, const void *d_pieces, size_t npieces, const void *d_entries, const uint32_t *d_words,
                                 uint32_t *d_status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_ok(g, plan, ix) || !n || !npieces || npieces > 0xffffffffull) { set_error("ranged window batch: not for this raster", 0); return -1; }
    WinRangedArgs ra = {};
    IxTable none = ix;
    none.base = nullptr;            // (the table is not in device memory)
    window_dec_args(ra.d, g, plan, nullptr, in_bit0, in_bits, d_status, none);
    ra.src.pieces = (const WinPiece *)d_pieces; ra.src.npieces = (uint32_t)npieces;
    ra.src.ents = (const uint8_t *)d_entries; ra.src.words = d_words;
    // one launch, unless the waves exceed WIN_LAUNCH_WAVES (window_batch_plan's prefixes)
    window_ranged_launches(ra, h_descs, d_descs, n, d_status, [&](const WinRangedArgs &ra, dim3 grid) {
        ProfScope ps("dec_window_ranged", st);
        if (g.bands == 1) launch_dec_wins_ranged_b<1, false>(ra, grid, plan.lds_px, st);
        else if (g.bands == 3) { if (plan.px_rgb) launch_dec_wins_ranged_b<3, true>(ra, grid, plan.lds_px, st); else launch_dec_wins_ranged_b<3, false>(ra, grid, plan.lds_px, st); }
        else { if (plan.px_rgb) launch_dec_wins_ranged_b<4, true>(ra, grid, plan.lds_px, st); else launch_dec_wins_ranged_b<4, false>(ra, grid, plan.lds_px, st); }
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
