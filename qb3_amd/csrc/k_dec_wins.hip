// qb3_amd/csrc/k_dec_wins.hip -- a batch of windows of one raster in ONE launch: dec_win_kernel's work (qb3_win.h, k_dec_win.hip) for
// many rectangles at once.  A tile server asks for tens of small windows of a raster it keeps in device memory; each is a hundred
// waves or so, far from filling the device, and each single call pays a launch, a status word and a wait.
//   * DESCRIPTORS  What the single kernel takes as arguments about its window (WinDesc) sits in an array in device memory, one
//     entry a window, with the exclusive prefix of the windows' wave counts.  Wave g of the launch finds its window by a binary
//     search for the last entry whose prefix is not above g; g and the search are wave uniform, the entry is read with scalar
//     loads, and from there on the wave is wave g - prefix of that window: mapping, de-duplication, clipping and stores are
//     win_decode_wave's.
//   * TRUST  The host merges the ranges of table chunks the windows read entries from into a sorted list without duplicates (the
//     table's last chunk is always in it); the launch's first workgroups check one chunk of the list each, one more compares the
//     table's last entry with the stream's length.  Their failures go to a call-wide status word: the table is then not this
//     stream's, for any window.
//   * STATUS  A word per window: a wave raises bits in the word of its window only, so one bad segment costs the windows that hold
//     it the shortcut and leaves the others alone.
#include "qb3_win.h"

namespace qb3dev {

template <int B, bool RGB, uint64_t ORDER, bool STEP>
__global__ void __launch_bounds__(256) dec_wins_kernel(const WinBatchArgs ba) {
    const DecArgs &a = ba.d;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (blockIdx.x < ba.chk_n) {                        // the launch's first workgroups: a chunk of the container's table each
        ix_check_chunk(a, ba.chunks[blockIdx.x], (uint32_t *)smem);
        return;
    }
    if (blockIdx.x < ba.chk_n + ba.tail) {              // ... and one for the table's end
        if (threadIdx.x == 0) ix_tail_check(a);
        return;
    }
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t gw = (blockIdx.x - ba.chk_n - ba.tail) * 4 + wave;      // (wave uniform, as is all of the search)
    // the last window whose first wave is not behind gw (wave0 grows strictly: every window has a wave; window 0 starts at 0).
    // A wave behind the last window's waves lands in the last window and leaves there (wid >= nwaves).
    uint32_t lo = 0, hi = ba.nwin;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ba.wins[mid].wave0 <= gw) lo = mid; else hi = mid;
    }
    lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    const WinDesc w = ba.wins[lo];                      // sixteen dwords, read before anything is stored
    win_decode_wave<B, RGB, ORDER, STEP>(a, w, ba.wstatus + lo, smem, wave, gw - w.wave0);
}

template <int B, bool RGB>
static void launch_dec_wins_b(const WinBatchArgs &ba, dim3 grid, size_t lds, hipStream_t st) {
    const bool step = ba.d.g.mode != CM_FTL, z = ba.d.g.order == ZCURVE;
    const dim3 block(256);
    if (!z && !step) hipLaunchKernelGGL((dec_wins_kernel<B, RGB, HILBERT, false>), grid, block, lds, st, ba);
    else if (!z && step) hipLaunchKernelGGL((dec_wins_kernel<B, RGB, HILBERT, true>), grid, block, lds, st, ba);
    else if (z && !step) hipLaunchKernelGGL((dec_wins_kernel<B, RGB, ZCURVE, false>), grid, block, lds, st, ba);
    else hipLaunchKernelGGL((dec_wins_kernel<B, RGB, ZCURVE, true>), grid, block, lds, st, ba);
}

size_t window_batch_plan(const Geometry &g, const IxTable &ix, const WinRect *rects, void *const *dsts, size_t n, void *descs,
                         std::vector<uint32_t> &chunks, uint64_t *segments) {
    WinDesc *d = (WinDesc *)descs;
    const bool checked = ix.version >= 3 || ix.check_heads;
    uint64_t waves = 0, segs = 0;
    chunks.clear();
    for (size_t i = 0; i < n; i++) {
        window_desc(g, rects[i], dsts[i], &d[i]);
        // a launch ends in front of the window that would take it beyond WIN_LAUNCH_WAVES; the prefix starts again there
        if (waves && waves + d[i].nwaves > WIN_LAUNCH_WAVES) waves = 0;
        d[i].wave0 = (uint32_t)waves;
        waves += d[i].nwaves;
        segs += window_segments(g, rects[i]);
        if (checked) {      // table chunks an entry is read from: the first segment's to the one of the entry behind the last segment
            const uint64_t first = ((uint64_t)d[i].by0 * g.nbx + d[i].bx0) / g.seg_blocks, last = std::min<uint64_t>(((uint64_t)d[i].by1 * g.nbx + d[i].bx1) / g.seg_blocks + 1, ix.K - 1);
            for (uint64_t c = first / ix.per_chunk; c <= last / ix.per_chunk; c++) chunks.push_back((uint32_t)c);
        }
    }
    if (checked) {
        chunks.push_back((ix.K - 1) / ix.per_chunk);    // the tail check reads the table's last entry
        std::sort(chunks.begin(), chunks.end());
        chunks.erase(std::unique(chunks.begin(), chunks.end()), chunks.end());
    }
    if (segments) *segments = segs;
    return chunks.size();
}

int launch_decode_windows(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                          const void *h_descs, const void *d_descs, size_t n, const uint32_t *d_chunks, size_t nchunks,
                          uint32_t *d_status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_ok(g, plan, ix) || !n) { set_error("window batch: not for this raster", 0); return -1; }
    WinBatchArgs ba = {};
    window_dec_args(ba.d, g, plan, in32, in_bit0, in_bits, d_status, ix);
    window_batch_launches(ba, h_descs, d_descs, n, d_chunks, nchunks, d_status, [&](const WinBatchArgs &ba, dim3 grid) {
        ProfScope ps("dec_window", st);
        if (g.bands == 1) launch_dec_wins_b<1, false>(ba, grid, plan.lds_px, st);
        else if (g.bands == 3) { if (plan.px_rgb) launch_dec_wins_b<3, true>(ba, grid, plan.lds_px, st); else launch_dec_wins_b<3, false>(ba, grid, plan.lds_px, st); }
        else { if (plan.px_rgb) launch_dec_wins_b<4, true>(ba, grid, plan.lds_px, st); else launch_dec_wins_b<4, false>(ba, grid, plan.lds_px, st); }
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
