// qb3_amd/csrc/k_dec_win_best.hip -- window decode of 8-bit grey / RGB / RGBA rasters in the common-factor modes (QB3M_CF, QB3M_CF_H;
// QB3M_BEST / QB3M_CF_RLE where the RLE0 pass did not win) from the container's restart table: what k_dec_win.hip and k_dec_wins.hip do
// for FTL / BASE rasters -- only the index segments that hold a block of a window are decoded, only the window's bytes are written --
// with the decoding of dec_px_best_kernel's BL branch (k_dec_px_best.hip).  The wave's work is win_best_decode_wave (qb3_win_best.h);
// mapping, de-duplication, clipping, trust and status are described at the head of k_dec_win.hip and hold here.  What differs:
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
// Two kernel families, as for FTL / BASE data: dec_win_best_kernel takes its window as kernel arguments, dec_wins_best_kernel finds it in
// the batch's descriptor array.  The host takes them only for handles that asked (qb3x_set_decoder_window_kernels, QB3X_WINK_CF8).
// Destinations need no alignment: the stores are win_decode_wave's.
#include "qb3_win_best.h"

namespace qb3dev {

template <int B, bool RGB, uint64_t ORDER>
__global__ void __launch_bounds__(256, win_best_waves(B)) dec_win_best_kernel(const WinArgs wa) {
    const DecArgs &a = wa.d;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (blockIdx.x < wa.chk_n) {                        // the launch's first workgroups: a chunk of the container's table each
        ix_check_chunk(a, wa.chk0 + blockIdx.x, (uint32_t *)smem);
        return;
    }
    if (blockIdx.x == wa.chk_n) {                       // ... and one for the table's end
        if (wa.tail_chunk) ix_check_chunk(a, (a.ix_K - 1) / a.ix_per_chunk, (uint32_t *)smem);
        if (threadIdx.x == 0) ix_tail_check(a);
        return;
    }
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // (wave uniform: what follows from it stays in scalar registers)
    win_best_decode_wave<B, RGB, ORDER>(a, wa.w, a.status, smem, wave, (blockIdx.x - wa.chk_n - 1) * 4 + wave);
}

template <int B, bool RGB, uint64_t ORDER>
__global__ void __launch_bounds__(256, win_best_waves(B)) dec_wins_best_kernel(const WinBatchArgs ba) {
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
    // the last window whose first wave is not behind gw, as dec_wins_kernel finds it
    uint32_t lo = 0, hi = ba.nwin;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ba.wins[mid].wave0 <= gw) lo = mid; else hi = mid;
    }
    lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    const WinDesc w = ba.wins[lo];                      // sixteen dwords, read before anything is stored
    win_best_decode_wave<B, RGB, ORDER>(a, w, ba.wstatus + lo, smem, wave, gw - w.wave0);
}

bool decode_window_best_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    return decode_strips_ok(g, plan, ix) && aligned_dec_kernel(g, plan) == DecKernel::px_best && g.seg_blocks == 64 && g.nblocks < (1ull << 31);
}

int launch_decode_window_best(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                              void *dst, const WinRect &r, uint32_t *status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_best_ok(g, plan, ix) || !window_segments(g, r) || r.stride < (uint64_t)r.w * g.bands) {
        set_error("common-factor window decode: not for this raster", 0);
        return -1;
    }
    WinArgs wa = {};
    const dim3 grid(window_launch_args(wa, g, plan, in32, in_bit0, in_bits, dst, r, status, ix));
    HIPCHK(hipMemsetAsync(status, 0, 4, st));
    {
        ProfScope ps("dec_window_best", st);
        QB3_WIN_BEST_DISPATCH(dec_win_best_kernel, wa);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_decode_windows_best(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                               const void *h_descs, const void *d_descs, size_t n, const uint32_t *d_chunks, size_t nchunks,
                               uint32_t *d_status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_best_ok(g, plan, ix) || !n) { set_error("common-factor window batch: not for this raster", 0); return -1; }
    WinBatchArgs args = {};
    window_dec_args(args.d, g, plan, in32, in_bit0, in_bits, d_status, ix);
    window_batch_launches(args, h_descs, d_descs, n, d_chunks, nchunks, d_status, [&](const WinBatchArgs &ba, dim3 grid) {
        ProfScope ps("dec_window_best", st);
        QB3_WIN_BEST_DISPATCH(dec_wins_best_kernel, ba);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
