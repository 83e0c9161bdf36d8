// qb3_amd/csrc/k_dec_win16.hip -- window decode of 16-bit rasters of 1, 2, 3, 4, 6 or 8 bands (FTL / BASE) from the container's level-2
// restart table: what k_dec_win.hip and k_dec_wins.hip do for 8-bit rasters -- only the index segments that hold a block of a window
// are decoded, only the window's bytes are written -- with the decoding of dec_px16_kernel's BL branch (k_dec_px16.hip): a wave per
// segment of 64 / band groups blocks, a lane per block and band group.  The wave's work is win16_decode_wave (qb3_win16.h); mapping,
// de-duplication, clipping, trust and status are described at the head of k_dec_win.hip and hold here with the raster's blocks per
// segment in place of 64.  What differs:
//   * STAGING  The launch brings LDS for the worst-case segment (the plan's px_cap_dw), so there is no "sized for this stream's average,
//     run again" status: a segment that does not fit is not this stream's.
//   * STORES  A lane holds BG bands of its block's pixels.  A block wholly inside the window's columns stores dwords, the form chosen
//     row by row from the address (a row on a dword; a row off by a halfword: head halfword, aligned dwords, tail halfword); the two
//     lanes of an eight-band block swap halves and store 32 contiguous bytes each where the row lies on a 16-byte address.  An edge
//     block stores halfwords one by one under the column mask.
// Two kernel families, as for 8-bit data: dec_win16_kernel takes its window as kernel arguments (no descriptor goes up for a single
// call), dec_wins16_kernel finds it in the batch's descriptor array.  The host takes them only for handles that asked
// (qb3x_set_decoder_window_kernels, QB3X_WINK_U16) and only for halfword-aligned destinations.
#include "qb3_win16.h"

namespace qb3dev {

template <int BG, bool RGB, uint64_t ORDER, bool STEP>
__global__ void __launch_bounds__(256, 4) dec_win16_kernel(const WinArgs wa) {
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
    win16_decode_wave<BG, RGB, ORDER, STEP>(a, wa.w, a.status, smem, wave, (blockIdx.x - wa.chk_n - 1) * 4 + wave);
}

template <int BG, bool RGB, uint64_t ORDER, bool STEP>
__global__ void __launch_bounds__(256, 4) dec_wins16_kernel(const WinBatchArgs ba) {
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
    win16_decode_wave<BG, RGB, ORDER, STEP>(a, w, ba.wstatus + lo, smem, wave, gw - w.wave0);
}

bool decode_window16_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    return decode_strips_ok(g, plan, ix) && aligned_dec_kernel(g, plan) == DecKernel::px16 && ix.block_lens && ix.version >= 3 && g.nblocks < (1ull << 31);
}

int launch_decode_window16(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                           void *dst, const WinRect &r, uint32_t *status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window16_ok(g, plan, ix) || !window_segments(g, r) || r.stride < (uint64_t)r.w * g.bands || ((uintptr_t)dst & 1)) {
        set_error("16-bit window decode: not for this raster", 0);
        return -1;
    }
    WinArgs wa = {};
    const dim3 grid(window_launch_args(wa, g, plan, in32, in_bit0, in_bits, dst, r, status, ix));
    window16_dec_args(wa.d, plan);
    HIPCHK(hipMemsetAsync(status, 0, 4, st));
    {
        ProfScope ps("dec_window16", st);
        QB3_WIN16_DISPATCH(dec_win16_kernel, wa);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_decode_windows16(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                            const void *h_descs, const void *d_descs, size_t n, const uint32_t *d_chunks, size_t nchunks,
                            uint32_t *d_status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window16_ok(g, plan, ix) || !n) { set_error("16-bit window batch: not for this raster", 0); return -1; }
    WinBatchArgs args = {};
    window_dec_args(args.d, g, plan, in32, in_bit0, in_bits, d_status, ix);
    window16_dec_args(args.d, plan);
    window_batch_launches(args, h_descs, d_descs, n, d_chunks, nchunks, d_status, [&](const WinBatchArgs &ba, dim3 grid) {
        ProfScope ps("dec_window16", st);
        QB3_WIN16_DISPATCH(dec_wins16_kernel, ba);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
