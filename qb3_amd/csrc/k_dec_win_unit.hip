// qb3_amd/csrc/k_dec_win_unit.hip -- window decode of the rasters of the lane-per-unit decoder (8-bit rasters of 2 or more than 4 bands,
// 16-bit rasters of an odd band count above 4, 32/64-bit rasters of several bands) and of one-band 32/64-bit rasters, FTL / BASE, from the
// container's level-2 restart table: what k_dec_win.hip and k_dec_wins.hip do for 8-bit grey / RGB / RGBA rasters -- only the index
// segments that hold a block of a window are decoded, only the window's bytes are written -- with the decoding of dec_pxu_kernel's BL
// branch (k_dec_pxu.hip): a wave per segment of 64 / bands blocks, a lane per unit.  The one-band 32/64-bit entry (dec_pxw_kernel's,
// k_dec_pxw.hip) has the lane-per-unit layout with one band, so the same routine takes it.  The wave's work is winu_decode_wave
// (qb3_win_unit.h); mapping, de-duplication, trust and status are described at the head of k_dec_win.hip and hold here with the raster's
// blocks per segment in place of 64.  What differs:
//   * STAGING  The launch brings LDS for the worst-case segment (the plan's px_cap_dw), so there is no "sized for this stream's average,
//     run again" status: a segment that does not fit is not this stream's.
//   * STORES  The lanes write their values into the wave's LDS tile, laid out like the image ([row][block][x][band]), once every lane
//     holds its sixteen values.  A block whose four columns are its own and the window's stores its rows -- those that are its own and
//     the window's -- in pieces of 16, 8 or 4 bytes at value-aligned addresses; an edge block stores value by value under its column
//     mask.  A lane finds the numbers of the block it stores for (offset in the window, row and column masks) by a shuffle from the lane
//     of that block's number.
// Two kernel families, as for 8-bit data: dec_winu_kernel takes its window as kernel arguments, dec_winsu_kernel finds it in the batch's
// descriptor array.  The host takes them only for handles that asked (qb3x_set_decoder_window_kernels, QB3X_WINK_UNIT) and only for
// value-aligned destinations.
#include "qb3_win_unit.h"

namespace qb3dev {

template <typename T, bool STEP>
__global__ void __launch_bounds__(256) dec_winu_kernel(const WinArgs wa) {
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
    winu_decode_wave<T, STEP>(a, wa.w, a.status, smem, wave, (blockIdx.x - wa.chk_n - 1) * 4 + wave);
}

template <typename T, bool STEP>
__global__ void __launch_bounds__(256) dec_winsu_kernel(const WinBatchArgs ba) {
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
    winu_decode_wave<T, STEP>(a, w, ba.wstatus + lo, smem, wave, gw - w.wave0);
}

// one place names the instantiations: KERNEL<T, STEP> by the raster's value size and mode
#define QB3_WINU_DISPATCH(KERNEL, args)                                                                                     \
    do {                                                                                                                    \
        const bool step = g.mode != CM_FTL;                                                                                 \
        const size_t lds = window_unit_lds_bytes(g, plan);                                                                  \
        auto go = [&](auto t) {                                                                                             \
            typedef decltype(t) T;                                                                                          \
            if (step) hipLaunchKernelGGL((KERNEL<T, true>), grid, dim3(256), lds, st, args);                                \
            else hipLaunchKernelGGL((KERNEL<T, false>), grid, dim3(256), lds, st, args);                                    \
        };                                                                                                                  \
        switch (g.tsz) {                                                                                                    \
        case 1: go(uint8_t()); break;                                                                                       \
        case 2: go(uint16_t()); break;                                                                                      \
        case 4: go(uint32_t()); break;                                                                                      \
        default: go(uint64_t()); break;                                                                                     \
        }                                                                                                                   \
    } while (0)

bool decode_window_unit_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    const DecKernel k = aligned_dec_kernel(g, plan);
    return decode_strips_ok(g, plan, ix) && (k == DecKernel::pxu || k == DecKernel::pxw) && g.seg_blocks * g.bands <= 64 &&
           ix.block_lens && ix.version >= 3 && window_unit_geometry_ok(g);
}

int launch_decode_window_unit(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                              void *dst, const WinRect &r, uint32_t *status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_unit_ok(g, plan, ix) || !window_segments(g, r) || r.stride < (uint64_t)r.w * g.bands || ((uintptr_t)dst & (g.tsz - 1))) {
        set_error("lane-per-unit window decode: not for this raster", 0);
        return -1;
    }
    WinArgs wa = {};
    const dim3 grid(window_launch_args(wa, g, plan, in32, in_bit0, in_bits, dst, r, status, ix));
    window_unit_dec_args(wa.d, plan);
    HIPCHK(hipMemsetAsync(status, 0, 4, st));
    {
        ProfScope ps("dec_window_unit", st);
        QB3_WINU_DISPATCH(dec_winu_kernel, wa);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_decode_windows_unit(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                               const void *h_descs, const void *d_descs, size_t n, const uint32_t *d_chunks, size_t nchunks,
                               uint32_t *d_status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_unit_ok(g, plan, ix) || !n) { set_error("lane-per-unit window batch: not for this raster", 0); return -1; }
    WinBatchArgs args = {};
    window_dec_args(args.d, g, plan, in32, in_bit0, in_bits, d_status, ix);
    window_unit_dec_args(args.d, plan);
    window_batch_launches(args, h_descs, d_descs, n, d_chunks, nchunks, d_status, [&](const WinBatchArgs &ba, dim3 grid) {
        ProfScope ps("dec_window_unit", st);
        QB3_WINU_DISPATCH(dec_winsu_kernel, ba);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
