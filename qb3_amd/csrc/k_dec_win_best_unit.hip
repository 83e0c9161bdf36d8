// qb3_amd/csrc/k_dec_win_best_unit.hip -- window decode of the common-factor rasters (QB3M_CF, QB3M_CF_H; QB3M_BEST / QB3M_CF_RLE where the
// RLE0 pass did not win) that the whole-raster decoders dec_pxu_best_kernel and dec_pxw_best_kernel take: 8-bit rasters of 2 or more than 4
// bands, 16/32/64-bit rasters of several bands, and one-band 16/32/64-bit rasters, from the container's restart table (level 1 or 2: the
// common-factor entries carry a three-byte field per unit at either).  What k_dec_win_unit.hip does for the FTL / BASE streams of such
// shapes -- only the index segments that hold a block of a window are decoded, only the window's bytes are written -- with the decoding of
// dec_pxu_best_kernel's BL branch (k_dec_pxu.hip): a wave per segment of 64 / bands blocks, a lane per unit.  The one-band entry
// (dec_pxw_best_kernel's, k_dec_pxw.hip) has the lane-per-unit layout with one band, so the same routine takes it.  The wave's work is
// winu_best_decode_wave (qb3_win_best_unit.h); mapping, de-duplication, trust and status are described at the head of k_dec_win.hip and
// hold here with the raster's blocks per segment in place of 64.  What differs from k_dec_win_unit.hip:
//   * THE ENTRY  carries, besides position and entering values, the FACTOR each band is entered with, and per unit its bits | the rung it
//     is entered with << 12: a common-factor unit leaves its band at the rung of the multiplied values, so rungs are not a scan of the
//     switch codes.  Inside the segment the factor in force is the band's nearest writer among the lanes below, found by a ballot; before
//     the first writer it is the entry's.
//   * NO CODE TABLE, NO BARRIER  The common-factor parser reads the stream with the branchy reader and no table in LDS: the launch brings
//     four waves' worst-case staging and nothing else, and the waves share nothing.
//   * TRUST  Every consistency test of dec_pxu_best_kernel stays: a unit's leaving rung against the band's next unit's entering rung, the
//     end of a unit against its length, a malformed unit.  An entry's entering VALUE or FACTOR that was changed under a re-sealed check is
//     detected by neither this kernel nor the whole decode from the table: both give the same wrong pixels.
// Two kernel families, as for the FTL / BASE streams: dec_winbu_kernel takes its window as kernel arguments, dec_winsbu_kernel finds it in
// the batch's descriptor array.  The host takes them only for handles that asked (qb3x_set_decoder_window_kernels, QB3X_WINK_CFU) and only
// for value-aligned destinations.
#include "qb3_win_best_unit.h"

namespace qb3dev {

template <typename T>
__global__ void __launch_bounds__(256) dec_winbu_kernel(const WinArgs wa) {
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
    winu_best_decode_wave<T>(a, wa.w, a.status, smem, wave, (blockIdx.x - wa.chk_n - 1) * 4 + wave);
}

template <typename T>
__global__ void __launch_bounds__(256) dec_winsbu_kernel(const WinBatchArgs ba) {
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
    winu_best_decode_wave<T>(a, w, ba.wstatus + lo, smem, wave, gw - w.wave0);
}

// one place names the instantiations: KERNEL<T> by the raster's value size
#define QB3_WINBU_DISPATCH(KERNEL, args)                                                                                    \
    do {                                                                                                                    \
        const size_t lds = window_best_unit_lds_bytes(g, plan);                                                             \
        switch (g.tsz) {                                                                                                    \
        case 1: hipLaunchKernelGGL((KERNEL<uint8_t>), grid, dim3(256), lds, st, args); break;                               \
        case 2: hipLaunchKernelGGL((KERNEL<uint16_t>), grid, dim3(256), lds, st, args); break;                              \
        case 4: hipLaunchKernelGGL((KERNEL<uint32_t>), grid, dim3(256), lds, st, args); break;                              \
        default: hipLaunchKernelGGL((KERNEL<uint64_t>), grid, dim3(256), lds, st, args); break;                             \
        }                                                                                                                   \
    } while (0)

bool decode_window_best_unit_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    const DecKernel k = aligned_dec_kernel(g, plan);
    return decode_strips_ok(g, plan, ix) && (k == DecKernel::pxu_best || k == DecKernel::pxw_best) && g.seg_blocks * g.bands <= 64 &&
           ix.block_lens && ix.version >= 3 && window_unit_geometry_ok(g);
}

int launch_decode_window_best_unit(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                                   void *dst, const WinRect &r, uint32_t *status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_best_unit_ok(g, plan, ix) || !window_segments(g, r) || r.stride < (uint64_t)r.w * g.bands || ((uintptr_t)dst & (g.tsz - 1))) {
        set_error("common-factor lane-per-unit window decode: not for this raster", 0);
        return -1;
    }
    WinArgs wa = {};
    const dim3 grid(window_launch_args(wa, g, plan, in32, in_bit0, in_bits, dst, r, status, ix));
    window_unit_dec_args(wa.d, plan);
    HIPCHK(hipMemsetAsync(status, 0, 4, st));
    {
        ProfScope ps("dec_window_best_unit", st);
        QB3_WINBU_DISPATCH(dec_winbu_kernel, wa);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_decode_windows_best_unit(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                                    const void *h_descs, const void *d_descs, size_t n, const uint32_t *d_chunks, size_t nchunks,
                                    uint32_t *d_status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_best_unit_ok(g, plan, ix) || !n) { set_error("common-factor lane-per-unit window batch: not for this raster", 0); return -1; }
    WinBatchArgs args = {};
    window_dec_args(args.d, g, plan, in32, in_bit0, in_bits, d_status, ix);
    window_unit_dec_args(args.d, plan);
    window_batch_launches(args, h_descs, d_descs, n, d_chunks, nchunks, d_status, [&](const WinBatchArgs &ba, dim3 grid) {
        ProfScope ps("dec_window_best_unit", st);
        QB3_WINBU_DISPATCH(dec_winsbu_kernel, ba);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
