// qb3_amd/csrc/k_win_bands.hip -- band-selected windows where no window kernel writes the selection itself: full-band pixels lie in memory
// of the handle's (tight windows a window kernel wrote, or the scratch raster of a strip or a whole decode), and ONE launch picks the
// selected bands of every window a path produced into the caller's buffers.  It takes the place of the crop (hipMemcpy2DAsync) of the
// full-band calls.
//   * MAPPING  blockIdx.x walks the windows, blockIdx.y the rows of one, the workgroup's lanes run along the w * nsel values of an output
//     row: lane j writes slot j % nsel of pixel j / nsel, which is band sel[slot] of the source pixel.  Consecutive lanes write consecutive
//     values; they read values at most `sbands` apart, from lines the row's other lanes read too.
//   * ANY DESTINATION  A window whose first byte and row distance are multiples of the value size stores whole values, any other bytes.
//     The source is the handle's own: always value aligned.
//   * NOTHING ELSE IS WRITTEN  h runs of w * nsel values a window.
// This is the simple version (a value a lane, the selection in kernel arguments); DESIGN.md says what a wider one would be measured against.
#include "qb3_kernels.h"

namespace qb3dev {

static_assert(sizeof(WinGather) == WIN_GATHER_BYTES, "WinGather goes up as the host wrote it");

// reference QB3decode.cpp:77-107, as dequantize_kernel (k_host.hip) has it: multiply back, saturating
template <typename TS> __device__ __forceinline__ TS win_gather_scale(TS v, TS q) {
    constexpr bool is_signed = (TS)-1 < (TS)0;
    constexpr TS tmax = is_signed ? (TS)(((uint64_t)1 << (8 * sizeof(TS) - 1)) - 1) : (TS)~(TS)0;
    constexpr TS tmin = is_signed ? (TS)((uint64_t)1 << (8 * sizeof(TS) - 1)) : (TS)0;
    const TS mai = (TS)(tmax / q), mii = (TS)(tmin / q);
    TS r = (v <= mai) ? (TS)(v * q) : tmax;
    if (is_signed && q > 2 && v < mii) r = tmin;
    return r;
}

template <typename TS>
__global__ void __launch_bounds__(256) win_band_gather_kernel(const WinGather *descs, uint32_t n, uint64_t sel_nibs, uint32_t nsel, uint64_t quanta) {
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const WinGather d = descs[i];
        const uint32_t rowvals = d.w * nsel;            // (below 2^32: the host refuses a wider row)
        const bool whole = (((uintptr_t)d.dst | d.dstride) & (sizeof(TS) - 1)) == 0;
        for (uint32_t y = blockIdx.y; y < d.h; y += gridDim.y) {
            const TS *src = (const TS *)((const uint8_t *)d.src + (uint64_t)y * d.spitch);
            uint8_t *row = (uint8_t *)d.dst + (uint64_t)y * d.dstride;
            for (uint32_t j = threadIdx.x; j < rowvals; j += blockDim.x) {
                const uint32_t px = j / nsel, k = j - px * nsel;
                TS v = src[(uint64_t)px * d.sbands + ((uint32_t)(sel_nibs >> (4 * k)) & 15u)];
                if (quanta > 1) v = win_gather_scale<TS>(v, (TS)quanta);
                if (whole) ((TS *)row)[j] = v;
                else {
#pragma unroll
                    for (uint32_t b = 0; b < sizeof(TS); b++) row[(uint64_t)j * sizeof(TS) + b] = (uint8_t)((uint64_t)v >> (8 * b));
                }
            }
        }
    }
}

template <typename TS>
static void gather_launch(const void *d_descs, size_t n, uint64_t max_rows, uint64_t nibs, uint32_t nsel, uint64_t q, hipStream_t st) {
    const dim3 grid((uint32_t)std::min<size_t>(n, 65535), (uint32_t)std::min<uint64_t>(std::max<uint64_t>(max_rows, 1), 4096));
    hipLaunchKernelGGL(win_band_gather_kernel<TS>, grid, dim3(256), 0, st, (const WinGather *)d_descs, (uint32_t)n, nibs, nsel, q);
}

int launch_window_gather(const void *d_descs, size_t n, uint64_t max_rows, const uint8_t *sel, uint32_t nsel, int dtype, uint64_t quanta, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!d_descs || !n || n > 0xffffffffull || !sel || !nsel || nsel > (uint32_t)MAXBANDS) { set_error("window band gather: bad arguments", 0); return -1; }
    uint64_t nibs = 0;
    for (uint32_t k = 0; k < nsel; k++) nibs |= (uint64_t)(sel[k] & 15u) << (4 * k);
    {
        ProfScope ps("win_band_gather", st);
        switch (dtype) {
        case 0: gather_launch<uint8_t>(d_descs, n, max_rows, nibs, nsel, quanta, st); break;
        case 1: gather_launch<int8_t>(d_descs, n, max_rows, nibs, nsel, quanta, st); break;
        case 2: gather_launch<uint16_t>(d_descs, n, max_rows, nibs, nsel, quanta, st); break;
        case 3: gather_launch<int16_t>(d_descs, n, max_rows, nibs, nsel, quanta, st); break;
        case 4: gather_launch<uint32_t>(d_descs, n, max_rows, nibs, nsel, quanta, st); break;
        case 5: gather_launch<int32_t>(d_descs, n, max_rows, nibs, nsel, quanta, st); break;
        case 6: gather_launch<uint64_t>(d_descs, n, max_rows, nibs, nsel, quanta, st); break;
        case 7: gather_launch<int64_t>(d_descs, n, max_rows, nibs, nsel, quanta, st); break;
        default: set_error("window band gather: bad type", 0); return -1;
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
