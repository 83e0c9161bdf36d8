// qb3_amd/csrc/k_mosaic.hip -- the edge tiles of a mosaic (api_mosaic.cpp).  The tiles that lie inside the raster are coded and decoded
// where they are; the at most tx + ty - 1 tiles that cross its right or bottom edge go through memory of the handle's: the encoder codes
// their replicated images from there ("mosaic_pad" builds them), the decoder writes whole tiles there ("mosaic_crop" copies the part
// inside the raster out).  Both are the same copy, described by MosaicRect (qb3_dev.h), and ONE launch each however many edge tiles:
//   * MAPPING  blockIdx.x walks the rectangles, blockIdx.y the destination rows of one, the workgroup's lanes run along a row.  A row
//     whose ends and pitches are all on sixteen bytes moves sixteen bytes a lane (consecutive lanes, consecutive lines); the bytes behind
//     the last whole sixteen, every row of any other rectangle, and the replicated pixels go byte by byte, consecutive lanes on consecutive
//     bytes.  Pure bandwidth over a few percent of a raster: nothing cleverer is warranted ("Mosaics").
//   * BOUNDS   source: rows [0, ch), bytes [0, cw) of each; destination: rows [0, oh), bytes [0, ow) of each.  Nothing else is touched:
//     the gaps of a raster's stride and whatever lies behind its last row stay as they are.
#include "qb3_kernels.h"

namespace qb3dev {

static_assert(sizeof(MosaicRect) == MOSAIC_RECT_BYTES, "MosaicRect goes up as the host wrote it");

__global__ void __launch_bounds__(256) mosaic_rect_kernel(const MosaicRect *descs, uint32_t n, uint32_t pb) {
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const MosaicRect d = descs[i];
        const bool v16 = !(((uintptr_t)d.src | (uintptr_t)d.dst | d.spitch | d.dpitch) & 15);
        const uint32_t nvec = v16 ? d.cw >> 4 : 0;
        for (uint32_t y = blockIdx.y; y < d.oh; y += gridDim.y) {
            const uint8_t *s = (const uint8_t *)d.src + (uint64_t)(y < d.ch ? y : d.ch - 1) * d.spitch;
            uint8_t *o = (uint8_t *)d.dst + (uint64_t)y * d.dpitch;
            for (uint32_t x = threadIdx.x; x < nvec; x += blockDim.x) ((uint4 *)o)[x] = ((const uint4 *)s)[x];
            for (uint32_t x = 16 * nvec + threadIdx.x; x < d.ow; x += blockDim.x)
                o[x] = s[x < d.cw ? x : d.cw - pb + (x - d.cw) % pb];         // (behind the rectangle: its last pixel again)
        }
    }
}

int launch_mosaic_rects(const void *d_descs, size_t n, uint32_t max_rows, uint32_t pixel_bytes, bool pad, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!d_descs || !n || n > 0xffffffffull || !pixel_bytes) { set_error("mosaic edge tiles: bad arguments", 0); return -1; }
    {
        ProfScope ps(pad ? "mosaic_pad" : "mosaic_crop", st);
        const dim3 grid((uint32_t)std::min<size_t>(n, 65535), std::min<uint32_t>(std::max<uint32_t>(max_rows, 1), 4096));
        hipLaunchKernelGGL(mosaic_rect_kernel, grid, dim3(256), 0, st, (const MosaicRect *)d_descs, (uint32_t)n, pixel_bytes);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
