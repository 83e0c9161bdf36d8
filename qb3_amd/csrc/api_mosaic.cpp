// qb3_amd/csrc/api_mosaic.cpp -- a raster in device memory as a grid of independently coded tiles (include/qb3x.h, "Mosaics"):
// qb3x_encode_mosaic codes the tiles where they lie in the raster, qb3x_decode_mosaic decodes them back into place.  The tiles wholly
// inside the raster are one grid of the tile batcher (api_tiles.cpp: TileGrid), read or written through the raster's stride; the tiles
// that cross the right or bottom edge -- at most tx + ty - 1 -- are a row and a column of tiles in memory of the handle's, which one
// launch of k_mosaic.hip fills from the raster (edge replication) or copies back into it (clipped).
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

QB3_API size_t qb3x_mosaic_tiles(size_t W, size_t H, size_t tw, size_t th, size_t *tx, size_t *ty) {
    if (!W || !H || !tw || !th) return 0;
    const size_t nx = (W - 1) / tw + 1, ny = (H - 1) / th + 1;
    if (tx) *tx = nx;
    if (ty) *ty = ny;
    return nx * ny;
}

namespace {

// The grids of a mosaic and the copies of its edge tiles.  Order: the inside, the bottom row (without the corner when there is a right
// column), the right column -- so that the call's last tile is the raster's last, whose band state an encoder handle is left with.
struct MosaicPlan {
    size_t tx, ty, ngrids = 0, nedge = 0, tile_pitch = 0, desc_bytes = 0;
    TileGrid grids[3];
    std::vector<MosaicRect> rects;          // pad: raster -> tile; crop: the same with the two ends exchanged
    uint32_t max_rows = 0;
};

// raster: its first value; scratch: the handle's memory (null: only sizes are wanted); stride in values, not 0
MosaicPlan mosaic_plan(size_t W, size_t H, size_t tw, size_t th, size_t bands, size_t tsz, const void *raster, size_t stride, uint8_t *scratch, bool pad) {
    MosaicPlan m;
    qb3x_mosaic_tiles(W, H, tw, th, &m.tx, &m.ty);
    const size_t txi = W / tw, tyi = H / th, pb = bands * tsz;
    const size_t nbottom = m.ty > tyi ? txi : 0, nright = m.tx > txi ? m.ty : 0;
    m.nedge = nbottom + nright;
    m.tile_pitch = (tw * th * pb + 15) & ~(size_t)15;
    m.desc_bytes = (m.nedge * MOSAIC_RECT_BYTES + 255) & ~(size_t)255;
    uint8_t *tiles = scratch ? scratch + m.desc_bytes : nullptr;
    if (txi && tyi) m.grids[m.ngrids++] = TileGrid{ txi * tyi, txi, raster, tw * pb, th * stride * tsz, stride, 0, m.tx };
    if (nbottom) m.grids[m.ngrids++] = TileGrid{ nbottom, nbottom, tiles, m.tile_pitch, 0, 0, (m.ty - 1) * m.tx, 0 };
    if (nright) m.grids[m.ngrids++] = TileGrid{ nright, 1, tiles + nbottom * m.tile_pitch, m.tile_pitch, m.tile_pitch, 0, m.tx - 1, m.tx };
    for (size_t s = 0; s < m.nedge && scratch; s++) {
        const size_t i = s < nbottom ? s : m.tx - 1, j = s < nbottom ? m.ty - 1 : s - nbottom;
        const uint32_t cw = (uint32_t)(std::min(tw, W - i * tw) * pb), ch = (uint32_t)std::min(th, H - j * th);
        uint8_t *in_raster = (uint8_t *)const_cast<void *>(raster) + (j * th * stride + i * tw * bands) * tsz, *tile = tiles + s * m.tile_pitch;
        if (pad) m.rects.push_back(MosaicRect{ in_raster, stride * tsz, tile, tw * pb, cw, ch, (uint32_t)(tw * pb), (uint32_t)th });
        else m.rects.push_back(MosaicRect{ tile, tw * pb, in_raster, stride * tsz, cw, ch, cw, ch });
        m.max_rows = std::max(m.max_rows, pad ? (uint32_t)th : ch);
    }
    return m;
}

bool raster_ok(const void *d_raster, size_t W, size_t H, size_t stride, size_t bands) {
    return d_raster && W && H && W <= 0xffffffffull && H <= 0xffffffffull && (!stride || stride >= W * bands);
}

// descriptors up, then the one launch (the copy is from pageable memory: the runtime has taken the bytes when it returns)
bool edge_launch(const MosaicPlan &m, void *d_scratch, size_t pb, bool pad, hipStream_t st) {
    if (hipMemcpyAsync(d_scratch, m.rects.data(), m.nedge * MOSAIC_RECT_BYTES, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("mosaic: descriptors", 0); return false; }
    return 0 == launch_mosaic_rects(d_scratch, m.nedge, m.max_rows, (uint32_t)pb, pad, st);
}

size_t encode_mosaic_body(encsp p, const void *d_raster, size_t W, size_t H, size_t raster_stride, void *d_dst, size_t dst_pitch,
                          void *d_index, size_t *sizes, void *stream) {
    if (!p) return 0;
    if (!d_dst || !sizes || (dst_pitch & 3) || ((uintptr_t)d_dst & 3) || !raster_ok(d_raster, W, H, raster_stride, p->nbands)) { p->error = QB3E_EINV; return 0; }
    const size_t tsz = szof(p->type), stride = raster_stride ? raster_stride : W * p->nbands;
    hipStream_t st = (hipStream_t)stream;
    MosaicPlan m = mosaic_plan(W, H, p->xsize, p->ysize, p->nbands, tsz, d_raster, stride, nullptr, true);
    if (m.nedge) {
        if (!device_ok() || !p->d_mos.ensure(m.desc_bytes + m.nedge * m.tile_pitch)) { p->error = QB3E_LIBERR; return 0; }
        m = mosaic_plan(W, H, p->xsize, p->ysize, p->nbands, tsz, d_raster, stride, (uint8_t *)p->d_mos.p, true);
        if (!edge_launch(m, p->d_mos.p, p->nbands * tsz, true, st)) { p->error = QB3E_LIBERR; return 0; }
    }
    return encode_tile_grids(p, m.grids, m.ngrids, d_dst, dst_pitch, d_index, sizes, stream);
}

size_t decode_mosaic_body(decsp p, const void *d_src, size_t src_pitch, const size_t *sizes, size_t W, size_t H, void *d_raster,
                          size_t raster_stride, const void *d_index, void *stream) {
    if (!p || !d_src || !sizes || (src_pitch & 3) || ((uintptr_t)d_src & 3) || !raster_ok(d_raster, W, H, raster_stride, p->nbands)) return 0;
    if (p->stage != 2 || p->error != QB3E_OK) return 0;
    const size_t tsz = szof(p->type), stride = raster_stride ? raster_stride : W * p->nbands;
    hipStream_t st = (hipStream_t)stream;
    MosaicPlan m = mosaic_plan(W, H, p->xsize, p->ysize, p->nbands, tsz, d_raster, stride, nullptr, false);
    if (m.nedge) {
        if (!device_ok() || !p->d_mos.ensure(m.desc_bytes + m.nedge * m.tile_pitch)) { p->error = QB3E_LIBERR; return 0; }
        m = mosaic_plan(W, H, p->xsize, p->ysize, p->nbands, tsz, d_raster, stride, (uint8_t *)p->d_mos.p, false);
    }
    const size_t done = decode_tile_grids(p, d_src, m.tx * m.ty, src_pitch, sizes, m.grids, m.ngrids, d_index, stream);
    if (m.nedge && p->error == QB3E_OK && device_ok()) {
        // (a tile that failed leaves its own rectangle unspecified: whatever its scratch tile holds goes there, nothing goes anywhere else)
        bool ok = edge_launch(m, p->d_mos.p, p->nbands * tsz, false, st);
        if (ok && hipStreamSynchronize(st) != hipSuccess) { set_error("mosaic crop", 0); ok = false; }
        prof_collect();
        if (!ok) { p->error = QB3E_LIBERR; return 0; }
    }
    return done;
}

}  // namespace

QB3_API size_t qb3x_encode_mosaic(encsp p, const void *d_raster, size_t W, size_t H, size_t raster_stride,
                                  void *d_dst, size_t dst_pitch, void *d_index, size_t *sizes, void *stream) {
    return abi_guard<size_t>(0, [&] { return encode_mosaic_body(p, d_raster, W, H, raster_stride, d_dst, dst_pitch, d_index, sizes, stream); });
}

QB3_API size_t qb3x_decode_mosaic(decsp p, const void *d_src, size_t src_pitch, const size_t *sizes, size_t W, size_t H,
                                  void *d_raster, size_t raster_stride, const void *d_index, void *stream) {
    return abi_guard<size_t>(0, [&] { return decode_mosaic_body(p, d_src, src_pitch, sizes, W, H, d_raster, raster_stride, d_index, stream); });
}
