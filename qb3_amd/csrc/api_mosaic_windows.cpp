// qb3_amd/csrc/api_mosaic_windows.cpp -- rectangles of a mosaic (include/qb3x.h, "Mosaic windows"): qb3x_decode_mosaic_windows cuts every
// window along the tile grid into PIECES, a piece the part of one window in one tile, and gives each piece its pixels by one of two routes:
//   kernel  the tile is of tile 0's kind and tile 0's handle is one the 8-bit window family takes: the pieces of all windows are ONE
//           descriptor array and ONE launch over many containers (k_dec_wins_mosaic.hip), straight into the windows; one status copy,
//           one wait.  Whether a tile is of tile 0's kind -- mode byte, "ix" tag, "DT" mark -- is asked by that launch, not by copies to
//           the host in front of it: a tile that is not fails its check as a damaged table does, and goes the other way;
//   whole   everything else, and every tile or piece the first route raised a status bit for: the touched tiles that need it, and no
//           others, are decoded whole into memory of the handle's (decode_tile_grids, a run of consecutive tiles a call), each at most
//           once, then ONE launch of the mosaic's crop copies the pieces out of them.
// Host loops and copies follow the touched tiles and the pieces, never the mosaic's tile count.
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

QB3_API size_t qb3x_mosaic_window_tiles(size_t W, size_t H, size_t tw, size_t th, size_t x0, size_t y0, size_t w, size_t h,
                                        size_t *i0, size_t *j0, size_t *i1, size_t *j1) {
    if (!W || !H || !tw || !th || !w || !h || x0 >= W || w > W - x0 || y0 >= H || h > H - y0) return 0;
    const size_t a = x0 / tw, b = (x0 + w - 1) / tw, c = y0 / th, d = (y0 + h - 1) / th;
    if (i0) *i0 = a;
    if (j0) *j0 = c;
    if (i1) *i1 = b;
    if (j1) *j1 = d;
    return (b - a + 1) * (d - c + 1);
}

namespace {

constexpr size_t MAX_PIECES = (size_t)1 << 20;

struct Piece {
    size_t k;                       // the tile, as the mosaic counts it
    uint32_t win, slot;             // the window; the tile among the call's touched tiles
    uint32_t x, y, w, h;            // the piece in the tile's pixels
    uint8_t *dst;                   // where it lies in its window
    uint64_t stride;                // values between its rows there
    bool whole, ok;                 // takes the whole-tile route; has its pixels
};

// what a call works on: the pieces of all windows in window order, the touched tiles sorted, without duplicates
struct Cut { std::vector<Piece> pcs; std::vector<size_t> touched; };

// every window along the tile grid (the caller has checked the windows; npieces: their pieces in all)
void cut_pieces(const decs *p, size_t W, size_t H, const qb3x_window *wins, size_t n, size_t npieces, Cut &cut) {
    const size_t tw = p->xsize, th = p->ysize, bands = p->nbands, tsz = szof(p->type);
    std::vector<Piece> &pcs = cut.pcs;
    std::vector<size_t> &touched = cut.touched;
    size_t tx = 0, ty = 0;
    qb3x_mosaic_tiles(W, H, tw, th, &tx, &ty);
    pcs.reserve(npieces);
    touched.reserve(npieces);
    for (size_t i = 0; i < n; i++) {
        const qb3x_window &w = wins[i];
        const uint64_t stride = w.dst_stride ? w.dst_stride : w.w * bands;
        size_t i0, j0, i1, j1;
        qb3x_mosaic_window_tiles(W, H, tw, th, w.x0, w.y0, w.w, w.h, &i0, &j0, &i1, &j1);
        for (size_t j = j0; j <= j1; j++)
            for (size_t ii = i0; ii <= i1; ii++) {
                const size_t px0 = std::max(w.x0, ii * tw), px1 = std::min(w.x0 + w.w, (ii + 1) * tw);
                const size_t py0 = std::max(w.y0, j * th), py1 = std::min(w.y0 + w.h, (j + 1) * th);
                Piece q;
                q.k = j * tx + ii; q.win = (uint32_t)i; q.slot = 0;
                q.x = (uint32_t)(px0 - ii * tw); q.y = (uint32_t)(py0 - j * th); q.w = (uint32_t)(px1 - px0); q.h = (uint32_t)(py1 - py0);
                q.dst = (uint8_t *)w.dst + ((py0 - w.y0) * stride + (px0 - w.x0) * bands) * tsz;
                q.stride = stride; q.whole = true; q.ok = false;
                pcs.push_back(q);
                touched.push_back(q.k);
            }
    }
    std::sort(touched.begin(), touched.end());
    touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
    for (Piece &q : pcs) q.slot = (uint32_t)(std::lower_bound(touched.begin(), touched.end(), q.k) - touched.begin());
}

// The window-kernel route: where tile 0's handle qualifies, every piece whose tile has a stream behind tile 0's header goes up; the
// pieces that come back clean have their pixels (whole = false, ok).  *segs: the segments the launch decoded.  false: a failure of
// the device or of memory -- p->error is set, nothing of the handle's stays in flight
bool kernel_route(decsp p, const void *d_src, size_t src_pitch, const size_t *sizes, Cut &cut, hipStream_t st, size_t *segs) {
    std::vector<Piece> &pcs = cut.pcs;
    const std::vector<size_t> &touched = cut.touched;
    const size_t tw = p->xsize, th = p->ysize, nt = touched.size();
    auto fail = [&]() -> bool { (void)hipStreamSynchronize(st); p->error = QB3E_LIBERR; return false; };
    const size_t hdr = (size_t)(p->s_in - p->s_start);
    const bool coded = p->mode != QB3M_STORED && tw >= 4 && th >= 4;
    if (!(coded && p->ix_K && p->ix_bl && p->ix_off && !is_rle_mode(p->mode) && p->quanta <= 1 && hdr >= 2 && hdr <= 0xffffffffull)) return true;
    const Geometry g = decoder_geometry(p, tw, th, 0);
    const WinSrc s = window_source(p, g, d_src);
    const WinKernels *fam = window_family(g, s.plan, s.ixt, p->win_kernels);
    std::vector<uint32_t> kp;                           // the pieces that go up
    if (fam && fam->mosaic && fam->align(g) == 1)
        for (size_t j = 0; j < pcs.size(); j++) if (sizes[pcs[j].k] > hdr) kp.push_back((uint32_t)j);
    if (kp.empty()) return true;
    {
        const size_t nk = kp.size();
        const uint32_t K = s.ixt.K, per_chunk = s.ixt.per_chunk, last_chunk = (K - 1) / per_chunk;
        std::vector<std::pair<uint32_t, uint32_t>> checks;  // (tile, chunk): the chunks the pieces read entries from, every tile's last one
        for (uint32_t j : kp) {
            const Piece &q = pcs[j];
            uint32_t c0, c1;
            window_chunk_range(g, window_blocks(g, q.x, q.y, q.w, q.h), K, per_chunk, &c0, &c1);
            for (uint32_t c = c0; c <= c1; c++) checks.push_back({ q.slot, c });
            checks.push_back({ q.slot, last_chunk });
        }
        std::sort(checks.begin(), checks.end());
        checks.erase(std::unique(checks.begin(), checks.end()), checks.end());
        const size_t nchecks = checks.size();
        const size_t dbytes = nk * WIN_DESC_BYTES, tbytes = nt * WIN_TILE_BYTES, up = dbytes + tbytes + nchecks * WIN_TILE_CHECK_BYTES;
        const size_t stbytes = 4 * (1 + nk + nt);
        if (!p->h_wdesc.ensure(up) || !p->h_wst.ensure(stbytes) || !p->d_wdesc.ensure(up) || !p->d_wst.ensure(stbytes)) { p->error = QB3E_LIBERR; return false; }
        {
            std::vector<WinRect> rects(nk);
            std::vector<void *> dsts(nk);
            std::vector<uint32_t> slots(nk);
            for (size_t j = 0; j < nk; j++) {
                const Piece &q = pcs[kp[j]];
                rects[j] = WinRect{ q.x, q.y, q.w, q.h, q.stride }; dsts[j] = q.dst; slots[j] = q.slot;
            }
            uint64_t wsegs = 0;
            window_mosaic_plan(g, rects.data(), dsts.data(), slots.data(), nk, p->h_wdesc.p, &wsegs);
            *segs = (size_t)wsegs;
        }
        WinTile *tl = (WinTile *)((uint8_t *)p->h_wdesc.p + dbytes);
        for (size_t t = 0; t < nt; t++) {
            const uint8_t *base = (const uint8_t *)d_src + touched[t] * src_pitch;
            const size_t sz = sizes[touched[t]];
            tl[t] = WinTile{ (const uint32_t *)(base + (hdr & ~(size_t)3)), sz > hdr ? (uint64_t)(sz - hdr) * 8 : 0, base + p->ix_off, 0 };
        }
        WinTileCheck *ck = (WinTileCheck *)((uint8_t *)p->h_wdesc.p + dbytes + tbytes);
        for (size_t c = 0; c < nchecks; c++) ck[c] = WinTileCheck{ checks[c].first, checks[c].second | (checks[c].second == last_chunk ? WIN_TILE_TAIL : 0u) };
        uint32_t *d_status = (uint32_t *)p->d_wst.p;
        const uint8_t *d_up = (const uint8_t *)p->d_wdesc.p;
        if (hipMemcpyAsync(p->d_wdesc.p, p->h_wdesc.p, up, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("mosaic windows: upload", 0); return fail(); }
        if (hipMemsetAsync(d_status, 0, stbytes, st) != hipSuccess) return fail();
        if (launch_decode_windows_mosaic(*fam, g, s.plan, s.in_bit0, p->h_wdesc.p, d_up, nk, d_up + dbytes, nt, d_up + dbytes + tbytes, nchecks,
                                         d_status, st, s.ixt, (uint32_t)p->ix_off, (uint32_t)hdr, (uint32_t)p->mode & 0xffu)) return fail();
        hipError_t e = hipMemcpyAsync(p->h_wst.p, d_status, stbytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = wait_stream(st);
        if (e != hipSuccess) { set_error("mosaic window kernel", (int)e); return fail(); }
        prof_collect();
        // a tile's word: its table or its kind failed -- every piece in it goes the other way; a piece's word: that piece alone
        const uint32_t *status = (const uint32_t *)p->h_wst.p;
        for (size_t j = 0; j < nk; j++) {
            Piece &q = pcs[kp[j]];
            if (!status[1 + j] && !status[1 + nk + q.slot]) { q.whole = false; q.ok = true; }
        }
    }
    return true;
}

// The whole-tile route: the touched tiles that hold a piece without pixels are decoded whole, each once, a run of consecutive tiles a
// call of decode_tile_grids; one crop launch copies the pieces out.  false: as above
bool whole_route(decsp p, const void *d_src, size_t src_pitch, const size_t *sizes, Cut &cut, void *stream) {
    std::vector<Piece> &pcs = cut.pcs;
    const std::vector<size_t> &touched = cut.touched;
    hipStream_t st = (hipStream_t)stream;
    const size_t tw = p->xsize, th = p->ysize, tsz = szof(p->type), pb = p->nbands * tsz, nt = touched.size();
    auto fail = [&]() -> bool { (void)hipStreamSynchronize(st); p->error = QB3E_LIBERR; return false; };
    std::vector<uint32_t> place(nt, 0xffffffffu);           // the tile's place among the whole tiles
    std::vector<uint32_t> needed;
    size_t nrect = 0;
    for (const Piece &q : pcs) if (q.whole) { place[q.slot] = 0; nrect++; }
    for (size_t t = 0; t < nt; t++) if (!place[t]) { place[t] = (uint32_t)needed.size(); needed.push_back((uint32_t)t); }
    if (needed.empty()) return true;
    const size_t desc_bytes = (nrect * MOSAIC_RECT_BYTES + 255) & ~(size_t)255, tile_pitch = (tw * th * pb + 15) & ~(size_t)15;
    if (!p->d_mos.ensure(desc_bytes + needed.size() * tile_pitch)) { p->error = QB3E_LIBERR; return false; }
    uint8_t *tiles = (uint8_t *)p->d_mos.p + desc_bytes;
    std::vector<uint8_t> got(needed.size(), 0), keep;
    keep.swap(p->tile_ok);                              // (qb3x_decode_tile_ok speaks of the tile calls)
    for (size_t a = 0, b; a < needed.size(); a = b) {   // a run of consecutive tiles: one grid of one row
        for (b = a + 1; b < needed.size() && touched[needed[b]] == touched[needed[b - 1]] + 1; b++) {}
        const size_t k0 = touched[needed[a]];
        const TileGrid row = { b - a, b - a, tiles + a * tile_pitch, tile_pitch, 0, 0, 0, 0 };
        decode_tile_grids(p, (const uint8_t *)d_src + k0 * src_pitch, b - a, src_pitch, sizes + k0, &row, 1, nullptr, stream);
        if (p->error != QB3E_OK) { keep.swap(p->tile_ok); (void)hipStreamSynchronize(st); return false; }
        for (size_t i = 0; i < b - a && i < p->tile_ok.size(); i++) got[a + i] = p->tile_ok[i];
    }
    keep.swap(p->tile_ok);
    std::vector<MosaicRect> rects;
    rects.reserve(nrect);
    uint32_t max_rows = 0;
    for (Piece &q : pcs) {
        if (!q.whole || !got[place[q.slot]]) continue;
        const uint8_t *tile = tiles + place[q.slot] * tile_pitch;
        const uint32_t cw = (uint32_t)(q.w * pb);
        rects.push_back(MosaicRect{ tile + ((size_t)q.y * tw + q.x) * pb, tw * pb, q.dst, q.stride * tsz, cw, q.h, cw, q.h });
        max_rows = std::max(max_rows, q.h);
        q.ok = true;
    }
    if (!rects.empty()) {
        // (the copy is from pageable memory: the runtime has taken the bytes when it returns)
        if (hipMemcpyAsync(p->d_mos.p, rects.data(), rects.size() * MOSAIC_RECT_BYTES, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("mosaic windows: descriptors", 0); return fail(); }
        if (launch_mosaic_rects(p->d_mos.p, rects.size(), max_rows, (uint32_t)pb, false, st)) return fail();
    }
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("mosaic windows: crop", 0); return fail(); }    // (the whole tiles are the handle's: the next call may come on another stream)
    prof_collect();
    p->mos_whole = needed.size();
    return true;
}

size_t mosaic_windows_body(decsp p, const void *d_src, size_t src_pitch, const size_t *sizes, size_t W, size_t H,
                           const qb3x_window *wins, size_t n, void *stream) {
    if (!p) return 0;
    if (!d_src || !sizes || (src_pitch & 3) || ((uintptr_t)d_src & 3) || !W || !H || W > 0xffffffffull || H > 0xffffffffull) return 0;
    if (p->stage != 2 || p->error != QB3E_OK || !p->xsize || !p->ysize) return 0;
    if (!wins || !n || n > MAX_PIECES) return 0;
    const size_t tw = p->xsize, th = p->ysize, bands = p->nbands;
    size_t npieces = 0;
    for (size_t i = 0; i < n; i++) {
        const qb3x_window &w = wins[i];
        const size_t c = qb3x_mosaic_window_tiles(W, H, tw, th, w.x0, w.y0, w.w, w.h, nullptr, nullptr, nullptr, nullptr);
        if (!c || !w.dst || (w.dst_stride && w.dst_stride < w.w * bands)) return 0;
        npieces += c;
        if (npieces > MAX_PIECES) return 0;
    }
    // ---- nothing was touched up to here
    hipStream_t st = (hipStream_t)stream;
    p->wins_path.assign(n, 0);
    p->win_path = 0; p->win_segs = 0; p->mos_whole = 0;
    Cut cut;
    cut_pieces(p, W, H, wins, n, npieces, cut);
    if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }
    size_t segs = 0;
    if (!kernel_route(p, d_src, src_pitch, sizes, cut, st, &segs) || !whole_route(p, d_src, src_pitch, sizes, cut, stream)) return 0;

    // ---- a window is written when all of its pieces are
    for (size_t i = 0; i < n; i++) p->wins_path[i] = 1;
    for (const Piece &q : cut.pcs) {
        uint8_t &path = p->wins_path[q.win];
        if (!q.ok) path = 0;
        else if (q.whole && path) path = 3;
    }
    size_t done = 0;
    for (size_t i = 0; i < n; i++) done += p->wins_path[i] != 0;
    p->win_path = p->wins_path[n - 1]; p->win_segs = segs;
    return done;
}

}  // namespace

QB3_API size_t qb3x_decode_mosaic_windows(decsp p, const void *d_src, size_t src_pitch, const size_t *sizes, size_t W, size_t H,
                                          const qb3x_window *wins, size_t n, void *stream) {
    return abi_guard<size_t>(0, [&] { return mosaic_windows_body(p, d_src, src_pitch, sizes, W, H, wins, n, stream); });
}

QB3_API size_t qb3x_last_mosaic_whole_tiles(const decsp p) { return p ? p->mos_whole : 0; }
