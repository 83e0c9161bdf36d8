// qb3_amd/csrc/api_window.cpp -- window decode, host side: a rectangle of a raster (qb3x_decode_window_device, qb3x_read_window) or a batch
// of rectangles of one raster (qb3x_decode_windows_device, qb3x_read_windows), and the way from the shortcuts back to the whole decode.
#include <utility>
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

// A window's bytes are by definition "decode everything, crop" (path 3); the other two ways are shortcuts to the same bytes that are
// taken when the container carries a level-2 table and dropped again on ANY nonzero status word:
//   path 1  a raster one of the families of window kernels takes (window_family, qb3_dev.h: 8-bit rasters of 1, 3 or 4 bands in FTL /
//           BASE always; the other four on a handle that asked for them, qb3x_set_decoder_window_kernels) and destinations aligned as
//           the family stores: a window kernel decodes only the segments that hold a block of a window, straight into the caller's
//           buffer.  The single call's kernel takes its window as kernel arguments and gives one status word; the batch's decodes
//           all windows in ONE launch, a status word per window;
//   path 2  every other raster that decodes strip by strip (decode_strips_ok): the windows' block rows as ranges of segments, merged
//           so that a segment is decoded once, into the handle's scratch raster, then a crop per window;
//   path 3  ONE whole decode with its fallback ladder into the scratch raster for all windows that have no pixels yet, then their crops.
// Everything but path 1 is written once, over a span of windows.  The single calls pass a span of one and a result word of their
// own, so the per-window results of an earlier batch (qb3x_window_ok / qb3x_window_path) stay as they are.

static WinRect win_rect(const decs *p, const qb3x_window &w) { return WinRect{ (uint32_t)w.x0, (uint32_t)w.y0, (uint32_t)w.w, (uint32_t)w.h, win_stride(p, w) }; }
static bool window_check(const decs *p, const qb3x_window &w) {
    return w.dst && window_inside(p, w.x0, w.y0, w.w, w.h) && (!w.dst_stride || w.dst_stride >= w.w * p->nbands);
}
// handle and rectangles of a window call (host: the container is read from the handle's host memory); false: p->error is set, nothing was touched
bool qb3api::windows_check(decsp p, const qb3x_window *wins, size_t n, bool host) {
    if (p->stage != 2 || p->error != QB3E_OK || p->s_in == nullptr || p->s_size == 0) {
        if (p->error == QB3E_OK) p->error = QB3E_EINV;
        return false;
    }
    bool ok = wins && n && n <= ((size_t)1 << 20);
    for (size_t i = 0; ok && i < n; i++) ok = window_check(p, wins[i]);
    if (host && p->hdr_avail < (size_t)(p->s_in - p->s_start) + p->s_size) ok = false;     // (a handle over a copy of the container's head only: as qb3_read_data)
    if (!ok) p->error = QB3E_EINV;
    return ok;
}

// rows [y0, y0 + h) x columns [x0, x0 + w) of a tight raster in device memory into the window's device buffer; does not wait
static bool window_crop(decsp p, const void *d_raster, const qb3x_window &w, hipStream_t st) {
    const size_t tsz = szof(p->type), pix = p->nbands * tsz, line = p->xsize * pix;
    const hipError_t e = hipMemcpy2DAsync(w.dst, win_stride(p, w) * tsz, (const uint8_t *)d_raster + w.y0 * line + w.x0 * pix, line, w.w * pix, w.h, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) set_error("window crop", (int)e);
    return e == hipSuccess;
}

// a container in device memory as the kernels take it: geometry and plan, the container's table, the stream's first bit and its length
// (struct WinSrc: qb3_host.h)
WinSrc qb3api::window_source(const decs *p, const Geometry &g, const void *d_src) {
    const size_t off = (size_t)(p->s_in - p->s_start);
    return WinSrc{ g, plan_decode(g), handle_table(p, (const uint8_t *)d_src + p->ix_off), (const uint32_t *)((const uint8_t *)d_src + (off & ~(size_t)3)),
                   (uint32_t)(8 * (off & 3)), (uint64_t)p->s_size * 8 };
}

// The three functions below mark the windows they gave their pixels (paths[i]) and count the segments they decoded; false: a HIP failure.
// path 1, the single call: the window as kernel arguments, one status word back
static bool window_kernel_one(decsp p, const WinSrc &s, const qb3x_window &w, uint8_t *path, size_t *segs, hipStream_t st, const WinKernels &fam) {
    const WinRect r = win_rect(p, w);
    uint32_t status = 1;
    if (!p->d_wst.ensure(64) || launch_decode_window(fam, s.g, s.plan, s.in32, s.in_bit0, s.in_bits, w.dst, r, (uint32_t *)p->d_wst.p, st, s.ixt)) return false;
    const hipError_t e = fetch_small(&status, p->d_wst.p, 4, st);
    if (e != hipSuccess) { set_error("window kernel", (int)e); return false; }
    *segs = (size_t)window_segments(s.g, r);
    if (!status) *path = 1;
    return true;
}
// path 1, a batch: descriptors and the chunk list are built in the pinned area, one copy up; n + 1 status words, one memset, one copy back
// (ws: a band-selected call -- the family's band-selected form when ws->sel is set, and ws->extra_bytes more bytes behind the chunk list, on sixteen)
bool qb3api::window_kernel_batch(decsp p, const WinSrc &s, const qb3x_window *wins, size_t n, uint8_t *paths, size_t *segs, hipStream_t st, const WinKernels &fam,
                                 const WinSel *ws) {
    const size_t dbytes = n * WIN_DESC_BYTES, extra = ws ? ws->extra_bytes : 0;
    const size_t upbytes = dbytes + 4 * ix_chunks(s.ixt) + (extra ? 16 + extra : 0), stbytes = 4 * (n + 1);
    if (!p->h_wdesc.ensure(upbytes) || !p->h_wst.ensure(stbytes) || !p->d_wdesc.ensure(upbytes) || !p->d_wst.ensure(stbytes)) return false;
    std::vector<WinRect> rects(n);
    std::vector<void *> dsts(n);
    for (size_t i = 0; i < n; i++) { rects[i] = win_rect(p, wins[i]); dsts[i] = wins[i].dst; }
    std::vector<uint32_t> chunks;
    uint64_t wsegs = 0;
    const size_t nchunks = window_batch_plan(s.g, s.ixt, rects.data(), dsts.data(), n, p->h_wdesc.p, chunks, &wsegs);
    if (nchunks) memcpy((uint8_t *)p->h_wdesc.p + dbytes, chunks.data(), 4 * nchunks);
    uint32_t *d_status = (uint32_t *)p->d_wst.p;
    size_t up = dbytes + 4 * nchunks;
    if (extra) {
        up = (up + 15) & ~(size_t)15;
        memcpy((uint8_t *)p->h_wdesc.p + up, ws->extra, extra);
        *ws->d_extra = (const uint8_t *)p->d_wdesc.p + up;
        up += extra;
    }
    HIPOK(hipMemcpyAsync(p->d_wdesc.p, p->h_wdesc.p, up, hipMemcpyHostToDevice, st));
    if (hipMemsetAsync(d_status, 0, stbytes, st) != hipSuccess) return false;
    if (launch_decode_windows(fam, s.g, s.plan, s.in32, s.in_bit0, s.in_bits, p->h_wdesc.p, p->d_wdesc.p, n,
                              (const uint32_t *)((const uint8_t *)p->d_wdesc.p + dbytes), nchunks, d_status, st, s.ixt,
                              ws ? ws->sel : nullptr, ws ? ws->nsel : 0)) return false;
    hipError_t e = hipMemcpyAsync(p->h_wst.p, d_status, stbytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = wait_stream(st);
    if (e != hipSuccess) { set_error("window batch kernel", (int)e); return false; }
    const uint32_t *status = (const uint32_t *)p->h_wst.p;
    *segs = (size_t)wsegs;
    // word 0: a table chunk failed its check, or the table's end lies beyond the stream's -- no window keeps its shortcut
    for (size_t i = 0; i < n && !status[0]; i++) if (!status[1 + i]) paths[i] = 1;
    return true;
}
// path 2: the segments of the windows' block rows into the scratch raster, one status word for all of them, then the crops
// (crop false: a band-selected call, whose gather reads the scratch raster)
bool qb3api::window_strips(decsp p, const WinSrc &s, const qb3x_window *wins, size_t n, uint8_t *paths, size_t *segs, hipStream_t st, bool crop) {
    const Geometry &g = s.g;
    if (!p->d_win.ensure(qb3_decoded_size(p)) || !p->d_ws.ensure(s.plan.ws_bytes)) return false;
    std::vector<std::pair<uint64_t, uint64_t>> rg(n);
    for (size_t i = 0; i < n; i++) {
        const WinBlocks b = window_blocks(g, wins[i].x0, wins[i].y0, wins[i].w, wins[i].h);
        rg[i] = { (uint64_t)b.by0 * g.nbx / g.seg_blocks, ((uint64_t)(b.by1 + 1) * g.nbx - 1) / g.seg_blocks + 1 };
    }
    merge_ranges(rg);
    uint32_t *d_status = nullptr, status = 1;
    for (size_t k = 0; k < rg.size(); k++) {               // the first with first-strip semantics: status zeroed, table checked
        const DecStrip strip = { rg[k].first, rg[k].second - rg[k].first, k == 0 };
        if (launch_decode(g, s.plan, s.in32, s.in_bit0, s.in_bits, p->d_win.p, nullptr, p->d_ws.p, &d_status, st, TileBatch(), nullptr, s.ixt,
                          nullptr, 0, false, 16, &strip)) return false;
        *segs += (size_t)(rg[k].second - rg[k].first);
    }
    if (launch_window_tail_check(g, s.in_bits, d_status, st, s.ixt)) return false;
    const hipError_t e = fetch_small(&status, d_status, 4, st);
    if (e != hipSuccess) { set_error("window strips", (int)e); return false; }
    for (size_t i = 0; i < n && !status; i++) {
        if (crop && !window_crop(p, p->d_win.p, wins[i], st)) return false;
        paths[i] = 2;
    }
    return true;
}

// The windows of a container in device memory into their device buffers.  paths: a zeroed byte per window, which receives the path the
// window's pixels came by (0: none); single: one of the single calls.  Returns the number of windows written.
size_t qb3api::windows_device(decsp p, const void *d_src, const void *d_index, const qb3x_window *wins, size_t n, uint8_t *paths, bool single, hipStream_t st) {
    const bool coded = p->mode != QB3M_STORED && p->xsize >= 4 && p->ysize >= 4;       // (narrow images decode through a stand-in shape: no block grid)
    p->win_path = 0; p->win_segs = 0;
    Geometry g;
    memset(&g, 0, sizeof(g));
    if (coded) g = decoder_geometry(p, p->xsize, p->ysize, 0);
    auto fail = [&]() -> size_t { (void)hipStreamSynchronize(st); p->error = QB3E_LIBERR; return 0; };    // (nothing of the handle's stays in flight)
    size_t segs = 0, todo = n;                              // todo: windows that have no pixels yet
    if (coded && !d_index && p->ix_K && p->ix_bl && !is_rle_mode(p->mode)) {
        if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }
        const WinSrc s = window_source(p, g, d_src);
        bool scratch = false;
        // path 1: the family that takes the raster and its table, on a handle that asked for it, with stores every destination is aligned for
        const WinKernels *fam = family_if_aligned(window_family(g, s.plan, s.ixt, p->win_kernels), g, wins, n);
        if (fam) {
            if (!(single ? window_kernel_one(p, s, wins[0], paths, &segs, st, *fam) : window_kernel_batch(p, s, wins, n, paths, &segs, st, *fam))) return fail();
        } else if ((scratch = decode_strips_ok(g, s.plan, s.ixt))) {
            if (!window_strips(p, s, wins, n, paths, &segs, st)) return fail();
        }
        for (size_t i = 0; i < n; i++) {
            if (!paths[i]) continue;
            if (!window_dequantize(p, g, wins[i].dst, wins[i].w, wins[i].h, win_stride(p, wins[i]), st)) return fail();
            todo--;
        }
        if (scratch && !todo && hipStreamSynchronize(st) != hipSuccess) return fail();      // (the scratch raster is the handle's: the next call may come on another stream)
        prof_collect();
        if (!todo) p->last_status = 0;
    }
    if (todo) {
        // a raster no shortcut takes, a table that failed its check, segments that did not decode, a stream that ends early: ONE
        // whole decode for all the windows that are left; what a shortcut wrote to them is overwritten by the crop
        if (single) segs = 0;                               // (qb3x.h: a single call reports the segments of the path it ended on, a batch all its kernels decoded)
        if (!p->d_win.ensure(qb3_decoded_size(p))) { p->error = QB3E_LIBERR; return 0; }
        const size_t keep = p->stride;
        p->stride = 0;                                      // (the scratch raster is tight; the caller's setting is for qb3_read_data)
        const size_t got = decode_common(p, nullptr, d_src, p->d_win.p, d_index, st);
        p->stride = keep;
        if (got) {
            for (size_t i = 0; i < n; i++) if (!paths[i] && !window_crop(p, p->d_win.p, wins[i], st)) return fail();
            if (hipStreamSynchronize(st) != hipSuccess) return fail();
            for (size_t i = 0; i < n; i++) if (!paths[i]) paths[i] = 3;
            if (coded) segs += (size_t)g.nseg;
        }
    }
    size_t done = 0;
    for (size_t i = 0; i < n; i++) done += paths[i] != 0;
    p->win_path = paths[n - 1]; p->win_segs = segs;
    return done;
}

bool qb3api::window_dequantize(decsp p, const Geometry &g, void *dst, size_t w, size_t h, size_t stride, hipStream_t st) {
    Geometry gw = g;
    gw.w = (uint32_t)w; gw.h = (uint32_t)h; gw.stride = stride;
    return p->quanta <= 1 || !launch_dequantize(dst, gw, (int)p->type, p->quanta, st);
}
bool qb3api::windows_out(decsp p, const qb3x_window *wins, size_t n, std::vector<void *> &dsts) {
    const size_t pix = p->nbands * szof(p->type);
    std::vector<size_t> at(n + 1, 0);
    for (size_t i = 0; i < n; i++) at[i + 1] = at[i] + ((wins[i].h * wins[i].w * pix + 3) & ~(size_t)3);
    if (!p->d_wout.ensure(at[n])) return false;
    dsts = std::vector<void *>(n);
    for (size_t i = 0; i < n; i++) dsts[i] = (uint8_t *)p->d_wout.p + at[i];
    return true;
}

// The same for a container in host memory and host destinations (paths, single: as above): STORED containers are cropped on the
// host; else the whole container goes up ONCE (the stream and its table), the windows are decoded back to back into one device
// buffer (each starts on a dword) and come down one by one, each with its stride
size_t qb3api::windows_host(decsp p, const qb3x_window *wins, size_t n, uint8_t *paths, bool single) {
    const size_t tsz = szof(p->type), pix = p->nbands * tsz, line = p->xsize * pix, csize = (size_t)(p->s_in - p->s_start) + p->s_size;
    p->win_path = 0; p->win_segs = 0;
    if (p->mode == QB3M_STORED) {           // raw pixels: no device needed (reference QB3decode.cpp:356-375)
        if (p->s_size != qb3_decoded_size(p)) { p->error = QB3E_EINV; return 0; }
        for (size_t i = 0; i < n; i++) {
            const qb3x_window &w = wins[i];
            for (size_t y = 0; y < w.h; y++) memcpy((uint8_t *)w.dst + y * win_stride(p, w) * tsz, p->s_in + (w.y0 + y) * line + w.x0 * pix, w.w * pix);
            paths[i] = 3;
        }
        p->win_path = 3;
        return n;
    }
    if (p->xsize * p->ysize < 16) { p->error = QB3E_EINV; return 0; }
    if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }
    hipStream_t st = nullptr;
    std::vector<qb3x_window> dw(wins, wins + n);
    std::vector<void *> dsts;
    if (!p->d_wsrc.ensure(csize + 8) || !windows_out(p, wins, n, dsts)) { p->error = QB3E_LIBERR; return 0; }
    for (size_t i = 0; i < n; i++) { dw[i].dst = dsts[i]; dw[i].dst_stride = 0; }
    if (!upload(p->stager, p->d_wsrc.p, p->s_start, csize, st)) { p->error = QB3E_LIBERR; return 0; }
    HIPOK(hipMemsetAsync((uint8_t *)p->d_wsrc.p + csize, 0, 8, st));      // (a stream that ends early reads as zeros behind its end)
    if (!windows_device(p, p->d_wsrc.p, nullptr, dw.data(), n, paths, single, st)) return 0;
    if (single && win_stride(p, wins[0]) == wins[0].w * p->nbands) {      // one window with tight rows: through the pinned ring when large; waits
        if (!download(p->stager, wins[0].dst, dw[0].dst, wins[0].h * wins[0].w * pix, st)) { p->error = QB3E_LIBERR; return 0; }
        return 1;
    }
    size_t done = 0;
    for (size_t i = 0; i < n; i++) {
        if (!paths[i]) continue;
        const qb3x_window &w = wins[i];
        const size_t wline = w.w * pix;
        HIPOK(hipMemcpy2DAsync(w.dst, win_stride(p, w) * tsz, dw[i].dst, wline, wline, w.h, hipMemcpyDeviceToHost, st));
        done++;
    }
    HIPOK(hipStreamSynchronize(st));
    return done;
}

QB3_API size_t qb3x_decode_window_device(decsp p, const void *d_src, const void *d_index, size_t x0, size_t y0, size_t w, size_t h,
                                         void *d_dst, size_t dst_stride, void *stream) {
    if (!p || !d_src || !d_dst || ((uintptr_t)d_src & 3)) { if (p) p->error = QB3E_EINV; return 0; }
    return abi_guard<size_t>(0, [&]() -> size_t {
        const qb3x_window win = { x0, y0, w, h, d_dst, dst_stride };
        uint8_t path = 0;
        if (!windows_check(p, &win, 1, false) || !windows_device(p, d_src, d_index, &win, 1, &path, true, (hipStream_t)stream)) return 0;
        return h * w * p->nbands * szof(p->type);
    });
}
QB3_API size_t qb3x_read_window(decsp p, size_t x0, size_t y0, size_t w, size_t h, void *dst, size_t dst_stride) {
    if (!p || !dst) { if (p) p->error = QB3E_EINV; return 0; }
    return abi_guard<size_t>(0, [&]() -> size_t {
        const qb3x_window win = { x0, y0, w, h, dst, dst_stride };
        uint8_t path = 0;
        if (!windows_check(p, &win, 1, true) || !windows_host(p, &win, 1, &path, true)) return 0;
        return h * w * p->nbands * szof(p->type);
    });
}
QB3_API size_t qb3x_decode_windows_device(decsp p, const void *d_src, const void *d_index, const qb3x_window *wins, size_t n, void *stream) {
    if (!p || !d_src || ((uintptr_t)d_src & 3)) { if (p) p->error = QB3E_EINV; return 0; }
    return abi_guard<size_t>(0, [&]() -> size_t {
        if (!windows_check(p, wins, n, false)) return 0;
        p->wins_path.assign(n, 0);
        return windows_device(p, d_src, d_index, wins, n, p->wins_path.data(), false, (hipStream_t)stream);
    });
}
QB3_API size_t qb3x_read_windows(decsp p, const qb3x_window *wins, size_t n) {
    if (!p) return 0;
    return abi_guard<size_t>(0, [&]() -> size_t {
        if (!windows_check(p, wins, n, true)) return 0;
        p->wins_path.assign(n, 0);
        return windows_host(p, wins, n, p->wins_path.data(), false);
    });
}

QB3_API int qb3x_window_ok(const decsp p, size_t i) { return (p && i < p->wins_path.size() && p->wins_path[i]) ? 1 : 0; }
QB3_API int qb3x_window_path(const decsp p, size_t i) { return (p && i < p->wins_path.size()) ? p->wins_path[i] : 0; }

QB3_API size_t qb3x_window_segments(const decsp p, size_t x0, size_t y0, size_t w, size_t h, size_t *blocks_per_segment) {
    if (blocks_per_segment) *blocks_per_segment = 0;
    if (!p || p->stage != 2 || !window_inside(p, x0, y0, w, h)) return 0;
    if (p->mode == QB3M_STORED || p->xsize < 4 || p->ysize < 4) return 1;      // no block grid: one piece
    return abi_guard<size_t>(0, [&]() -> size_t {
        const Geometry g = decoder_geometry(p, p->xsize, p->ysize, 0);
        if (blocks_per_segment) *blocks_per_segment = g.seg_blocks;
        const WinRect r = { (uint32_t)x0, (uint32_t)y0, (uint32_t)w, (uint32_t)h, 0 };
        return (size_t)window_segments(g, r);
    });
}
QB3_API int qb3x_last_window_path(const decsp p) { return p ? p->win_path : 0; }
QB3_API size_t qb3x_last_window_segments(const decsp p) { return p ? p->win_segs : 0; }
