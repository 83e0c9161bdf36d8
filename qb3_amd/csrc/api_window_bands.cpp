// qb3_amd/csrc/api_window_bands.cpp -- band-selected windows, host side (qb3x_decode_windows_bands_device, qb3x_read_windows_bands): the
// rectangles of a batch call with `nsel` chosen bands a pixel in place of all the raster's.  The bytes are by definition those of
// qb3x_decode_windows_device with the bands picked; the three paths, their order and the per-window results are api_window.cpp's.
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

// Two ROUTES lead to the selected bands:
//   fused   a lane-per-unit family (win_unit, win_cfu) on a handle that set its bit, value-aligned destinations, seg_blocks * nsel <= 64
//           (window_sel_fused): the family's band-selected batch writes the selection from the wave's LDS tile, nothing else runs;
//   gather  everything else: full-band pixels go where the handle owns the memory -- on path 1 the family's ordinary batch into tight
//           windows in d_wfull, each on a multiple of sixteen bytes (every family's alignment), on paths 2 and 3 the scratch raster as
//           for the full-band calls -- and ONE launch of win_band_gather_kernel per path picks the bands (it takes the crop's place and
//           multiplies back where the path's pixels are still quantised).  A gather call waits for its stream: descriptors and sources
//           are the handle's, and the next call may come on another stream.
// The identity selection is the full-band call itself.

static bool sel_identity(const decs *p, const uint8_t *sel, size_t nsel) {
    bool id = nsel == p->nbands;
    for (size_t k = 0; id && k < nsel; k++) id = sel[k] == k;
    return id;
}
// as windows_check, with the selection and with nsel values a pixel in the stride rule; false: p->error is set, nothing was touched
static bool bands_check(decsp p, const qb3x_window *wins, size_t n, const uint8_t *sel, size_t nsel, bool host) {
    if (p->stage != 2 || p->error != QB3E_OK || p->s_in == nullptr || p->s_size == 0) {
        if (p->error == QB3E_OK) p->error = QB3E_EINV;
        return false;
    }
    bool ok = wins && n && n <= ((size_t)1 << 20) && sel && nsel >= 1 && nsel <= (size_t)MAXBANDS;
    for (size_t k = 0; ok && k < nsel; k++) ok = sel[k] < p->nbands;
    for (size_t i = 0; ok && i < n; i++) {
        const qb3x_window &w = wins[i];
        ok = w.dst && window_inside(p, w.x0, w.y0, w.w, w.h) && (!w.dst_stride || w.dst_stride >= w.w * nsel) && w.w * nsel <= 0xffffffffull;
    }
    if (host && p->hdr_avail < (size_t)(p->s_in - p->s_start) + p->s_size) ok = false;
    if (!ok) p->error = QB3E_EINV;
    return ok;
}

// the gather's descriptor of window w whose full-band pixels start at src, rows spitch bytes apart
static WinGather gather_desc(const decs *p, const qb3x_window &w, const void *src, size_t spitch, size_t nsel) {
    return WinGather{ src, (uint64_t)spitch, w.dst, (uint64_t)(w.dst_stride * szof(p->type)), (uint32_t)w.w, (uint32_t)w.h, (uint32_t)p->nbands, 0u };
}
// one gather launch for the windows of wins that `take` says yes to, out of the tight raster at d_raster; quanta: multiply back
template <class Take>
static bool gather_from_raster(decsp p, const void *d_raster, const qb3x_window *wins, size_t n, const uint8_t *sel, size_t nsel, uint64_t quanta, hipStream_t st, Take take) {
    const size_t pix = p->nbands * szof(p->type), line = p->xsize * pix;
    std::vector<WinGather> gd;
    uint64_t rows = 0;
    for (size_t i = 0; i < n; i++) {
        if (!take(i)) continue;
        gd.push_back(gather_desc(p, wins[i], (const uint8_t *)d_raster + wins[i].y0 * line + wins[i].x0 * pix, line, nsel));
        rows = std::max<uint64_t>(rows, wins[i].h);
    }
    if (gd.empty()) return true;
    const size_t bytes = gd.size() * WIN_GATHER_BYTES;
    if (!p->h_wgat.ensure(bytes) || !p->d_wgat.ensure(bytes)) return false;
    memcpy(p->h_wgat.p, gd.data(), bytes);
    if (hipMemcpyAsync(p->d_wgat.p, p->h_wgat.p, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return false;
    if (launch_window_gather(p->d_wgat.p, gd.size(), rows, sel, (uint32_t)nsel, (int)p->type, quanta, st)) return false;
    p->win_gathers++;
    return true;
}

// The selected bands of the windows of a container in device memory into their device buffers (paths: a zeroed byte per window).
// Returns the number of windows written.
static size_t windows_bands_device(decsp p, const void *d_src, const void *d_index, const qb3x_window *wins, size_t n, const uint8_t *sel, size_t nsel,
                                   uint8_t *paths, hipStream_t st) {
    const bool coded = p->mode != QB3M_STORED && p->xsize >= 4 && p->ysize >= 4;
    const size_t tsz = szof(p->type), pix = p->nbands * tsz;
    p->win_path = 0; p->win_segs = 0; p->win_gathers = 0;
    std::vector<qb3x_window> sw(wins, wins + n);           // ... with the stride said
    for (size_t i = 0; i < n; i++) if (!sw[i].dst_stride) sw[i].dst_stride = sw[i].w * nsel;
    Geometry g;
    memset(&g, 0, sizeof(g));
    if (coded) g = decoder_geometry(p, p->xsize, p->ysize, 0);
    auto fail = [&]() -> size_t { (void)hipStreamSynchronize(st); p->error = QB3E_LIBERR; return 0; };
    size_t segs = 0, todo = n;
    if (coded && !d_index && p->ix_K && p->ix_bl && !is_rle_mode(p->mode)) {
        if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }
        const WinSrc s = window_source(p, g, d_src);
        const WinKernels *fam = window_family(g, s.plan, s.ixt, p->win_kernels);
        bool aligned = true, wait = false;
        for (size_t i = 0; i < n; i++) aligned = aligned && ((uintptr_t)sw[i].dst & (tsz - 1)) == 0;
        if (aligned && window_sel_fused(fam, g, (uint32_t)nsel)) {
            const WinSel ws = { sel, (uint32_t)nsel, nullptr, 0, nullptr };
            if (!window_kernel_batch(p, s, sw.data(), n, paths, &segs, st, *fam, &ws)) return fail();
            Geometry gs = g;
            gs.bands = (uint32_t)nsel;                      // (the window as a raster of nsel bands)
            for (size_t i = 0; i < n; i++)
                if (paths[i] && !window_dequantize(p, gs, sw[i].dst, sw[i].w, sw[i].h, sw[i].dst_stride, st)) return fail();
        } else if (fam) {
            // the family's ordinary batch into tight windows of the handle's, the gather's descriptors behind its own in the same copy
            std::vector<qb3x_window> fw(sw);
            std::vector<size_t> at(n + 1, 0);
            for (size_t i = 0; i < n; i++) at[i + 1] = at[i] + ((sw[i].h * sw[i].w * pix + 15) & ~(size_t)15);
            if (!p->d_wfull.ensure(at[n])) return fail();
            std::vector<WinGather> gd(n);
            uint64_t rows = 0;
            for (size_t i = 0; i < n; i++) {
                fw[i].dst = (uint8_t *)p->d_wfull.p + at[i]; fw[i].dst_stride = 0;
                gd[i] = gather_desc(p, sw[i], fw[i].dst, sw[i].w * pix, nsel);
                rows = std::max<uint64_t>(rows, sw[i].h);
            }
            const void *d_gd = nullptr;
            const WinSel ws = { nullptr, 0, gd.data(), n * WIN_GATHER_BYTES, &d_gd };
            if (!window_kernel_batch(p, s, fw.data(), n, paths, &segs, st, *fam, &ws)) return fail();
            bool any = false;
            for (size_t i = 0; i < n; i++) any = any || paths[i];
            // (all n: a window that lost its shortcut gets bytes the whole decode's gather overwrites, as a window kernel's own stores are)
            if (any) {
                if (launch_window_gather(d_gd, n, rows, sel, (uint32_t)nsel, (int)p->type, p->quanta, st)) return fail();
                p->win_gathers++;
                wait = true;
            }
        } else if (decode_strips_ok(g, s.plan, s.ixt)) {
            if (!window_strips(p, s, sw.data(), n, paths, &segs, st, false)) return fail();
            if (!gather_from_raster(p, p->d_win.p, sw.data(), n, sel, nsel, p->quanta, st, [&](size_t i) { return paths[i] != 0; })) return fail();
            wait = true;
        }
        for (size_t i = 0; i < n; i++) todo -= paths[i] != 0;
        if (wait && hipStreamSynchronize(st) != hipSuccess) return fail();
        prof_collect();
        if (!todo) p->last_status = 0;
    }
    if (todo) {
        // ONE whole decode (dequantised) for all the windows that are left, then their gather
        if (!p->d_win.ensure(qb3_decoded_size(p))) { p->error = QB3E_LIBERR; return 0; }
        const size_t keep = p->stride;
        p->stride = 0;
        const size_t got = decode_common(p, nullptr, d_src, p->d_win.p, d_index, st);
        p->stride = keep;
        if (got) {
            if (!gather_from_raster(p, p->d_win.p, sw.data(), n, sel, nsel, 1, st, [&](size_t i) { return paths[i] == 0; })) return fail();
            if (hipStreamSynchronize(st) != hipSuccess) return fail();
            prof_collect();
            for (size_t i = 0; i < n; i++) if (!paths[i]) paths[i] = 3;
            if (coded) segs += (size_t)g.nseg;
        }
    }
    size_t done = 0;
    for (size_t i = 0; i < n; i++) done += paths[i] != 0;
    p->win_path = paths[n - 1]; p->win_segs = segs;
    return done;
}

// The same for a container in host memory and host destinations: STORED containers are cropped and selected on the host; else the
// container goes up once, the selected bands are decoded back to back into one device buffer and only they come down
static size_t windows_bands_host(decsp p, const qb3x_window *wins, size_t n, const uint8_t *sel, size_t nsel, uint8_t *paths) {
    const size_t tsz = szof(p->type), pix = p->nbands * tsz, line = p->xsize * pix, csize = (size_t)(p->s_in - p->s_start) + p->s_size;
    p->win_path = 0; p->win_segs = 0; p->win_gathers = 0;
    auto stride_of = [&](const qb3x_window &w) { return w.dst_stride ? w.dst_stride : w.w * nsel; };
    if (p->mode == QB3M_STORED) {           // raw pixels: no device needed
        if (p->s_size != qb3_decoded_size(p)) { p->error = QB3E_EINV; return 0; }
        for (size_t i = 0; i < n; i++) {
            const qb3x_window &w = wins[i];
            for (size_t y = 0; y < w.h; y++) {
                const uint8_t *src = p->s_in + (w.y0 + y) * line + w.x0 * pix;
                uint8_t *dst = (uint8_t *)w.dst + y * stride_of(w) * tsz;
                for (size_t x = 0; x < w.w; x++)
                    for (size_t k = 0; k < nsel; k++) memcpy(dst + (x * nsel + k) * tsz, src + x * pix + sel[k] * tsz, tsz);
            }
            paths[i] = 3;
        }
        p->win_path = 3;
        return n;
    }
    if (p->xsize * p->ysize < 16) { p->error = QB3E_EINV; return 0; }
    if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }
    hipStream_t st = nullptr;
    std::vector<qb3x_window> dw(wins, wins + n);
    std::vector<size_t> at(n + 1, 0);
    for (size_t i = 0; i < n; i++) at[i + 1] = at[i] + ((wins[i].h * wins[i].w * nsel * tsz + 15) & ~(size_t)15);
    if (!p->d_wsrc.ensure(csize + 8) || !p->d_wout.ensure(at[n])) { p->error = QB3E_LIBERR; return 0; }
    for (size_t i = 0; i < n; i++) { dw[i].dst = (uint8_t *)p->d_wout.p + at[i]; dw[i].dst_stride = 0; }
    if (!upload(p->stager, p->d_wsrc.p, p->s_start, csize, st)) { p->error = QB3E_LIBERR; return 0; }
    HIPOK(hipMemsetAsync((uint8_t *)p->d_wsrc.p + csize, 0, 8, st));      // (a stream that ends early reads as zeros behind its end)
    if (!windows_bands_device(p, p->d_wsrc.p, nullptr, dw.data(), n, sel, nsel, paths, st)) return 0;
    size_t done = 0;
    for (size_t i = 0; i < n; i++) {
        if (!paths[i]) continue;
        const qb3x_window &w = wins[i];
        const size_t wline = w.w * nsel * tsz;
        HIPOK(hipMemcpy2DAsync(w.dst, stride_of(w) * tsz, dw[i].dst, wline, wline, w.h, hipMemcpyDeviceToHost, st));
        done++;
    }
    HIPOK(hipStreamSynchronize(st));
    return done;
}

QB3_API size_t qb3x_decode_windows_bands_device(decsp p, const void *d_src, const void *d_index, const qb3x_window *wins, size_t n,
                                                const uint8_t *sel, size_t nsel, void *stream) {
    if (!p || !d_src || ((uintptr_t)d_src & 3)) { if (p) p->error = QB3E_EINV; return 0; }
    return abi_guard<size_t>(0, [&]() -> size_t {
        if (!bands_check(p, wins, n, sel, nsel, false)) return 0;
        p->wins_path.assign(n, 0);
        if (sel_identity(p, sel, nsel)) {
            p->win_gathers = 0;
            return windows_device(p, d_src, d_index, wins, n, p->wins_path.data(), false, (hipStream_t)stream);
        }
        return windows_bands_device(p, d_src, d_index, wins, n, sel, nsel, p->wins_path.data(), (hipStream_t)stream);
    });
}
QB3_API size_t qb3x_read_windows_bands(decsp p, const qb3x_window *wins, size_t n, const uint8_t *sel, size_t nsel) {
    if (!p) return 0;
    return abi_guard<size_t>(0, [&]() -> size_t {
        if (!bands_check(p, wins, n, sel, nsel, true)) return 0;
        p->wins_path.assign(n, 0);
        if (sel_identity(p, sel, nsel)) {
            p->win_gathers = 0;
            return windows_host(p, wins, n, p->wins_path.data(), false);
        }
        return windows_bands_host(p, wins, n, sel, nsel, p->wins_path.data());
    });
}
QB3_API size_t qb3x_last_window_gathers(const decsp p) { return p ? p->win_gathers : 0; }
