// qb3_amd/csrc/qb3_host.h -- what the host files of the C ABI share: the two handle structs, the buffers they own, and the
// prototypes of the functions one file defines and another calls (namespace qb3api: nothing of it is exported).
// Host code only -- no kernel file includes it.  Which file holds what: DESIGN.md, "Host files".
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <exception>
#include <initializer_list>
#include <vector>
#include <utility>
#include <algorithm>
#include "../../include/QB3.h"
#include "../../include/qb3x.h"
#include "qb3_dev.h"
#include "qb3_host_io.h"

#define QB3_API extern "C" __attribute__((visibility("default")))
// for functions that take the handle as `p` and return 0 on failure
#define HIPOK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { qb3dev::set_error(#x, (int)e_); p->error = QB3E_LIBERR; return 0; } } while (0)

// ---------------------------------------------------------------- buffers a handle owns (api_mem.cpp)
// device memory; a released buffer waits in a per-process pool for the next handle
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int dev = 0;
    bool ensure(size_t n);
    void release(bool idle = false);        // idle: the caller has just waited for the device
};
// a small pinned host area a handle owns (descriptors up, status words back: one copy each way, no staging by the runtime)
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        release();
        n = std::max<size_t>(n + n / 2, 4096);
        if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); qb3dev::set_error("hipHostMalloc", 0); p = nullptr; return false; }
        cap = n;
        return true;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
// The reference API hands over pageable host memory (qb3_host_io.h: the ring of pinned slices, the pool of copy threads).
struct Stager {
    qb3host::PinnedRing *ring = nullptr;
    static constexpr size_t SLICE = qb3host::PinnedRing::SLICE, NSLOT = qb3host::PinnedRing::NSLOT, MIN_BYTES = qb3host::PinnedRing::MIN_BYTES;
    bool failed = false;
    bool init() {
        if (ring) return true;
        if (failed) return false;
        try { ring = qb3host::ring_acquire(); } catch (...) { ring = nullptr; }
        failed = !ring;
        return ring != nullptr;
    }
    void release() { try { qb3host::ring_release(ring); } catch (...) {} ring = nullptr; }
    uint8_t *slot(size_t i) const { return ring->slot[i % NSLOT]; }
    hipEvent_t ev(size_t i) const { return ring->ev[i % NSLOT]; }
};
// Streams and events of a pipelined host call (upload, kernels and download of different strips at once), kept by the handle
struct Pipe {
    hipStream_t up = nullptr, k = nullptr, dn = nullptr;
    std::vector<hipEvent_t> ev;
    uint64_t *words = nullptr;                      // pinned: a few result words the kernel stream copies down (WORDS of them)
    static constexpr size_t WORDS = 2048;
    bool failed = false;
    bool init();
    bool events(size_t n);
    void sync() { if (up) { (void)hipStreamSynchronize(up); (void)hipStreamSynchronize(k); (void)hipStreamSynchronize(dn); } }
    void release();
};

// ---------------------------------------------------------------- the handles (qb3_api.cpp: lifetime and setters)
struct band_state { size_t prev, runbits, cf; };

struct encs {
    size_t xsize, ysize, nbands, stride;
    uint64_t order, quanta;
    band_state band[QB3_MAXBANDS];
    size_t cband[QB3_MAXBANDS];
    int error;
    qb3_mode mode;
    qb3_dtype type;
    bool away;
    int ix_chunk;           // qb3x_set_encoder_index_chunk: embed the restart table ("ix" chunks); 2: with block lengths
    DevBuf d_img, d_out, d_ws, d_q, d_idx, d_rle;      // d_rle: workspace of the RLE0 passes (k_rle0.hip)
    DevBuf d_mos;                                      // qb3x_encode_mosaic: the edge tiles' descriptors and their replicated images
    Stager stager, stager2;                            // (stager2: the download ring of a pipelined host call)
    Pipe pipe;                                         // ... its streams and events
};

struct decs {
    size_t xsize, ysize, nbands, stride;
    uint64_t order, quanta;
    int error, stage;
    uint8_t cband[QB3_MAXBANDS];
    qb3_mode mode;
    qb3_dtype type;
    uint8_t *s_in;
    size_t s_size;
    uint8_t *s_start;       // the pointer given to qb3_read_start
    bool saw_cb;            // a CB chunk was present
    unsigned compat;
    size_t hdr_avail;       // bytes readable at s_start (the whole stream, or the header copy given to qb3x_read_start)
    size_t ix_off;          // restart table found in the container: offset of its first chunk from s_start (0: none)
    uint32_t ix_K, ix_blocks, ix_E, ix_per_chunk;
    bool ix_bl;             // ... its entries carry block lengths
    bool ix_pads, ix_bad;   // pad chunks behind the table chunks (version 2); the chunks seen do not form one table
    uint32_t ix_ver;        // version of the table's chunks (3: each carries a check of its entries)
    bool ix_heads_unchecked;    // the parser stepped over a regular table in one go: the chunk heads behind the first are checked on the device
    bool hdr_short;         // qb3_read_info read beyond the host copy of the header (whatever it then made of the zeros it got)
    size_t ix_need_off;     // ... and would have, but the bytes at this offset from s_start (the "DT" behind the table) are not on the host (0: no)
    std::vector<uint8_t> own_head, win2;    // qb3x_read_start_device: the handle's own copy of the container's first bytes, and of a few bytes further on
    size_t win2_off = 0;    // ... at this offset from s_start
    std::vector<uint8_t> tile_ok;   // qb3x_decode_tiles: per tile outcome of the last call
    uint32_t last_status = 0;       // status bits of the last decode call (qb3x_last_decode_status; tiles: of all tiles together)
    DevBuf d_in, d_img, d_ws, d_ix, d_rle, d_tab;      // d_rle: RLE0 workspace (+ the packed bytes of a host call); d_tab: the unit-length table a plain 8-bit stream is walked through
    DevBuf d_win, d_wst, d_wout, d_wsrc;               // window calls: the raster a strip or a whole decode goes to before the crop; the window kernel's status word; a host call's window and container
    int win_path = 0;                                  // ... which way the last one went (qb3x_last_window_path) and how many segments it decoded
    size_t win_segs = 0;
    unsigned win_kernels = 0;                          // qb3x_set_decoder_window_kernels: rasters beyond path 1's own that take a window kernel (the families' switches)
    DevBuf d_wdesc;                                    // a batch of windows: descriptors and the list of table chunks to check, as uploaded
    PinBuf h_wdesc, h_wst;                             // ... their pinned host copy (one copy up), and the status words (one copy back)
    std::vector<uint8_t> wins_path;                    // ... per window outcome of the last batch call (0: not written, else its path)
    DevBuf d_wfull, d_wgat;                            // band-selected windows (api_window_bands.cpp): full-band windows a window kernel wrote for the gather; the gather's descriptors
    PinBuf h_wgat;                                     // ... their pinned host copy
    size_t win_gathers = 0;                            // ... gather launches of the last band-selected call (qb3x_last_window_gathers)
    DevBuf d_mos;                                      // qb3x_decode_mosaic: the edge tiles' descriptors and the whole tiles they decode to; qb3x_decode_mosaic_windows: the same for the tiles it decodes whole
    size_t mos_whole = 0;                              // ... tiles the last qb3x_decode_mosaic_windows decoded whole (qb3x_last_mosaic_whole_tiles)
    Stager stager, stager2;                            // (stager2: the download ring of a pipelined host call)
    Pipe pipe;                                         // ... its streams and events
    // a ranged handle (qb3x_open_ranged, api_ranged.cpp): the caller's reader, the container's size, what the last call asked of the reader
    qb3x_read_fn rg_rd = nullptr;
    void *rg_ctx = nullptr;
    uint64_t rg_size = 0, rg_bytes = 0, rg_reads = 0;
    size_t rg_gap = 0, rg_cache_cap = (size_t)64 << 20, rg_cache_bytes = 0;
    std::vector<std::pair<uint32_t, std::vector<uint8_t>>> rg_chunks;      // verified table chunks by number, oldest first
    PinBuf h_rg;                                       // ... pieces, entries, piece list and descriptors as uploaded
    DevBuf d_rg;
};

namespace qb3api {

inline size_t szof(int dt) {                                // bytes of a value
    constexpr int typesizes[8] = { 1, 1, 2, 2, 4, 4, 8, 8 };
    return (dt < 0 || dt > QB3_I64) ? 0 : typesizes[dt];
}
inline bool is_rle_mode(int m) { return m == QB3M_RLE || m == QB3M_CF_RLE || m == QB3M_RLE_H || m == QB3M_CF_RLE_H; }

// No C++ exception crosses the C ABI: a failed allocation (std::vector, std::thread) inside a call is an error return with
// a message for qb3x_last_error, not std::terminate in the caller's process
template <class R, class F> R abi_guard(R fail, F &&f) noexcept {
    try { return f(); }
    catch (const std::exception &e) { qb3dev::set_error(e.what(), -1); }
    catch (...) { qb3dev::set_error("C++ exception inside the library", -1); }
    return fail;
}

// api_mem.cpp
void release_all(std::initializer_list<DevBuf *> bufs);    // one wait for the device, then every buffer
bool device_ok();
hipError_t wait_stream(hipStream_t st);
hipError_t fetch_small(void *dst, const void *d_src, size_t n, hipStream_t st);
bool upload(Stager &sg, void *d_dst, const void *h_src, size_t bytes, hipStream_t st);
bool download(Stager &sg, void *h_dst, const void *d_src, size_t bytes, hipStream_t st);

// api_header.cpp
size_t write_headers(const encs *p, uint8_t *dst, bool with_dt = true);
decsp read_start_impl(void *source, size_t hdr_avail, size_t source_size, size_t *image_size);
qb3dev::IxTable handle_table(const decs *p, const uint8_t *base);
qb3dev::Geometry decoder_geometry(const decs *p, size_t w, size_t h, size_t stride);

// api_tiles.cpp: equally shaped tiles of one call that go through one set of launches.  Tile u is tile (u / cols, u % cols) of a grid:
// its image img_row bytes down and img_col bytes along from `img`, its container (size, index, outcome) number k0 + (u / cols) * k_row +
// u % cols of the call's.  n is a multiple of cols; tiles back to back are one row (cols == n).  The mosaic calls (api_mosaic.cpp) hand
// in up to three grids: the tiles inside the raster where they lie, the bottom row and the right column in memory of the handle's.
struct TileGrid {
    size_t n, cols;
    const void *img;            // encode: the source; decode: the destination
    size_t img_col, img_row;
    size_t stride;              // values between the pixel rows of a tile (0: tight); the handle's own setting is set aside for the call
    size_t k0, k_row;
};
size_t encode_tile_grids(encsp p, const TileGrid *grids, size_t ngrids, void *d_dst, size_t dst_pitch, void *d_index, size_t *sizes, void *stream);
size_t decode_tile_grids(decsp p, const void *d_src, size_t n, size_t src_pitch, const size_t *sizes, const TileGrid *grids, size_t ngrids,
                         const void *d_index, void *stream);

// what the window calls say once (api_window.cpp, api_ranged.cpp): values between the destination's rows; is the rectangle inside the raster
inline size_t win_stride(const decs *p, const qb3x_window &w) { return w.dst_stride ? w.dst_stride : w.w * p->nbands; }
inline bool window_inside(const decs *p, size_t x0, size_t y0, size_t w, size_t h) {
    return w && h && x0 < p->xsize && w <= p->xsize - x0 && y0 < p->ysize && h <= p->ysize - y0;
}
// sorts ranges [first, second) and merges those that overlap, touch or lie within `gap` of each other
template <class T> inline void merge_ranges(std::vector<std::pair<T, T>> &r, T gap = 0) {
    std::sort(r.begin(), r.end());
    size_t m = 0;
    for (size_t i = 1; i < r.size(); i++) {
        if (r[i].first - std::min(r[i].first, r[m].second) <= gap) r[m].second = std::max(r[m].second, r[i].second);
        else r[++m] = r[i];
    }
    if (!r.empty()) r.resize(m + 1);
}
// the family of window kernels that takes a raster (qb3_dev.h: window_family), if every one of these device destinations meets its
// alignment; else none, and the call goes the way of a raster no family takes
inline const qb3dev::WinKernels *family_if_aligned(const qb3dev::WinKernels *fam, const qb3dev::Geometry &g, const qb3x_window *wins, size_t n) {
    for (size_t i = 0; fam && i < n; i++) if ((uintptr_t)wins[i].dst & (fam->align(g) - 1)) fam = nullptr;
    return fam;
}

// api_window.cpp: handle and rectangles of a window call (false: p->error is set); the windows of a container in device / host memory
// (paths: a zeroed byte per window, which receives the path its pixels came by); host destinations' stand-ins in the handle's d_wout,
// back to back with tight rows, each on a dword (false: no memory); the window as a raster of its own, dequantised (false: a HIP failure)
bool windows_check(decsp p, const qb3x_window *wins, size_t n, bool host);
bool windows_out(decsp p, const qb3x_window *wins, size_t n, std::vector<void *> &dsts);
bool window_dequantize(decsp p, const qb3dev::Geometry &g, void *dst, size_t w, size_t h, size_t stride, hipStream_t st);
size_t windows_device(decsp p, const void *d_src, const void *d_index, const qb3x_window *wins, size_t n, uint8_t *paths, bool single, hipStream_t st);
size_t windows_host(decsp p, const qb3x_window *wins, size_t n, uint8_t *paths, bool single);
// ... and what the band-selected calls (api_window_bands.cpp) take from there: the container as the kernels take it, the batch of a family
// (sel: its band-selected form, the rectangles' strides then count nsel values a pixel; extra: bytes that go up behind the descriptors and the
// chunk list in the same copy, *d_extra: where they are then), the strips of path 2 (crop: into the windows; else only the scratch raster)
struct WinSrc { qb3dev::Geometry g; qb3dev::DecPlan plan; qb3dev::IxTable ixt; const uint32_t *in32; uint32_t in_bit0; uint64_t in_bits; };
WinSrc window_source(const decs *p, const qb3dev::Geometry &g, const void *d_src);
struct WinSel { const uint8_t *sel; uint32_t nsel; const void *extra; size_t extra_bytes; const void **d_extra; };
bool window_kernel_batch(decsp p, const WinSrc &s, const qb3x_window *wins, size_t n, uint8_t *paths, size_t *segs, hipStream_t st, const qb3dev::WinKernels &fam,
                         const WinSel *ws = nullptr);
bool window_strips(decsp p, const WinSrc &s, const qb3x_window *wins, size_t n, uint8_t *paths, size_t *segs, hipStream_t st, bool crop = true);

// qb3_api.cpp
qb3dev::Geometry make_geometry(size_t w, size_t h, size_t bands, int dtype, size_t stride, uint64_t order, int mode,
                               const size_t *cband_sz, const uint8_t *cband_u8);
size_t ix_room(const encs *p);
bool walk_table_ready(decsp p, const qb3dev::Geometry &g, const qb3dev::DecPlan &plan, uint32_t ntiles, uint64_t max_bits);
size_t decode_common(decsp p, void *host_dst, const void *d_src, void *d_dst, const void *d_index, hipStream_t st);

}  // namespace qb3api
