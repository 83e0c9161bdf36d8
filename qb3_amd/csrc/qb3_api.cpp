// qb3_amd/csrc/qb3_api.cpp -- the C ABI (include/QB3.h, include/qb3x.h) of the MI355X-native QB3 codec.
//
// Host side only.  This file: the handles' lifetime and setters and the whole-raster calls (qb3_encode / qb3x_encode_device,
// qb3_read_data / qb3x_decode_device) with their strip pipelines and the STORED fallback (the RLE0 byte pass is a device pass:
// k_rle0.hip).  Memory and copies: api_mem.cpp; container headers: api_header.cpp; tile batches: api_tiles.cpp; windows:
// api_window.cpp; reindex: api_reindex.cpp; what they share: qb3_host.h.  The block coding itself -- the hot
// path -- is in the k_*.hip files and always runs on the GPU; there is no CPU fallback for it.
//
// Behaviour mirrors the reference C API (reference QB3lib/QB3encode.cpp, QB3decode.cpp), including the
// quirks a drop-in has to keep: band state carried across qb3_encode calls until qb3_reset_encoder
// (QB3encode.h:446-449), sticky Z order (QB3encode.cpp:124-132), mode left at STORED after a fallback
// (QB3encode.cpp:464), stale error blocking the handle (QB3encode.cpp:514).
#include <chrono>
#include <new>
#include <limits>
#include <thread>
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

static size_t raw_size(const encs *p) { return p->xsize * p->ysize * p->nbands * szof(p->type); }

// ---------------------------------------------------------------- geometry helpers
static CodecMode codec_mode(int mode) {
    if (mode == QB3M_FTL) return CM_FTL;
    if (mode == QB3M_BASE_H || mode == QB3M_BASE_Z || mode == QB3M_RLE || mode == QB3M_RLE_H) return CM_BASE;   // RLE0 only wraps the BASE stream
    return CM_BEST;
}

Geometry qb3api::make_geometry(size_t w, size_t h, size_t bands, int dtype, size_t stride, uint64_t order, int mode,
                              const size_t *cband_sz, const uint8_t *cband_u8) {
    Geometry g;
    memset(&g, 0, sizeof(g));
    g.w = (uint32_t)w; g.h = (uint32_t)h; g.bands = (uint32_t)bands; g.tsz = (uint32_t)szof(dtype);
    g.stride = stride ? stride : w * bands;
    g.order = order ? order : HILBERT;
    g.nbx = (uint32_t)((w + 3) / 4); g.nby = (uint32_t)((h + 3) / 4);
    g.nblocks = (uint64_t)g.nbx * g.nby;
    g.mode = codec_mode(mode);
    g.ulen_sz = ulen_size_for(g.tsz, g.mode, g.bands);
    for (size_t c = 0; c < bands; c++) g.cband[c] = cband_sz ? (uint8_t)cband_sz[c] : cband_u8[c];
    g.seg_blocks = seg_blocks_for(g);
    g.nseg = (g.nblocks + g.seg_blocks - 1) / g.seg_blocks;
    return g;
}

// ---------------------------------------------------------------- encoder handle
QB3_API encsp qb3_create_encoder(size_t w, size_t h, size_t b, qb3_dtype dt) {
    if (w == 0 || w > 0x10000 || h == 0 || h > 0x10000 || b == 0 || b > QB3_MAXBANDS || (int)dt < 0 || (int)dt > (int)QB3_I64)
        return nullptr;
    encs *p = new (std::nothrow) encs();
    if (!p) return nullptr;
    p->xsize = w; p->ysize = h; p->nbands = b; p->type = dt;
    p->stride = 0; p->order = 0; p->quanta = 1; p->away = false; p->mode = QB3M_DEFAULT; p->error = 0;
    { const char *e = getenv("QB3X_INDEX_CHUNK"); p->ix_chunk = e ? (atoi(e) >= 2 ? 2 : atoi(e) != 0) : 0; }
    for (size_t c = 0; c < QB3_MAXBANDS; c++) p->cband[c] = c < b ? c : 0;
    if (b == 3 || b == 4) p->cband[0] = p->cband[2] = 1;
    qb3_reset_encoder(p);
    return p;
}

QB3_API void qb3_reset_encoder(encsp p) {
    for (size_t c = 0; c < QB3_MAXBANDS; c++) p->band[c].prev = p->band[c].runbits = p->band[c].cf = 0;
    p->error = 0;
}

QB3_API void qb3_destroy_encoder(encsp p) {
    if (!p) return;
    release_all({&p->d_img, &p->d_out, &p->d_ws, &p->d_q, &p->d_idx, &p->d_rle, &p->d_mos});
    p->stager.release(); p->stager2.release(); p->pipe.release();
    delete p;
}

QB3_API bool qb3_set_encoder_coreband(encsp p, size_t b, size_t *bands) {
    if (b != p->nbands) return false;
    for (size_t i = 0; i < b; i++) p->cband[i] = (uint8_t)((bands[i] < b) ? bands[i] : i);
    for (size_t i = 0; i < b; i++) if (p->cband[i] != i) p->cband[p->cband[i]] = p->cband[i];
    for (size_t i = 0; i < b; i++) bands[i] = p->cband[i];
    return true;
}

QB3_API void qb3_set_encoder_stride(encsp p, size_t stride) { p->stride = stride; }

QB3_API bool qb3_set_encoder_quanta(encsp p, uint64_t q, bool away) {
    if (q < 1) return false;
    p->quanta = q; p->away = away;
    if (q == 1) return true;
    // the reference's fall-through range switch (QB3encode.cpp:96-107): a type is checked against its own
    // limit and against the limits of every wider type listed after it
    static const int order[7] = { QB3_I8, QB3_U8, QB3_I16, QB3_U16, QB3_I32, QB3_U32, QB3_I64 };
    static const uint64_t lim[7] = { 0x7f, 0xff, 0x7fff, 0xffff, 0x7fffffff, 0xffffffffull, 0x7fffffffffffffffull };
    bool bad = false;
    int start = -1;
    for (int i = 0; i < 7; i++) if (order[i] == (int)p->type) start = i;
    for (int i = start; i >= 0 && i < 7; i++) bad |= q > lim[i];
    return !bad;
}

// reference QB3encode.cpp:112-118
static size_t max_encoded_size_ref(const encs *p) {
    size_t n = 16 * ((p->xsize + 3) / 4) * ((p->ysize + 3) / 4) * p->nbands;
    double bits_per_value = 17.0 / 16.0 + 8 * szof(p->type);
    return 1024 + static_cast<size_t>(bits_per_value * n / 8);
}
// bytes the restart-table chunks add to a container of this handle (0: none would be written)
size_t qb3api::ix_room(const encs *p) {
    if (!p->ix_chunk || p->xsize < 4 || p->ysize < 4 || p->xsize * p->ysize <= 16) return 0;
    // The bound must not depend on the mode (not even on QB3M_STORED, where a raw fallback leaves a handle: a caller that
    // sizes its buffer again then, and sets a coding mode afterwards, must not get less than the next call writes): the reference's callers size the buffer right after qb3_create_encoder and BEFORE
    // qb3_set_encoder_mode (reference cqb3.cpp:405-464, test_qb3.cpp:84-102).  The largest table any mode would write for this
    // raster: FTL and BASE streams share a layout, the common-factor modes have another.
    size_t room = 0;
    for (int m : {(int)QB3M_FTL, (int)QB3M_CF_H}) {
        const Geometry g = make_geometry(p->xsize, p->ysize, p->nbands, p->type, p->stride, p->order, m, p->cband, nullptr);
        room = std::max(room, ix_total_bytes(ix_layout(g, p->ix_chunk)));
    }
    return room;
}
QB3_API size_t qb3_max_encoded_size(const encsp p) { return max_encoded_size_ref(p) + ix_room(p); }

QB3_API qb3_mode qb3_set_encoder_mode(encsp p, qb3_mode mode) {
    if ((int)mode >= 0 && (int)mode < (int)QB3M_END) p->mode = mode;
    if ((int)p->mode <= (int)QB3M_CF_RLE) p->order = ZCURVE;
    return p->mode;
}

QB3_API int qb3_get_encoder_state(encsp p) { return p->error; }

// narrow-image remap (reference QB3encode.cpp:351-389, implemented per its intent; the reference itself has
// a use-after-scope there).  Returns the packed pixels, sets the stand-in dimensions.
static std::vector<uint8_t> remap_small(const uint8_t *src, size_t w, size_t h, size_t pix, size_t stride_bytes,
                                        size_t &nw, size_t &nh) {
    const size_t ngroups = (w * h + 15) / 16;
    std::vector<uint8_t> t(ngroups * 16 * pix, 0);
    uint8_t *d = t.data();
    if (w < 4) {
        for (size_t y = 0; y < h; y++, d += w * pix) memcpy(d, src + y * stride_bytes, w * pix);
        nw = 4; nh = ngroups * 4;
    } else {
        for (size_t x = 0; x < w; x++)
            for (size_t y = 0; y < h; y++, d += pix) memcpy(d, src + y * stride_bytes + x * pix, pix);
        nw = ngroups * 4; nh = 4;
    }
    return t;
}

// (RLE0, reference QB3encode.cpp:271-332 / QB3decode.cpp:267-307, runs on the device: k_rle0.hip)

// ---------------------------------------------------------------- encode
static size_t stored_encode_host(encsp p, const void *source, void *destination) {
    uint8_t *d = (uint8_t *)destination;
    p->mode = QB3M_STORED;
    const size_t hdr = write_headers(p, d);
    if (p->error) return 0;
    const size_t tsz = szof(p->type), line = p->xsize * p->nbands * tsz;
    const size_t stride = (p->stride ? p->stride : p->xsize * p->nbands) * tsz;
    for (size_t y = 0; y < p->ysize; y++) memcpy(d + hdr + y * line, (const uint8_t *)source + y * stride, line);
    return hdr + raw_size(p);
}

// Runs the block coder on a device image.  d_out mirrors the destination buffer: the stream starts at byte
// `hdr`.  On success *bits receives the stream length; the handle's band state is updated when `carry`.
// d_index may be null.  Synchronises the stream.
static bool encode_blocks_device(encsp p, const Geometry &g, const void *d_img, uint8_t *d_out, size_t hdr,
                                 void *d_index, hipStream_t st, bool carry, uint64_t *bits, const uint8_t *hdrbytes,
                                 size_t hdr_stamp, const IxTable &ix, int *zero_run = nullptr) {
    EncPlan plan = plan_encode(g, value_aligned_memory(g.tsz, (uintptr_t)d_img));
    if (!p->d_ws.ensure(plan.ws_bytes)) return false;
    EncJob job;
    memset(&job.st, 0, sizeof(job.st));
    for (size_t c = 0; c < p->nbands; c++) {
        job.st.prev[c] = p->band[c].prev; job.st.cf[c] = p->band[c].cf; job.st.rung[c] = (uint8_t)p->band[c].runbits;
    }
    job.img = d_img; job.out32 = (uint32_t *)(d_out + (hdr & ~(size_t)3)); job.out_bit0 = (uint32_t)(8 * (hdr & 3));
    job.ws = p->d_ws.p; job.index = d_index;
    job.hdr = hdrbytes; job.hdr_len = (uint32_t)hdr_stamp; job.ix = ix; job.zrun_probe = zero_run != nullptr;
    EncResult res;
    const uint8_t *dres = (const uint8_t *)p->d_ws.p + plan.ws_bytes - sizeof(EncResult);
    if (launch_encode(g, plan, job, st)) return false;
    const hipError_t e = fetch_small(&res, dres, sizeof(res), st);
    if (e != hipSuccess) { set_error("encode kernels", (int)e); return false; }
    prof_collect();
    *bits = res.total_bits;
    // (a chunk of the stream holds plan.nbp blocks of at least two bits a unit)
    { static const bool dbg = getenv("QB3_DEBUG_RLE") != nullptr; if (dbg && zero_run) fprintf(stderr, "encode: zero_run %llu ff_pairs %llu zero_dwords %llu (%u chunks)\n", (unsigned long long)res.zero_run, (unsigned long long)res.ff_pairs, (unsigned long long)res.zero_dwords, plan.nchunks); }
    if (zero_run) *zero_run = rle0_may_win(res) ? (rle0_no_uniform_chunk(res, (uint64_t)plan.nbp * g.bands / 4) ? 2 : 1) : 0;      // (2: and no 4 KB of the stream hold one byte value only)
    if (carry)
        for (size_t c = 0; c < p->nbands; c++) {
            p->band[c].prev = (size_t)res.prev[c]; p->band[c].runbits = res.rung[c]; p->band[c].cf = (size_t)res.cf[c];
        }
    return true;
}

// Puts the caller's mode back on every exit but the ones that are meant to change it (the reference leaves a handle
// at QB3M_STORED after a raw fallback, QB3encode.cpp:464, and demotes RLE modes only for the block pass, :495-506).
struct ModeGuard {
    encs *p; qb3_mode mode; bool armed = true;
    ModeGuard(encs *h) : p(h), mode(h->mode) {}
    ~ModeGuard() { if (armed) p->mode = mode; }
};


// ---------------------------------------------------------------- qb3_encode, pipelined
// The raster goes up the link in slices; as soon as the rows of a STRIP (a scan group of chunks, about 50 MB of an 8-bit RGB
// raster) are in device memory the strip is coded, scanned, moved into place and sealed (launch_encode_strip) -- its bits start
// where the strips before it ended, the dependency only points backwards -- and the part of the stream that is final comes
// down the link while later strips are still going up.  Three streams, two rings of pinned slices, host copies by the pool.
// Returns 1: the stream (and its table) is in host_dst behind the header's place, *bits_out and the handle's band state are
// set; 0: not taken (the caller goes the one-after-the-other way); -1: failed (p->error set).
static int encode_pipelined(encsp p, const Geometry &g, const void *host_src, void *host_dst, size_t src_bytes, size_t line, uint8_t *out_dev, size_t hdr,
                            const uint8_t *hdrbuf, size_t hdr_stamp, const IxTable &ixt, void *d_index, bool carry, uint64_t *bits_out) {
    using qb3host::CopyPool;
    constexpr size_t SLICE = Stager::SLICE, NSLOT = Stager::NSLOT;
    static const bool dbg = getenv("QB3_DEBUG_PIPE") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    const EncPlan plan = plan_encode(g);
    if (!encode_strips_ok(g, plan)) return 0;
    const uint32_t nstrips = encode_strip_count(plan);
    if (nstrips < 3 || nstrips + 64 > Pipe::WORDS) return 0;
    if (!p->pipe.init() || !p->pipe.events((size_t)nstrips + 1) || !p->stager.init() || !p->stager2.init()) return 0;
    if (!p->d_img.ensure(src_bytes) || !p->d_ws.ensure(plan.ws_bytes)) { p->error = QB3E_LIBERR; return -1; }
    const uint32_t out_bit0 = (uint32_t)(8 * (hdr & 3));
    EncJob job;             // of every strip and of the tail
    memset(&job.st, 0, sizeof(job.st));
    for (size_t c = 0; c < p->nbands; c++) { job.st.prev[c] = p->band[c].prev; job.st.cf[c] = p->band[c].cf; job.st.rung[c] = (uint8_t)p->band[c].runbits; }
    job.img = p->d_img.p; job.out32 = (uint32_t *)(out_dev + (hdr & ~(size_t)3)); job.out_bit0 = out_bit0;
    job.ws = p->d_ws.p; job.index = d_index;
    job.hdr = hdrbuf; job.hdr_len = (uint32_t)hdr_stamp; job.ix = ixt;
    // raster bytes a strip needs in device memory: the rows of its last block (the block before its first one is in the strip before)
    std::vector<size_t> need(nstrips);
    for (uint32_t s = 0; s < nstrips; s++) {
        const uint64_t blocks = std::min<uint64_t>(g.nblocks, encode_strip_blocks(plan, s));
        const uint64_t brow = (blocks - 1) / g.nbx;
        need[s] = std::min(src_bytes, (size_t)std::min<uint64_t>(g.h, 4 * (brow + 1)) * line);
    }
    need[nstrips - 1] = src_bytes;
    struct Slice { const uint8_t *dev; uint8_t *host; size_t n; };
    std::vector<Slice> dn;
    const size_t n_up = (src_bytes + SLICE - 1) / SLICE;
    CopyPool &pool = CopyPool::get();
    CopyPool::Batch b_up[NSLOT], b_dn[NSLOT];
    Stager &r1 = p->stager, &r2 = p->stager2;
    hipStream_t sU = p->pipe.up, sK = p->pipe.k, sD = p->pipe.dn;
    uint64_t *totals = p->pipe.words;                       // [s]: stream bits behind strip s; behind them the EncResult
    EncResult *res_host = (EncResult *)(totals + nstrips);
    const uint8_t *dres = (const uint8_t *)p->d_ws.p + plan.ws_bytes - sizeof(EncResult);
    size_t up_started = 0, up_enq = 0, bytes_enq = 0, dn_issued = 0, dn_copy = 0, dn_freed = 0, x_prev = hdr;
    uint32_t next_strip = 0, known = 0;
    bool tail_seen = false, launch_failed = false;
    hipError_t e = hipSuccess;
    auto ok = [&] { return e == hipSuccess && !launch_failed; };
    auto add_span = [&](size_t a, size_t b) {               // bytes [a, b) of the container are final in device memory
        for (size_t off = a; off < b; off += SLICE) dn.push_back({out_dev + off, (uint8_t *)host_dst + off, std::min(SLICE, b - off)});
    };
    const double t_setup = ms_since();
    double t_up_done = 0, t_first_dn = 0;
    while (ok() && (up_enq < n_up || !tail_seen || dn_freed < dn.size())) {
        bool progress = false;
        // ---- up
        if (up_started < n_up && up_started - up_enq < 2 && (up_started < NSLOT || hipEventQuery(r1.ev(up_started)) == hipSuccess)) {
            const size_t off = up_started * SLICE;
            pool.submit(r1.slot(up_started), (const uint8_t *)host_src + off, std::min(SLICE, src_bytes - off), b_up[up_started % NSLOT]);
            up_started++; progress = true;
        }
        if (up_enq < up_started && pool.done(b_up[up_enq % NSLOT])) {
            const size_t off = up_enq * SLICE, n = std::min(SLICE, src_bytes - off);
            e = hipMemcpyAsync((uint8_t *)p->d_img.p + off, r1.slot(up_enq), n, hipMemcpyHostToDevice, sU);
            if (e == hipSuccess) e = hipEventRecord(r1.ev(up_enq), sU);
            bytes_enq += n;
            up_enq++; progress = true;
            if (dbg && up_enq == n_up) t_up_done = ms_since();
            while (ok() && next_strip < nstrips && need[next_strip] <= bytes_enq) {
                hipEvent_t ev_u = p->pipe.ev[nstrips];     // (one event for "the rows are on their way": recorded and waited for at once)
                e = hipEventRecord(ev_u, sU);
                if (e == hipSuccess) e = hipStreamWaitEvent(sK, ev_u, 0);
                if (e != hipSuccess) break;
                if (launch_encode_strip(g, plan, job, sK, next_strip)) { launch_failed = true; break; }
                e = hipMemcpyAsync(&totals[next_strip], encode_strip_total(g, plan, p->d_ws.p, next_strip), 8, hipMemcpyDeviceToHost, sK);
                if (e == hipSuccess && next_strip + 1 == nstrips) {        // behind the last strip: index positions, the table, the result words
                    if (launch_encode_tail(g, plan, job, sK)) { launch_failed = true; break; }
                    e = hipMemcpyAsync(res_host, dres, sizeof(EncResult), hipMemcpyDeviceToHost, sK);
                }
                if (e == hipSuccess) e = hipEventRecord(p->pipe.ev[next_strip], sK);
                next_strip++;
            }
        }
        // ---- a strip is done: what is final behind it (all but the dword its end falls into; the last strip: everything, and the table)
        if (ok() && known < next_strip) {
            const hipError_t q = hipEventQuery(p->pipe.ev[known]);
            if (q == hipSuccess) {
                const uint64_t P = totals[known];
                const bool last = known + 1 == nstrips;
                const size_t x = last ? hdr + (size_t)((P + 7) / 8) : (hdr & ~(size_t)3) + 4 * (size_t)((out_bit0 + P) >> 5);
                if (x > x_prev) { add_span(x_prev, x); x_prev = x; }
                if (last) { if (hdr > hdr_stamp) add_span(hdr_stamp, hdr); tail_seen = true; }
                known++; progress = true;
            } else if (q != hipErrorNotReady) e = q;
        }
        // ---- down
        if (ok() && dn_issued < dn.size() && dn_issued - dn_freed < NSLOT) {
            e = hipMemcpyAsync(r2.slot(dn_issued), dn[dn_issued].dev, dn[dn_issued].n, hipMemcpyDeviceToHost, sD);
            if (e == hipSuccess) e = hipEventRecord(r2.ev(dn_issued), sD);
            dn_issued++; progress = true;
        }
        if (ok() && dn_copy < dn_issued) {
            const hipError_t q = hipEventQuery(r2.ev(dn_copy));
            if (q == hipSuccess) { if (dbg && !dn_copy) t_first_dn = ms_since(); pool.submit(dn[dn_copy].host, r2.slot(dn_copy), dn[dn_copy].n, b_dn[dn_copy % NSLOT]); dn_copy++; progress = true; }
            else if (q != hipErrorNotReady) e = q;
        }
        while (dn_freed < dn_copy && pool.done(b_dn[dn_freed % NSLOT])) { dn_freed++; progress = true; }
        if (!progress && !pool.help_one()) std::this_thread::yield();
    }
    (void)hipGetLastError();                                // (hipErrorNotReady of the queries is not an error)
    for (size_t i = 0; i < NSLOT; i++) { pool.wait(b_up[i]); pool.wait(b_dn[i]); }
    p->pipe.sync();
    if (dbg) fprintf(stderr, "encode_pipelined: setup %.2f ms, last upload enqueued %.2f, first slice down %.2f, done %.2f (%u strips, %zu + %zu slices)\n", t_setup, t_up_done, t_first_dn, ms_since(), nstrips, n_up, dn.size());
    if (!ok()) { if (!launch_failed) set_error("pipelined encode", (int)e); p->error = QB3E_LIBERR; return -1; }
    prof_collect();
    *bits_out = res_host->total_bits;
    if (carry)
        for (size_t c = 0; c < p->nbands; c++) {
            p->band[c].prev = (size_t)res_host->prev[c]; p->band[c].runbits = res_host->rung[c]; p->band[c].cf = (size_t)res_host->cf[c];
        }
    return 1;
}

// Shared by qb3_encode (host buffers) and qb3x_encode_device (device buffers).
// host_src/host_dst are null in the device flavour; d_src/d_dst are null in the host flavour.
static size_t encode_common(encsp p, const void *host_src, void *host_dst, const void *d_src, void *d_dst,
                            void *d_index, hipStream_t st) {
    const bool on_host = host_src != nullptr;
    const size_t tsz = szof(p->type), line = p->xsize * p->nbands * tsz;
    const size_t src_stride_bytes = (p->stride ? p->stride : p->xsize * p->nbands) * tsz;
    const size_t src_span = src_stride_bytes * (p->ysize - 1) + line;      // bytes from the first to the last pixel
    if (p->xsize * p->ysize <= 16) {        // tiny images are stored (reference QB3encode.cpp:490)
        if (on_host) return stored_encode_host(p, host_src, host_dst);
        std::vector<uint8_t> tmp(src_span), out(64 + raw_size(p));
        if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }
        HIPOK(hipMemcpyAsync(tmp.data(), d_src, tmp.size(), hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        size_t n = stored_encode_host(p, tmp.data(), out.data());
        HIPOK(hipMemcpyAsync(d_dst, out.data(), n, hipMemcpyHostToDevice, st));
        HIPOK(hipStreamSynchronize(st));
        return n;
    }
    ModeGuard guard(p);
    const qb3_mode mode = p->mode;
    const bool rle = is_rle_mode(mode);
    const size_t ixroom = mode == QB3M_STORED ? 0 : ix_room(p);   // (a handle left at STORED writes no table)
    if (rle) p->mode = (qb3_mode)((int)mode - 2);       // RLE is a post pass over the base mode's stream
    uint8_t hdrbuf[80];
    size_t hdr = write_headers(p, hdrbuf);
    if (p->error) return 0;                               // stale error blocks the handle until reset
    if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }

    // geometry, with the narrow-image stand-in where needed
    size_t w = p->xsize, h = p->ysize, stride = p->stride;
    const void *img_dev = d_src;
    std::vector<uint8_t> small;
    const bool narrow = w < 4 || h < 4;
    if (narrow) {
        std::vector<uint8_t> tmp;
        const uint8_t *hs = (const uint8_t *)host_src;
        if (!on_host) {
            tmp.resize(src_span);
            HIPOK(hipMemcpyAsync(tmp.data(), d_src, tmp.size(), hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
            hs = tmp.data();
        }
        small = remap_small(hs, p->xsize, p->ysize, p->nbands * tsz, src_stride_bytes, w, h);
        stride = 0;
    }
    // a large raster in host memory, coded as it is: upload, coding and download strip by strip, all three at once (encode_pipelined)
    static const bool no_pipeline = [] { const char *e = getenv("QB3_NO_PIPELINE"); return e && e[0] && e[0] != '0'; }();
    bool want_pipe = on_host && !narrow && !rle && p->quanta < 2 && src_stride_bytes == line && src_span >= ((size_t)64 << 20) && !no_pipeline;
    auto upload_now = [&]() -> bool {
        const uint8_t *hs = narrow ? small.data() : (const uint8_t *)host_src;
        const size_t bytes = narrow ? small.size() : src_span;
        return p->d_img.ensure(bytes) && upload(p->stager, p->d_img.p, hs, bytes, st);
    };
    if (on_host || narrow) {
        if (!want_pipe && !upload_now()) { p->error = QB3E_LIBERR; return 0; }
        if (want_pipe && !p->d_img.ensure(src_span)) { p->error = QB3E_LIBERR; return 0; }
        img_dev = p->d_img.p;
    }
    Geometry g = make_geometry(w, h, p->nbands, p->type, stride, p->order, p->mode, p->cband, nullptr);
    if (p->quanta >= 2) {
        // quantise into a compact device copy; like the reference (QB3encode.cpp:405-455) the band state then
        // lives on a copy of the handle and is not carried back
        if (!p->d_q.ensure((size_t)g.w * g.h * g.bands * tsz)) { p->error = QB3E_LIBERR; return 0; }
        if (launch_quantize(p->d_q.p, img_dev, g, (int)p->type, p->quanta, p->away, st)) { p->error = QB3E_LIBERR; return 0; }
        img_dev = p->d_q.p;
        g.stride = (uint64_t)g.w * g.bands;
    }
    const bool carry = !narrow && p->quanta < 2;
    const size_t maxsz = max_encoded_size_ref(p);         // the reference's bound: RLE0 decisions must not depend on the table
    uint8_t *out_dev = (uint8_t *)d_dst;
    if (on_host) {
        if (!p->d_out.ensure(maxsz + ixroom + 64)) { p->error = QB3E_LIBERR; return 0; }
        out_dev = (uint8_t *)p->d_out.p;
    }
    // check_info (reference QB3encode.h:364-373); cband is kept in range by the setter
    if (g.w < 4 || g.h < 4) { p->error = 1; return 0; }

    // optional restart table inside the container (a winning RLE0 pass keeps it in front of its bytes)
    IxTable ixt;
    size_t hdr_stamp = hdr;                               // header bytes prepared on the host
    if (ixroom && !narrow) {
        ixt = ix_layout(g, p->ix_chunk);
        hdr_stamp = write_headers(p, hdrbuf, false);
        hdr = hdr_stamp + ix_total_bytes(ixt) + 2;        // chunks, then "DT": both written by enc_finish_kernel
        ixt.base = out_dev + hdr_stamp;
        if (!d_index) {                                   // the table is a sample of the index: make one
            if (!p->d_idx.ensure(index_bytes(g))) { p->error = QB3E_LIBERR; return 0; }
            d_index = p->d_idx.p;
            ixt.own_index = true;
        }
    }
    uint64_t bits = 0;
    int has_run = 1;        // (RLE0 modes: the concatenation pass counts zero runs and pairs of 0xff; rle0_may_win, qb3_dev.h)
    bool piped = false;
    if (want_pipe) {
        const int r = encode_pipelined(p, g, host_src, host_dst, src_span, line, out_dev, hdr, hdrbuf, hdr_stamp, ixt, d_index, carry, &bits);
        if (r < 0) return 0;
        piped = r > 0;
        if (!piped && !upload_now()) { p->error = QB3E_LIBERR; return 0; }
    }
    if (!piped && !encode_blocks_device(p, g, img_dev, out_dev, hdr, d_index, st, carry, &bits, hdrbuf, hdr_stamp, ixt, rle ? &has_run : nullptr)) {   // the index describes the block stream, RLE0 wrapped or not
        p->error = QB3E_LIBERR; return 0;
    }
    p->error = 0;
    const size_t len = hdr + (size_t)((bits + 7) / 8);
    const size_t len_ref = len - (ixt.base ? ix_total_bytes(ixt) : 0);      // what the reference's container measures

    if (rle) {
        // the RLE0 post pass (reference QB3encode.cpp:536-565)
        p->mode = mode;
        // ... which can only win when the stream's zero runs outweigh its pairs of 0xff (has_run: the encoder kernels counted)
        if (len_ref <= maxsz / 2 && has_run) {
            // the byte pass on the device (k_rle0.hip): its size first, the bytes only when it wins -- into a buffer of its
            // own (the passes run in parallel: not in place), then behind the RLE mode's header
            const size_t n = len - hdr;
            uint64_t rsz64 = 0;
            if (!p->d_rle.ensure(rle0_ws_bytes(n)) || rle0_device_size(out_dev + hdr, n, p->d_rle.p, false, &rsz64, st, has_run == 2)) { p->error = QB3E_LIBERR; return 0; }
            const size_t rsz = (size_t)rsz64;
            if (rsz <= maxsz - len_ref && rsz < n) {
                // the RLE mode's header, the restart table when one was asked for (its chunks and the "DT" behind them stand in the
                // buffer as written: the table describes the block stream, which the decoder sees again once it has expanded the
                // bytes), then the RLE0 bytes
                uint8_t hdr2[80];
                const size_t tbl = ixt.base ? hdr - hdr_stamp : 0;      // (chunks + "DT")
                const size_t h2 = write_headers(p, hdr2, tbl == 0);
                if (!p->d_q.ensure(rsz) || rle0_device_write(out_dev + hdr, n, p->d_rle.p, false, p->d_q.p, st)) { p->error = QB3E_LIBERR; return 0; }
                if (on_host) {
                    memcpy(host_dst, hdr2, h2);
                    if (tbl && !download(p->stager, (uint8_t *)host_dst + h2, out_dev + hdr_stamp, tbl, st)) { p->error = QB3E_LIBERR; return 0; }
                    if (!download(p->stager, (uint8_t *)host_dst + h2 + tbl, p->d_q.p, rsz, st)) { p->error = QB3E_LIBERR; return 0; }
                } else {
                    // (device flavour: out_dev IS d_dst and h2 == hdr_stamp -- the modes' headers differ in one byte -- so the table stays where it is)
                    if (tbl && h2 != hdr_stamp) HIPOK(hipMemcpyAsync((uint8_t *)d_dst + h2, out_dev + hdr_stamp, tbl, hipMemcpyDeviceToDevice, st));
                    HIPOK(hipMemcpyAsync((uint8_t *)d_dst + h2 + tbl, p->d_q.p, rsz, hipMemcpyDeviceToDevice, st));
                    HIPOK(hipMemcpyAsync(d_dst, hdr2, h2, hipMemcpyHostToDevice, st));
                    HIPOK(hipStreamSynchronize(st));
                }
                return h2 + tbl + rsz;
            }
        }
    }
    // (the restart table does not take part in the decision: the same inputs give the same kind of container)
    if (raw_size(p) > len_ref) {
        if (on_host) {
            memcpy(host_dst, hdrbuf, hdr_stamp);
            if (!piped && !download(p->stager, (uint8_t *)host_dst + hdr_stamp, out_dev + hdr_stamp, len - hdr_stamp, st)) { p->error = QB3E_LIBERR; return 0; }
        }       // device flavour: the header was written by enc_finish_kernel, in stream order
        return len;
    }
    // not worth it: raw bypass (reference QB3encode.cpp:571-573), which leaves the handle's mode at STORED
    guard.armed = false;
    if (on_host) return stored_encode_host(p, host_src, host_dst);
    p->mode = QB3M_STORED;
    const size_t h2 = write_headers(p, hdrbuf);
    HIPOK(hipMemcpyAsync(d_dst, hdrbuf, h2, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpy2DAsync((uint8_t *)d_dst + h2, line, d_src, src_stride_bytes, line, p->ysize, hipMemcpyDeviceToDevice, st));
    HIPOK(hipStreamSynchronize(st));
    return h2 + raw_size(p);
}

QB3_API size_t qb3_encode(encsp p, void *source, void *destination) {
    if (!p || !source || !destination) return 0;
    return abi_guard<size_t>(0, [&] { return encode_common(p, source, destination, nullptr, nullptr, nullptr, nullptr); });
}

QB3_API size_t qb3x_encode_device(encsp p, const void *d_src, void *d_dst, void *d_index, void *stream) {
    if (!p || !d_src || !d_dst || ((uintptr_t)d_dst & 3)) { if (p) p->error = QB3E_EINV; return 0; }
    return abi_guard<size_t>(0, [&] { return encode_common(p, nullptr, nullptr, d_src, d_dst, d_index, (hipStream_t)stream); });
}

QB3_API void qb3x_set_encoder_index_chunk(encsp p, int on) { if (p) p->ix_chunk = on >= 2 ? 2 : on != 0; }

QB3_API size_t qb3x_index_size(const encsp p) {
    if (!p || p->xsize < 4 || p->ysize < 4) return 0;
    Geometry g = make_geometry(p->xsize, p->ysize, p->nbands, p->type, p->stride, p->order, p->mode, p->cband, nullptr);
    return index_bytes(g);
}

// ---------------------------------------------------------------- decoder handle
QB3_API void qb3_destroy_decoder(decsp p) {
    if (!p) return;
    release_all({&p->d_in, &p->d_img, &p->d_ws, &p->d_ix, &p->d_rle, &p->d_tab, &p->d_win, &p->d_wst, &p->d_wout, &p->d_wsrc, &p->d_wdesc, &p->d_rg, &p->d_wfull, &p->d_wgat, &p->d_mos});
    p->h_wdesc.release(); p->h_wst.release(); p->h_rg.release(); p->h_wgat.release();
    p->stager.release(); p->stager2.release(); p->pipe.release();
    delete p;
}
QB3_API void qb3_set_decoder_stride(decsp p, size_t stride) { p->stride = stride; }
QB3_API void qb3x_set_decoder_compat(decsp p, unsigned flags) { if (p) p->compat = flags; }
QB3_API void qb3x_set_decoder_window_kernels(decsp p, unsigned mask) { if (p) p->win_kernels = mask & (QB3X_WINK_U16 | QB3X_WINK_CF8 | QB3X_WINK_UNIT | QB3X_WINK_CFU); }

// A plain 8-bit stream (no index, no restart table) is walked through a table in device memory (qb3_dev.h): make sure
// the decoder holds one -- the whole call in one round, or walk_table_cap() and several rounds.  False: out of memory.
bool qb3api::walk_table_ready(decsp p, const Geometry &g, const DecPlan &plan, uint32_t ntiles, uint64_t max_bits) {
    if (!walk_table_applies(g, plan)) return true;
    size_t want = walk_memory_bytes(g, ntiles, max_bits);
    const size_t least = walk_table_min_bytes(ntiles, g.tsz);
    const size_t cap = walk_table_cap();
    if (want > cap) want = cap > least ? cap : least;
    return p->d_tab.cap >= want || p->d_tab.ensure(want);
}

// Decode the block stream at d_stream (+ byte offset off inside a 4-byte aligned device buffer) into d_img.
static bool decode_blocks_device(decsp p, const Geometry &g, const uint8_t *d_buf, size_t off, size_t nbytes,
                                 void *d_img, const void *d_index, hipStream_t st, const IxTable &ix = IxTable()) {
    DecPlan plan = plan_decode(g);
    if (!p->d_ws.ensure(plan.ws_bytes)) return false;
    uint32_t *d_status = nullptr;
    const uint32_t *in32 = (const uint32_t *)(d_buf + (off & ~(size_t)3));
    if (!d_index && !ix.base && !walk_table_ready(p, g, plan, 1, (uint64_t)nbytes * 8)) return false;
    uint32_t status = 0;
    IxTable table = ix;
    // (32/64-bit plain streams: the table of a band of sixteen rungs; a stream that leaves the band goes to the one-lane parser)
    bool walk_tab_ok = true, dropped_table = false;
    const uint32_t wide_band = 16;
    for (int turn = 0; turn < 3; turn++) {          // (the ladder of a tile batch: decode_tiles_body, api_tiles.cpp)
        for (int full = 0; full < 2; full++) {      // (second turn: a 16-bit segment outgrew the staging sized for the stream's average)
            if (launch_decode(g, plan, in32, (uint32_t)(8 * (off & 3)), (uint64_t)nbytes * 8, d_img, d_index, p->d_ws.p, &d_status, st, TileBatch(), nullptr, table,
                              walk_tab_ok ? p->d_tab.p : nullptr, walk_tab_ok ? p->d_tab.cap : 0, full != 0, wide_band))
                return false;
            const hipError_t e = fetch_small(&status, d_status, 4, st);
            if (e != hipSuccess) { set_error("decode kernels", (int)e); return false; }
            { static const bool dbg = getenv("QB3_DEBUG_DEC") != nullptr; if (dbg) fprintf(stderr, "decode turn %d full %d: status %u (table %d)\n", turn, full, status, table.base != nullptr); }
            if (!(status & 16)) break;
        }
        // The container's restart table is a convenience the format does not protect: when its check fails (bit 5) or the
        // decode that relied on it does, the stream is decoded again WITHOUT it -- the plain walk, what the reference does
        // with such a container -- so a damaged table costs time, never pixels.
        if (!(status & (27 | 32)) || d_index) break;
        if (table.base) {
            table = IxTable();
            dropped_table = true;
            if (!walk_table_ready(p, g, plan, 1, (uint64_t)nbytes * 8)) return false;
        } else if (walk_tab_ok && p->d_tab.p && walk_table_applies(g, plan)) walk_tab_ok = false;      // (the last rung of the ladder, for every width and mode: the one-lane
            // parser, whose reader behaves like the reference's on a stream that ends early -- zeros behind the end, bitstream.h:36 -- where the table walks stop)
        else break;
    }
    prof_collect();
    p->last_status = status | (dropped_table ? 32u : 0u);        // (bit 5: the container's table was not used in the end, whatever made it so)
    // bit 0: corrupt unit, bit 1: more than 7 unused bits at the end (reference QB3decode.h:411,569,740).
    // bit 2 (ran past the end) is not an error in the reference, whose reader clamps (bitstream.h:36).
    // bit 3: the index handed in does not describe this stream (a segment longer than any valid one).
    if (status & 27) { set_error("decode: corrupt or over-long stream", 0); p->error = QB3E_ERR; return false; }
    return true;
}


// ---------------------------------------------------------------- qb3_read_data, pipelined
// A self-indexed container (level 2 table: an entry per segment with its blocks' fields) decodes segment by segment with
// nothing but its table, so the call can be cut into STRIPS of block rows: while the stream of strip k + 1 goes up the link,
// strip k is decoded and the rows of strip k - 1 come down -- three streams, two rings of pinned slices, the host copies
// (caller's memory <-> pinned) by the pool of copy threads.  The link moves 48 GB/s each way at once (tools/pcie_probe.cpp),
// so the call is bound by its larger direction -- the raster -- instead of the sum of both.
// Returns the decoded size; 0 with p->error == QB3E_OK: not taken or not trusted (a table that fails its check, a segment
// that does not decode) -- the caller goes on with the one-after-the-other path, which has the fallback ladder;
// 0 with p->error set: a HIP failure.
static size_t decode_pipelined(decsp p, const Geometry &g, const IxTable &ix_host, void *host_dst, size_t nbytes, size_t total, size_t line) {
    using qb3host::CopyPool;
    constexpr size_t SLICE = Stager::SLICE, NSLOT = Stager::NSLOT;
    static const bool dbg = getenv("QB3_DEBUG_PIPE") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    const DecPlan plan = plan_decode(g);
    IxTable ixt = ix_host;
    const size_t tab_bytes = ix_total_bytes(ixt) + 2;
    if (!p->d_ix.ensure(tab_bytes + 16)) return 0;
    ixt.base = (uint8_t *)p->d_ix.p;
    if (!decode_strips_ok(g, plan, ixt)) return 0;
    // strips of block rows, about 48 MB of raster each, the last one at least two block rows (a shifted last row overlaps the one before)
    const uint32_t nby = g.nby, nbx = g.nbx, NB = g.seg_blocks;
    uint32_t BR = (uint32_t)std::max<size_t>(2, ((size_t)48 << 20) / (4 * line));
    uint32_t nstrips = (nby + BR - 1) / BR;
    if (nstrips > 1 && nby - (nstrips - 1) * BR < 2) nstrips--;
    if (nstrips < 3) return 0;
    if (!p->pipe.init() || !p->pipe.events(2 * (size_t)nstrips) || !p->stager.init() || !p->stager2.init()) return 0;
    if (!p->d_in.ensure(nbytes + 8) || !p->d_img.ensure(total) || !p->d_ws.ensure(plan.ws_bytes)) return 0;
    // where the stream must have arrived for a strip to be decoded: the position of the segment behind its last one, from
    // the table in the caller's memory (untrusted: not monotonous or behind the stream's end means "not this way")
    const uint8_t *tab_host = p->s_start + p->ix_off;
    auto entry_pos = [&](uint64_t k) -> uint64_t {
        const uint64_t c = k / ixt.per_chunk, j = k - c * ixt.per_chunk;
        const uint8_t *e = tab_host + c * (IX_HEAD + (ixt.pads ? IX_PAD : 0) + (uint64_t)ixt.per_chunk * ixt.entry_bytes) + IX_HEAD + j * ixt.entry_bytes;
        uint64_t v = 0;
        for (int i = 0; i < 6; i++) v |= (uint64_t)e[i] << (8 * i);
        return v;
    };
    struct Strip { uint64_t seg0, nseg; size_t need, row0, row1; };
    std::vector<Strip> strips(nstrips);
    size_t prev_need = 0;
    for (uint32_t s = 0; s < nstrips; s++) {
        const uint32_t br0 = s * BR, br1 = s + 1 == nstrips ? nby : (s + 1) * BR;
        const uint64_t b0 = (uint64_t)br0 * nbx, b1 = (uint64_t)br1 * nbx;
        Strip &t = strips[s];
        t.seg0 = b0 / NB;
        const uint64_t seg1 = std::min<uint64_t>(g.nseg, (b1 + NB - 1) / NB);
        t.nseg = seg1 - t.seg0;
        const uint64_t pos = seg1 < g.nseg ? entry_pos(seg1) : (uint64_t)nbytes * 8;
        if (pos > (uint64_t)nbytes * 8) return 0;
        t.need = std::min(nbytes, (size_t)(pos / 8) + 16);
        if (t.need < prev_need) return 0;
        prev_need = t.need;
        t.row0 = (size_t)4 * br0; t.row1 = s + 1 == nstrips ? g.h : (size_t)4 * br1;
    }
    strips[nstrips - 1].need = nbytes;
    // the slices: up = the table, then the stream; down = every strip's rows
    struct Slice { uint8_t *dev; uint8_t *host; size_t n; uint32_t strip; };
    std::vector<Slice> up, dn;
    for (size_t off = 0; off < tab_bytes; off += SLICE) up.push_back({(uint8_t *)p->d_ix.p + off, const_cast<uint8_t *>(tab_host) + off, std::min(SLICE, tab_bytes - off), 0});
    const size_t n_tab = up.size();
    for (size_t off = 0; off < nbytes; off += SLICE) up.push_back({(uint8_t *)p->d_in.p + off, p->s_in + off, std::min(SLICE, nbytes - off), 0});
    for (uint32_t s = 0; s < nstrips; s++) {
        const size_t a = strips[s].row0 * line, b = strips[s].row1 * line;
        for (size_t off = a; off < b; off += SLICE) dn.push_back({(uint8_t *)p->d_img.p + off, (uint8_t *)host_dst + off, std::min(SLICE, b - off), s});
    }
    CopyPool &pool = CopyPool::get();
    CopyPool::Batch b_up[NSLOT], b_dn[NSLOT];
    Stager &r1 = p->stager, &r2 = p->stager2;
    hipStream_t sU = p->pipe.up, sK = p->pipe.k, sD = p->pipe.dn;
    const double t_setup = ms_since();
    double t_up_done = 0, t_first_dn = 0;
    size_t up_started = 0, up_enq = 0, stream_enq = 0, dn_avail = 0, dn_issued = 0, dn_copy = 0, dn_freed = 0;
    uint32_t next_strip = 0;
    int last_strip_waited = -1;
    uint32_t *d_status = nullptr;
    hipError_t e = hipSuccess;
    bool launch_failed = false;
    auto ok = [&] { return e == hipSuccess && !launch_failed; };
    while (ok() && (up_enq < up.size() || dn_freed < dn.size())) {
        bool progress = false;
        // ---- up: the host copy of a slice into its pinned slot (two in flight), then its DMA
        if (up_started < up.size() && up_started - up_enq < 2 && (up_started < NSLOT || hipEventQuery(r1.ev(up_started)) == hipSuccess)) {
            pool.submit(r1.slot(up_started), up[up_started].host, up[up_started].n, b_up[up_started % NSLOT]);
            up_started++; progress = true;
        }
        if (up_enq < up_started && pool.done(b_up[up_enq % NSLOT])) {
            e = hipMemcpyAsync(up[up_enq].dev, r1.slot(up_enq), up[up_enq].n, hipMemcpyHostToDevice, sU);
            if (e == hipSuccess) e = hipEventRecord(r1.ev(up_enq), sU);
            if (up_enq >= n_tab) stream_enq += up[up_enq].n;
            up_enq++; progress = true;
            if (dbg && up_enq == up.size()) t_up_done = ms_since();
            // strips whose stream is on its way: their kernel waits for it on the kernel stream
            while (ok() && up_enq >= n_tab && next_strip < nstrips && strips[next_strip].need <= stream_enq) {
                hipEvent_t ev_u = p->pipe.ev[2 * next_strip], ev_k = p->pipe.ev[2 * next_strip + 1];
                e = hipEventRecord(ev_u, sU);
                if (e == hipSuccess) e = hipStreamWaitEvent(sK, ev_u, 0);
                if (e != hipSuccess) break;
                const DecStrip st = { strips[next_strip].seg0, strips[next_strip].nseg, next_strip == 0 };
                if (launch_decode(g, plan, (const uint32_t *)p->d_in.p, 0, (uint64_t)nbytes * 8, p->d_img.p, nullptr, p->d_ws.p, &d_status, sK, TileBatch(), nullptr, ixt,
                                  nullptr, 0, false, 16, &st)) { launch_failed = true; break; }
                e = hipEventRecord(ev_k, sK);
                while (dn_avail < dn.size() && dn[dn_avail].strip == next_strip) dn_avail++;
                next_strip++;
            }
        }
        // ---- down: the DMA of a slice into its pinned slot once its strip's kernel is done, then the host copy out of it
        if (ok() && dn_issued < dn_avail && dn_issued - dn_freed < NSLOT) {
            if ((int)dn[dn_issued].strip != last_strip_waited) {
                e = hipStreamWaitEvent(sD, p->pipe.ev[2 * dn[dn_issued].strip + 1], 0);
                last_strip_waited = (int)dn[dn_issued].strip;
            }
            if (e == hipSuccess) e = hipMemcpyAsync(r2.slot(dn_issued), dn[dn_issued].dev, dn[dn_issued].n, hipMemcpyDeviceToHost, sD);
            if (e == hipSuccess) e = hipEventRecord(r2.ev(dn_issued), sD);
            dn_issued++; progress = true;
        }
        if (ok() && dn_copy < dn_issued) {
            const hipError_t q = hipEventQuery(r2.ev(dn_copy));
            if (q == hipSuccess) { if (dbg && !dn_copy) t_first_dn = ms_since(); pool.submit(dn[dn_copy].host, r2.slot(dn_copy), dn[dn_copy].n, b_dn[dn_copy % NSLOT]); dn_copy++; progress = true; }
            else if (q != hipErrorNotReady) e = q;
        }
        while (dn_freed < dn_copy && pool.done(b_dn[dn_freed % NSLOT])) { dn_freed++; progress = true; }
        if (!progress && !pool.help_one()) std::this_thread::yield();
    }
    (void)hipGetLastError();                                // (hipErrorNotReady of the queries is not an error)
    for (size_t i = 0; i < NSLOT; i++) { pool.wait(b_up[i]); pool.wait(b_dn[i]); }
    p->pipe.sync();
    if (dbg) fprintf(stderr, "decode_pipelined: setup %.2f ms, last upload enqueued %.2f, first slice down %.2f, done %.2f (%u strips, %zu + %zu slices)\n", t_setup, t_up_done, t_first_dn, ms_since(), nstrips, up.size(), dn.size());
    if (!ok()) { if (!launch_failed) set_error("pipelined decode", (int)e); p->error = QB3E_LIBERR; return 0; }
    uint32_t status = 0;
    e = hipMemcpy(&status, d_status, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_error("pipelined decode: status", (int)e); p->error = QB3E_LIBERR; return 0; }
    prof_collect();
    p->last_status = status;
    if (status) return 0;                                   // not trusted: the caller decodes again, one step after the other
    return total;
}

size_t qb3api::decode_common(decsp p, void *host_dst, const void *d_src, void *d_dst, const void *d_index, hipStream_t st) {
    if (p->stage != 2 || p->error != QB3E_OK || p->s_in == nullptr || p->s_size == 0) {
        if (p->error == QB3E_OK) p->error = QB3E_EINV;
        return 0;
    }
    const bool on_host = host_dst != nullptr;
    const size_t tsz = szof(p->type), line = p->xsize * p->nbands * tsz, total = qb3_decoded_size(p);
    const size_t data_off = (size_t)(p->s_in - p->s_start);
    const size_t dst_stride = (p->stride ? p->stride : p->xsize * p->nbands) * tsz;
    // qb3x_read_start / qb3x_read_start_device handles hold a copy of the container's HEAD (hdr_avail bytes at s_start) while
    // s_size spans the whole container: the host-pointer call would read the stream, and the table, past that copy
    if (on_host && p->hdr_avail < data_off + p->s_size) { p->error = QB3E_EINV; return 0; }
    if (p->mode == QB3M_STORED) {           // reference QB3decode.cpp:356-375
        if (p->s_size != total) { p->error = QB3E_EINV; return 0; }
        if (on_host) {
            if (!p->stride) memcpy(host_dst, p->s_in, total);
            else for (size_t y = 0; y < p->ysize; y++) memcpy((uint8_t *)host_dst + y * dst_stride, p->s_in + y * line, line);   // stride in values, as everywhere (QB3.h:146-148)
        } else {
            HIPOK(hipMemcpy2DAsync(d_dst, dst_stride, (const uint8_t *)d_src + data_off, line, line, p->ysize, hipMemcpyDeviceToDevice, st));
            HIPOK(hipStreamSynchronize(st));
        }
        return total;
    }
    if (p->xsize * p->ysize < 16) { p->error = QB3E_EINV; return 0; }
    if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }

    // a large self-indexed container in host memory: upload, decode and download strip by strip, all three at once
    static const bool no_pipeline = [] { const char *e = getenv("QB3_NO_PIPELINE"); return e && e[0] && e[0] != '0'; }();
    if (on_host && !is_rle_mode(p->mode) && p->ix_K && p->ix_bl && p->quanta <= 1 && p->xsize >= 4 && p->ysize >= 4 && dst_stride == line &&
        total >= ((size_t)64 << 20) && !no_pipeline) {
        const size_t r = decode_pipelined(p, decoder_geometry(p, p->xsize, p->ysize, 0), handle_table(p, nullptr), host_dst, p->s_size, total, line);
        if (r) return r;
        if (p->error != QB3E_OK) return 0;
    }
    // locate the block stream on the device
    const uint8_t *dev_buf = nullptr;
    size_t off = 0, nbytes = p->s_size;
    const bool rle = is_rle_mode(p->mode);
    if (rle) {
        // the RLE0 expansion on the device (k_rle0.hip; reference QB3decode.cpp:396-413): size first, then the bytes
        const uint8_t *packed = (const uint8_t *)d_src + data_off;
        const size_t wsb = (rle0_ws_bytes(p->s_size) + 15) & ~(size_t)15;
        if (!p->d_rle.ensure(wsb + (on_host ? p->s_size : 0))) { p->error = QB3E_LIBERR; return 0; }
        if (on_host) {
            uint8_t *up = (uint8_t *)p->d_rle.p + wsb;
            if (!upload(p->stager, up, p->s_in, p->s_size, st)) { p->error = QB3E_LIBERR; return 0; }
            packed = up;
        }
        uint64_t sz = 0;
        if (rle0_device_size(packed, p->s_size, p->d_rle.p, true, &sz, st)) { p->error = QB3E_LIBERR; return 0; }
        if (sz > total) { p->error = QB3E_ERR; return 0; }
        if (!p->d_in.ensure((size_t)sz + 8)) { p->error = QB3E_LIBERR; return 0; }
        if (rle0_device_write(packed, p->s_size, p->d_rle.p, true, p->d_in.p, st)) { p->error = QB3E_LIBERR; return 0; }
        HIPOK(hipMemsetAsync((uint8_t *)p->d_in.p + sz, 0, 8, st));       // (a stream that ends early reads as zeros behind its end, not as what the buffer held before)
        nbytes = (size_t)sz;
        dev_buf = (const uint8_t *)p->d_in.p; off = 0;
    } else if (on_host) {
        if (!p->d_in.ensure(nbytes + 8)) { p->error = QB3E_LIBERR; return 0; }
        if (!upload(p->stager, p->d_in.p, p->s_in, nbytes, st)) { p->error = QB3E_LIBERR; return 0; }
        HIPOK(hipMemsetAsync((uint8_t *)p->d_in.p + nbytes, 0, 8, st));    // (a stream that ends early reads as zeros behind its end, not as what the buffer held before)
        dev_buf = (const uint8_t *)p->d_in.p; off = 0;
    } else { dev_buf = (const uint8_t *)d_src; off = data_off; }

    // geometry, narrow images decode into their stand-in shape (reference QB3decode.cpp:321-353)
    size_t w = p->xsize, h = p->ysize;
    const bool narrow = w < 4 || h < 4;
    if (narrow) {
        const size_t ngroups = (w * h + 15) / 16;
        if (p->xsize < 4) { w = 4; h = ngroups * 4; } else { w = ngroups * 4; h = 4; }
    }
    const bool direct = !on_host && !narrow;        // decode straight into the caller's device buffer
    const Geometry g = decoder_geometry(p, w, h, direct ? p->stride : 0);
    void *img_dev = d_dst;
    if (!direct) {
        if (!p->d_img.ensure((size_t)g.w * g.h * g.bands * tsz)) { p->error = QB3E_LIBERR; return 0; }
        img_dev = p->d_img.p;
    }
    // a restart table inside the container stands in for a missing index (also under RLE0: the table describes the block stream,
    // which is what the expansion above has just made)
    IxTable ixt;
    if (!d_index && p->ix_K && !narrow) {
        if (on_host) {
            const size_t bytes = ix_total_bytes(handle_table(p, nullptr)) + 2;      // (+2: the "DT" behind the last chunk, which the check kernel looks at)
            if (!p->d_ix.ensure(bytes + 16)) { p->error = QB3E_LIBERR; return 0; }       // (+16: the check kernel reads whole sixteen-byte groups)
            HIPOK(hipMemcpyAsync(p->d_ix.p, p->s_start + p->ix_off, bytes, hipMemcpyHostToDevice, st));
        }
        ixt = handle_table(p, on_host ? (const uint8_t *)p->d_ix.p : (const uint8_t *)d_src + p->ix_off);
    }
    if (!decode_blocks_device(p, g, dev_buf, off, nbytes, img_dev, d_index, st, ixt)) {
        if (p->error == QB3E_OK) p->error = QB3E_LIBERR;
        return 0;
    }
    if (p->quanta > 1 && launch_dequantize(img_dev, g, (int)p->type, p->quanta, st)) { p->error = QB3E_LIBERR; return 0; }

    if (narrow) {
        std::vector<uint8_t> t((size_t)g.w * g.h * g.bands * tsz);
        HIPOK(hipMemcpyAsync(t.data(), img_dev, t.size(), hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        std::vector<uint8_t> outimg;
        uint8_t *dst = (uint8_t *)host_dst;
        if (!on_host) { outimg.resize(dst_stride * p->ysize); dst = outimg.data(); }
        const size_t pix = p->nbands * tsz;
        const uint8_t *s = t.data();
        if (p->xsize < 4) for (size_t y = 0; y < p->ysize; y++, s += p->xsize * pix) memcpy(dst + y * dst_stride, s, p->xsize * pix);
        else for (size_t x = 0; x < p->xsize; x++) for (size_t y = 0; y < p->ysize; y++, s += pix) memcpy(dst + y * dst_stride + x * pix, s, pix);
        // (row by row: the gaps of a wide stride are not the image's -- in a mosaic they are the neighbouring tiles)
        if (!on_host) { HIPOK(hipMemcpy2DAsync(d_dst, dst_stride, dst, dst_stride, p->xsize * pix, p->ysize, hipMemcpyHostToDevice, st)); HIPOK(hipStreamSynchronize(st)); }
        return total;
    }
    if (on_host) {
        if (dst_stride == line) { if (!download(p->stager, host_dst, img_dev, total, st)) { p->error = QB3E_LIBERR; return 0; } }
        else {
            HIPOK(hipMemcpy2DAsync(host_dst, dst_stride, img_dev, line, line, p->ysize, hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
        }
    }
    return total;
}

QB3_API size_t qb3_read_data(decsp p, void *dst) {
    if (!p || !dst) return 0;
    return abi_guard<size_t>(0, [&] { return decode_common(p, dst, nullptr, nullptr, nullptr, nullptr); });
}

QB3_API size_t qb3x_decode_device(decsp p, const void *d_src, void *d_dst, const void *d_index, void *stream) {
    if (!p || !d_src || !d_dst || ((uintptr_t)d_src & 3)) { if (p) p->error = QB3E_EINV; return 0; }
    return abi_guard<size_t>(0, [&] { return decode_common(p, nullptr, d_src, d_dst, d_index, (hipStream_t)stream); });
}

// ---------------------------------------------------------------- misc
QB3_API unsigned qb3x_last_decode_status(const decsp p) { return p ? p->last_status : 0u; }

QB3_API int qb3x_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
QB3_API const char *qb3x_last_error(void) { return last_error(); }
// FNV-1a, 64 bit, over host bytes; chain calls by passing the previous result as `seed` (0 starts a new hash)
QB3_API uint64_t qb3x_fnv1a64(const void *data, size_t n, uint64_t seed) {
    uint64_t h = seed ? seed : 0xcbf29ce484222325ull;
    const uint8_t *b = (const uint8_t *)data;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
// The RLE0 byte pass on device buffers (k_rle0.hip): the coded (decode = 0) or expanded (decode != 0) form of the n bytes
// at d_src.  d_dst == NULL: the size only.  Returns the size, 0 on failure or when it exceeds dst_cap.
QB3_API size_t qb3x_rle0_device(const void *d_src, size_t n, void *d_dst, size_t dst_cap, int decode, void *stream) {
    if (!d_src || !n) return 0;
    DevBuf ws;
    if (!ws.ensure(rle0_ws_bytes(n))) return 0;
    uint64_t total = 0;
    size_t ret = 0;
    if (rle0_device_size(d_src, n, ws.p, decode != 0, &total, stream) == 0) {
        if (!d_dst) ret = (size_t)total;
        else if (total <= dst_cap && rle0_device_write(d_src, n, ws.p, decode != 0, d_dst, stream) == 0 &&
                 hipStreamSynchronize((hipStream_t)stream) == hipSuccess) ret = (size_t)total;
    }
    ws.release();
    return ret;
}
QB3_API void qb3x_profile_enable(int level) { prof_enable(level < 0 ? 0 : level); }
QB3_API void qb3x_profile_reset(void) { prof_reset(); }
QB3_API int qb3x_profile_get(const char *kernel, double *total_ms, uint64_t *count) { return prof_get(kernel, total_ms, count) ? 1 : 0; }
QB3_API int qb3x_profile_names(char *buf, size_t bufsize) { return prof_names(buf, bufsize); }

QB3_API decsp qb3_create_decoder(void *source, size_t source_size, size_t *image_size) {
    decsp p = qb3_read_start(source, source_size, image_size);
    if (p && !qb3_read_info(p)) { qb3_destroy_decoder(p); p = nullptr; }
    return p;
}
QB3_API size_t qb3_decode(decsp p, void *destination) { return qb3_read_data(p, destination); }
