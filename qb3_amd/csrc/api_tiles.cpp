// qb3_amd/csrc/api_tiles.cpp -- tile batches of the C ABI: qb3x_encode_tiles and qb3x_decode_tiles, n equally shaped images or
// containers through one set of launches (blockIdx.y = tile), with the one-by-one path for whatever a batch does not take.  The work is
// done on GRIDS of tiles (TileGrid, qb3_host.h): the two calls here hand in one row of n tiles, the mosaic calls (api_mosaic.cpp) the
// tiles of a raster where they lie.
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

static const uint8_t *grid_img(const TileGrid &G, size_t u) { return (const uint8_t *)G.img + (u / G.cols) * G.img_row + (u % G.cols) * G.img_col; }
static size_t grid_k(const TileGrid &G, size_t u) { return G.k0 + (u / G.cols) * G.k_row + u % G.cols; }
// The tiles [first, first + count) of a grid that the next set of launches takes, at most `batch`: whole rows of the grid while a row
// fits (*cols: the grid's), else a run of one row (*cols = 0)
static size_t grid_piece(const TileGrid &G, size_t first, size_t batch, uint32_t *cols) {
    const size_t c = first % G.cols;
    if (c == 0 && batch >= G.cols) {
        *cols = (uint32_t)G.cols;
        return std::min(batch / G.cols, (G.n - first) / G.cols) * G.cols;
    }
    *cols = 0;
    return std::min(batch, G.cols - c);
}
// the handle's stride setting, set aside while a call works on grids that bring their own
template <class H> struct StrideGuard {
    H *p; size_t saved;
    explicit StrideGuard(H *h) : p(h), saved(h->stride) {}
    ~StrideGuard() { p->stride = saved; }
};

// One tile at a time (general path: RLE modes, quantisation, narrow or tiny tiles, STORED fallbacks)
static size_t encode_tiles_loop(encsp p, const TileGrid &G, size_t first, size_t n, void *d_dst, size_t dst_pitch,
                                void *d_index, size_t isz, size_t *sizes, void *stream, qb3_mode mode) {
    size_t done = 0;
    for (size_t u = first; u < first + n; u++) {
        const size_t k = grid_k(G, u);
        qb3_reset_encoder(p);
        p->mode = mode;
        sizes[k] = qb3x_encode_device(p, grid_img(G, u), (uint8_t *)d_dst + k * dst_pitch,
                                      d_index ? (uint8_t *)d_index + k * isz : nullptr, stream);
        done += sizes[k] != 0;
    }
    return done;
}

size_t qb3api::encode_tile_grids(encsp p, const TileGrid *grids, size_t ngrids, void *d_dst, size_t dst_pitch,
                                 void *d_index, size_t *sizes, void *stream) {
    const size_t isz = d_index ? qb3x_index_size(p) : 0;
    const qb3_mode mode = p->mode;
    const size_t tsz = szof(p->type);
    hipStream_t st = (hipStream_t)stream;
    StrideGuard<encs> keep(p);
    size_t nmax = 0;
    for (size_t gi = 0; gi < ngrids; gi++) nmax = std::max(nmax, grids[gi].n);
    // batched path: every tile of a grid goes through ONE set of kernel launches (blockIdx.y = tile) and one
    // host synchronisation.  Anything unusual takes the one-by-one path.
    const bool batchable = !is_rle_mode(mode) && mode != QB3M_STORED && p->quanta < 2 && p->xsize >= 4 && p->ysize >= 4 &&
                           p->xsize * p->ysize > 16 && !p->error && device_ok();
    if (!batchable) {
        size_t k = 0;
        for (size_t gi = 0; gi < ngrids; gi++) {
            p->stride = grids[gi].stride;
            k += encode_tiles_loop(p, grids[gi], 0, grids[gi].n, d_dst, dst_pitch, d_index, isz, sizes, stream, mode);
        }
        if (mode != QB3M_STORED) p->mode = mode;
        return k;
    }

    uint8_t hdrbuf[80];
    size_t hdr = write_headers(p, hdrbuf);
    Geometry g = make_geometry(p->xsize, p->ysize, p->nbands, p->type, 0, p->order, p->mode, p->cband, nullptr);
    uintptr_t low = 0;                      // a tile of any grid off the alignment of its values: the plan of the kernels that read it
    for (size_t gi = 0; gi < ngrids; gi++) low |= (uintptr_t)grids[gi].img | grids[gi].img_col | grids[gi].img_row;
    EncPlan plan = plan_encode(g, value_aligned_memory(g.tsz, low));      // (no function of the stride: one plan for every grid)
    size_t wsp = (plan.ws_bytes + 255) & ~(size_t)255;
    size_t batch = (size_t)8 << 30 >= wsp ? ((size_t)8 << 30) / wsp : 1;     // keep the workspace under 8 GiB
    if (batch > nmax) batch = nmax;
    if (batch > 65535) batch = 65535;
    if (!p->d_ws.ensure(batch * wsp)) { p->error = QB3E_LIBERR; return 0; }
    // self-indexing containers (qb3x_set_encoder_index_chunk): every tile gets its own restart table, at the same place
    IxTable ixt;
    size_t hdr_stamp = hdr, ix_bytes = 0, isz_all = isz;
    void *index_all = d_index;
    if (ix_room(p)) {                                     // (batchable: the mode is not QB3M_STORED)
        ixt = ix_layout(g, p->ix_chunk);
        hdr_stamp = write_headers(p, hdrbuf, false);
        ix_bytes = ix_total_bytes(ixt);
        hdr = hdr_stamp + ix_bytes + 2;                   // chunks, then "DT": both written by enc_finish_kernel
        if (!index_all) {                                 // the table is a sample of the index: make one per tile of a batch
            isz_all = (index_bytes(g) + 7) & ~(size_t)7;
            if (!p->d_idx.ensure(batch * isz_all)) { p->error = QB3E_LIBERR; return 0; }
            index_all = p->d_idx.p;
            ixt.own_index = true;
        }
    }
    BandState bs;
    memset(&bs, 0, sizeof(bs));             // tiles are independent streams: every tile starts from the reset state
    std::vector<EncResult> res(batch);
    size_t done = 0;
    for (size_t gi = 0; gi < ngrids; gi++) {
        const TileGrid &G = grids[gi];
        p->stride = G.stride;
        g.stride = G.stride ? G.stride : p->xsize * p->nbands;
        for (size_t first = 0, cnt; first < G.n; first += cnt) {
            TileBatch tb;
            cnt = grid_piece(G, first, batch, &tb.cols);
            const size_t k0 = grid_k(G, first);
            tb.n = (uint32_t)cnt; tb.src_pitch = G.img_col; tb.src_row = G.img_row; tb.dst_pitch = dst_pitch; tb.dst_row = G.k_row * dst_pitch; tb.ws_pitch = wsp;
            // (the caller's index array is indexed by container; the internal one by tile of the launch)
            tb.idx_pitch = isz_all; tb.idx_row = d_index ? G.k_row * isz : tb.cols * isz_all;
            uint8_t *out0 = (uint8_t *)d_dst + k0 * dst_pitch;
            if (ix_bytes) ixt.base = out0 + hdr_stamp;
            EncJob job;
            job.img = grid_img(G, first); job.out32 = (uint32_t *)(out0 + (hdr & ~(size_t)3)); job.out_bit0 = (uint32_t)(8 * (hdr & 3));
            job.st = bs; job.ws = p->d_ws.p; job.tb = tb;
            job.index = !index_all ? nullptr : (d_index ? (uint8_t *)d_index + k0 * isz : (uint8_t *)index_all);
            job.hdr = hdrbuf; job.hdr_len = (uint32_t)hdr_stamp; job.ix = ixt;
            if (launch_encode(g, plan, job, st)) { p->error = QB3E_LIBERR; return done; }
            const uint8_t *dres = (const uint8_t *)p->d_ws.p + plan.ws_bytes - sizeof(EncResult);
            hipError_t e = hipMemcpy2DAsync(res.data(), sizeof(EncResult), dres, wsp, sizeof(EncResult), cnt, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { set_error("encode kernels (tiles)", (int)e); p->error = QB3E_LIBERR; return done; }
            prof_collect();
            const size_t raw = p->xsize * p->ysize * p->nbands * tsz;
            for (size_t i = 0; i < cnt; i++) {
                const size_t len = hdr + (size_t)((res[i].total_bits + 7) / 8);
                if (raw > len - ix_bytes) { sizes[grid_k(G, first + i)] = len; done++; }         // (the table does not take part in the decision)
                else done += encode_tiles_loop(p, G, first + i, 1, d_dst, dst_pitch, d_index, isz, sizes, stream, mode);   // STORED fallback
            }
            // handle state as after a loop over the tiles: the state left by the last one
            for (size_t c = 0; c < p->nbands; c++) {
                p->band[c].prev = (size_t)res[cnt - 1].prev[c]; p->band[c].runbits = res[cnt - 1].rung[c]; p->band[c].cf = (size_t)res[cnt - 1].cf[c];
            }
        }
    }
    p->mode = mode;         // a raw fallback of one tile must not turn the handle (and the next call) to QB3M_STORED
    p->error = 0;
    return done;
}

QB3_API size_t qb3x_encode_tiles(encsp p, const void *d_src, size_t n, size_t src_pitch, void *d_dst, size_t dst_pitch,
                                 void *d_index, size_t *sizes, void *stream) {
    return abi_guard<size_t>(0, [&]() -> size_t {
        if (!p || !d_src || !d_dst || !sizes || (dst_pitch & 3) || ((uintptr_t)d_dst & 3)) return 0;
        const TileGrid row = { n, n ? n : 1, d_src, src_pitch, 0, p->stride, 0, 0 };
        return encode_tile_grids(p, &row, 1, d_dst, dst_pitch, d_index, sizes, stream);
    });
}

// One tile through its own header: a host copy of its head is parsed into a handle of its own (a batch may hold
// containers of another kind than tile 0's: raw-stored tiles next to coded ones, QB3encode.cpp:571-573)
static bool decode_tile_alone(decsp ref, const uint8_t *d_tile, size_t size, void *d_out, size_t stride, const void *d_index, hipStream_t st) {
    size_t dims[3];
    decsp q = qb3x_read_start_device(d_tile, size, dims, st);
    if (!q) return false;
    bool ok = dims[0] == ref->xsize && dims[1] == ref->ysize && dims[2] == ref->nbands && q->type == ref->type;
    if (ok) {
        q->stride = stride; q->compat = ref->compat;
        ok = 0 != qb3x_decode_device(q, d_tile, d_out, d_index, st);
    }
    qb3_destroy_decoder(q);
    return ok;
}

size_t qb3api::decode_tile_grids(decsp p, const void *d_src, size_t n, size_t src_pitch, const size_t *sizes,
                                 const TileGrid *grids, size_t ngrids, const void *d_index, void *stream) {
    if (p->stage != 2 || p->error != QB3E_OK) return 0;
    const size_t hdr = (size_t)(p->s_in - p->s_start);
    hipStream_t st = (hipStream_t)stream;
    p->tile_ok.assign(n, 0);
    p->last_status = 0;
    if (!n || !device_ok()) return 0;
    // the mode byte of every tile: tiles of tile 0's kind go through one set of launches, the others one by one
    std::vector<uint8_t> modes(n);
    {
        hipError_t e = hipMemcpy2DAsync(modes.data(), 1, (const uint8_t *)d_src + 10, src_pitch, 1, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { set_error("decode tiles: mode bytes", (int)e); p->error = QB3E_LIBERR; return 0; }
    }
    // the pitch of the caller's index array is the encoder's qb3x_index_size: a function of the image and of the coding
    // mode, which a raw-stored tile 0 does not tell -- take it from the first coded tile
    size_t isz = 0;
    if (d_index && p->xsize >= 4 && p->ysize >= 4) {
        int m = p->mode;
        for (size_t i = 0; i < n && m == QB3M_STORED; i++) m = modes[i];
        if (m != QB3M_STORED && m < (int)QB3M_END)
            isz = index_bytes(make_geometry(p->xsize, p->ysize, p->nbands, p->type, 0, m <= (int)QB3M_CF_RLE ? ZCURVE : p->order, m, nullptr, p->cband));
    }
    const bool batchable = !is_rle_mode(p->mode) && p->mode != QB3M_STORED && p->quanta <= 1 && p->xsize >= 4 && p->ysize >= 4 &&
                           p->xsize * p->ysize >= 16;
    // restart tables (tile 0 has one, parsed by qb3_read_info): usable for the batch when every tile of it has its "ix" tag
    // and its "DT" mark where tile 0 has them (equally shaped tiles written by one encoder do); else the plain walk
    bool use_ix = !d_index && p->ix_K && hdr >= 2;
    std::vector<uint8_t> tags;
    if (use_ix) {
        tags.resize(4 * n);
        hipError_t e = hipMemcpy2DAsync(tags.data(), 4, (const uint8_t *)d_src + p->ix_off, src_pitch, 2, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpy2DAsync(tags.data() + 2, 4, (const uint8_t *)d_src + hdr - 2, src_pitch, 2, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { set_error("decode tiles: table tags", (int)e); p->error = QB3E_LIBERR; return 0; }
    }
    auto in_batch = [&](size_t i) { return batchable && modes[i] == (uint8_t)p->mode && sizes[i] > hdr; };
    for (size_t i = 0; i < n && use_ix; i++)
        if (in_batch(i) && !(tags[4 * i] == 'i' && tags[4 * i + 1] == 'x' && tags[4 * i + 2] == 'D' && tags[4 * i + 3] == 'T')) use_ix = false;
    size_t done = 0, nmax = 0;
    for (size_t gi = 0; gi < ngrids; gi++) nmax = std::max(nmax, grids[gi].n);
    for (size_t gi = 0; gi < ngrids && batchable; gi++) {
        const TileGrid &G = grids[gi];
        const Geometry g = decoder_geometry(p, p->xsize, p->ysize, G.stride);
        const DecPlan plan = plan_decode(g);
        const size_t wsp = (plan.ws_bytes + 255) & ~(size_t)255;
        size_t batch = d_index ? nmax : (((size_t)8 << 30) / wsp ? ((size_t)8 << 30) / wsp : 1);
        if (batch > nmax) batch = nmax;
        if (batch > 65535) batch = 65535;
        if (!p->d_ws.ensure(256 * ((batch + 63) / 64) + (d_index ? 0 : batch * wsp)) || !p->d_in.ensure(8 * batch)) { p->error = QB3E_LIBERR; return 0; }
        std::vector<uint64_t> bits(batch);
        std::vector<uint32_t> status(batch);
        for (size_t first = 0, cnt; first < G.n; first += cnt) {
            TileBatch tb;
            cnt = grid_piece(G, first, batch, &tb.cols);
            const size_t k0 = grid_k(G, first);
            auto kk = [&](size_t i) { return grid_k(G, first + i); };
            // a tile of another kind takes part with an empty stream: its lanes find nothing to read, its turn comes below
            for (size_t i = 0; i < cnt; i++) bits[i] = in_batch(kk(i)) ? (uint64_t)(sizes[kk(i)] - hdr) * 8 : 0;
            hipError_t e = hipMemcpyAsync(p->d_in.p, bits.data(), 8 * cnt, hipMemcpyHostToDevice, st);
            if (e != hipSuccess) { set_error("decode tiles: upload of stream lengths", (int)e); p->error = QB3E_LIBERR; return done; }
            tb.n = (uint32_t)cnt; tb.src_pitch = src_pitch; tb.src_row = G.k_row * src_pitch; tb.dst_pitch = G.img_col; tb.dst_row = G.img_row;
            tb.idx_pitch = isz; tb.idx_row = G.k_row * isz;
            for (size_t i = 0; i < cnt; i++) if (bits[i] > tb.max_bits) tb.max_bits = bits[i];
            const uint8_t *src0 = (const uint8_t *)d_src + k0 * src_pitch;
            IxTable ixt;
            if (use_ix) {
                ixt = handle_table(p, src0 + p->ix_off);
                ixt.check_heads = true;                     // (only tile 0's heads were read on the host)
            }
            if (!d_index && !use_ix && !walk_table_ready(p, g, plan, tb.n, tb.max_bits)) { p->error = QB3E_LIBERR; return done; }
            uint32_t *d_status = nullptr;
            bool walk_tab_ok = true;
            const uint32_t wide_band = 16;
            for (int turn = 0; turn < 3; turn++) {          // (the ladder of one stream: decode_blocks_device, qb3_api.cpp)
                for (int full = 0; full < 2; full++) {      // (second turn: a 16-bit segment outgrew the staging sized for the streams' average)
                    if (launch_decode(g, plan, (const uint32_t *)(src0 + (hdr & ~(size_t)3)), (uint32_t)(8 * (hdr & 3)), 0, const_cast<uint8_t *>(grid_img(G, first)),
                                      d_index ? (const uint8_t *)d_index + k0 * isz : nullptr, p->d_ws.p, &d_status, st, tb, (const uint64_t *)p->d_in.p,
                                      ixt, walk_tab_ok ? p->d_tab.p : nullptr, walk_tab_ok ? p->d_tab.cap : 0, full != 0, wide_band)) { p->error = QB3E_LIBERR; return done; }
                    e = hipMemcpyAsync(status.data(), d_status, 4 * cnt, hipMemcpyDeviceToHost, st);
                    if (e == hipSuccess) e = hipStreamSynchronize(st);
                    if (e != hipSuccess) { set_error("decode kernels (tiles)", (int)e); p->error = QB3E_LIBERR; return done; }
                    bool again = false;
                    for (size_t i = 0; i < cnt; i++) again = again || (status[i] & 16);
                    if (!again) break;
                }
                // a tile whose table fails its check, or whose decode from the table fails: the batch again without the tables
                bool table_trouble = false;
                for (size_t i = 0; i < cnt; i++) table_trouble = table_trouble || (bits[i] && (status[i] & (27 | 32)));
                if (!table_trouble || d_index) break;
                if (ixt.base) {
                    ixt = IxTable();
                    if (!walk_table_ready(p, g, plan, tb.n, tb.max_bits)) { p->error = QB3E_LIBERR; return done; }
                } else if (walk_tab_ok && (g.tsz >= 4 || g.mode == CM_BEST) && p->d_tab.p && walk_table_applies(g, plan)) walk_tab_ok = false;   // a stream left the band of rungs: the one-lane parser
                else break;
            }
            prof_collect();
            for (size_t i = 0; i < cnt; i++) { p->last_status |= status[i]; if (bits[i] && !(status[i] & 27)) { p->tile_ok[kk(i)] = 1; done++; } }
        }
    }
    for (size_t gi = 0; gi < ngrids; gi++) {
        const TileGrid &G = grids[gi];
        for (size_t u = 0; u < G.n; u++) {
            const size_t i = grid_k(G, u);
            if (in_batch(i)) continue;
            if (decode_tile_alone(p, (const uint8_t *)d_src + i * src_pitch, sizes[i], const_cast<uint8_t *>(grid_img(G, u)), G.stride,
                                  d_index ? (const uint8_t *)d_index + i * isz : nullptr, st)) { p->tile_ok[i] = 1; done++; }
        }
    }
    return done;
}

QB3_API size_t qb3x_decode_tiles(decsp p, const void *d_src, size_t n, size_t src_pitch, const size_t *sizes,
                                 void *d_dst, size_t dst_pitch, const void *d_index, void *stream) {
    return abi_guard<size_t>(0, [&]() -> size_t {
        if (!p || !d_src || !d_dst || !sizes || (src_pitch & 3) || ((uintptr_t)d_src & 3)) return 0;
        const TileGrid row = { n, n ? n : 1, d_dst, dst_pitch, 0, p->stride, 0, 0 };
        return decode_tile_grids(p, d_src, n, src_pitch, sizes, &row, 1, d_index, stream);
    });
}

QB3_API int qb3x_decode_tile_ok(const decsp p, size_t i) { return (p && i < p->tile_ok.size()) ? p->tile_ok[i] : 0; }
