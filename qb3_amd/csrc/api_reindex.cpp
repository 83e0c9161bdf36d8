// qb3_amd/csrc/api_reindex.cpp -- reindex, host side (qb3x_reindex_size, qb3x_reindex_device, qb3x_reindex): the kept header, the plan of
// the new container, the whole decode that leaves the index, and the two launches of k_reindex.hip.
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

// A restart table for a container that exists: the source without its "ix" / "zz" chunks and, for levels 1 and 2, with the table
// chunks this library's encoder writes for the raster in front of "DT".  The stream is never coded again: the walk of the plain
// stream (decode_common without a table) leaves a complete index in the handle's workspace, the encoder's fill code makes the
// entries of it, one launch writes the rest of the new container (k_reindex.hip).

// the header of a container that is in host memory whole, without its "ix" / "zz" chunks and without "DT" (data_off: the first
// coded byte, right behind "DT").  The chunks are stepped over as qb3_read_info steps over them.  False: they do not add up.
static bool reindex_kept_header(const uint8_t *b, size_t data_off, std::vector<uint8_t> &kept) {
    if (data_off < 13) return false;
    const size_t dt = data_off - 2;
    kept.assign(b, b + 11);
    size_t pos = 11;
    while (pos < dt) {
        if (pos + 4 > dt) return false;
        const unsigned c0 = b[pos], c1 = b[pos + 1], len = b[pos + 2] | (b[pos + 3] << 8);
        const bool known = (c0 == 'Q' && c1 == 'V') || (c0 == 'C' && c1 == 'B') || (c0 == 'S' && c1 == 'C');
        const size_t size = known ? 4 + (size_t)len : len;     // (an ignorable chunk's length counts from the chunk's start, QB3decode.cpp:254-255)
        if (!size || (!known && !(c0 & 0x20)) || pos + size > dt) return false;
        const bool drop = (c0 == 'i' && c1 == 'x') || (c0 == 'z' && c1 == 'z');
        if (!drop) kept.insert(kept.end(), b + pos, b + pos + size);
        pos += size;
    }
    return pos == dt && b[dt] == 'D' && b[dt + 1] == 'T';
}

// what a reindex call works from: the kept header, the table the encoder would write (K == 0: none), the new container's size
struct ReindexPlan { std::vector<uint8_t> hdr; Geometry g; IxTable ixt; size_t table_bytes = 0, data_off = 0, size = 0; };
static bool reindex_plan(const decsp p, int level, ReindexPlan &rp) {
    if (!p || p->stage != 2 || p->error != QB3E_OK || p->s_in == nullptr || p->s_size == 0 || level < 0 || level > 2) return false;
    rp.data_off = (size_t)(p->s_in - p->s_start);
    if (p->hdr_avail < rp.data_off + p->s_size) return false;         // a handle over a copy of the container's head only
    if (!reindex_kept_header(p->s_start, rp.data_off, rp.hdr)) return false;
    memset(&rp.g, 0, sizeof(rp.g));
    // where the encoder writes a table (encode_common): coded, not narrow, more than one block
    if (level > 0 && p->mode != QB3M_STORED && p->xsize >= 4 && p->ysize >= 4 && p->xsize * p->ysize > 16) {
        rp.g = decoder_geometry(p, p->xsize, p->ysize, 0);
        rp.ixt = ix_layout(rp.g, level);
        if (rp.ixt.K) rp.table_bytes = ix_total_bytes(rp.ixt);
    }
    rp.size = rp.hdr.size() + rp.table_bytes + 2 + p->s_size;
    return true;
}

QB3_API size_t qb3x_reindex_size(const decsp p, int level) {
    return abi_guard<size_t>(0, [&]() -> size_t {
        ReindexPlan rp;
        return reindex_plan(p, level, rp) ? rp.size : 0;
    });
}

static size_t reindex_device_body(decsp p, const void *d_src, void *d_dst, size_t dst_cap, int level, hipStream_t st) {
    ReindexPlan rp;
    if (!reindex_plan(p, level, rp) || dst_cap < rp.size) { if (p->error == QB3E_OK) p->error = QB3E_EINV; return 0; }
    if (!device_ok()) { p->error = QB3E_LIBERR; return 0; }
    uint8_t *dst = (uint8_t *)d_dst;
    if (rp.table_bytes) {
        // the index: the whole decode without the container's own table (it is not trusted, whatever it says) into the scratch
        // raster; the pixels prove the stream sound, the walk leaves bit positions, rungs, entering values, factors and unit
        // lengths of every segment in the workspace
        if (!p->d_win.ensure(qb3_decoded_size(p))) { p->error = QB3E_LIBERR; return 0; }
        const uint32_t keep_K = p->ix_K;
        const size_t keep_stride = p->stride;
        const uint64_t keep_q = p->quanta;
        p->ix_K = 0; p->stride = 0; p->quanta = 1;          // (no table, tight rows, the coded values as they are)
        const size_t n = decode_common(p, nullptr, d_src, p->d_win.p, nullptr, st);
        p->ix_K = keep_K; p->stride = keep_stride; p->quanta = keep_q;
        if (!n) { if (p->error == QB3E_OK) p->error = QB3E_ERR; return 0; }
        // a stream that ends early decodes (the reference's reader clamps) but must not be indexed: the table's last entry would
        // lie beyond its end.  Bit 6 is no fault of the stream's (which lane walked it).
        if (p->last_status & ~64u) { set_error("reindex: the stream's walk ended with a nonzero status", 0); p->error = QB3E_ERR; return 0; }
        rp.ixt.base = dst + rp.hdr.size();
        if (launch_reindex_fill(rp.g, (uint8_t *)p->d_ws.p + DEC_WS_INDEX_OFF, rp.ixt, st)) { p->error = QB3E_LIBERR; return 0; }
    } else {
        rp.ixt = IxTable();
        rp.hdr.push_back('D'); rp.hdr.push_back('T');
        p->last_status = 0;
    }
    uint8_t *pay = dst + rp.size - p->s_size;
    if (launch_reindex_finish(rp.g, rp.ixt, rp.hdr.data(), rp.hdr.size(), dst, (const uint8_t *)d_src + rp.data_off, pay, p->s_size, st)) { p->error = QB3E_LIBERR; return 0; }
    const hipError_t e = wait_stream(st);                   // (the index and the header bytes are the handle's and this call's)
    if (e != hipSuccess) { set_error("reindex kernels", (int)e); p->error = QB3E_LIBERR; return 0; }
    prof_collect();
    return rp.size;
}

QB3_API size_t qb3x_reindex_device(decsp p, const void *d_src, void *d_dst, size_t dst_cap, int level, void *stream) {
    if (!p) return 0;
    if (!d_src || !d_dst || ((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 3)) { if (p->error == QB3E_OK) p->error = QB3E_EINV; return 0; }
    return abi_guard<size_t>(0, [&] { return reindex_device_body(p, d_src, d_dst, dst_cap, level, (hipStream_t)stream); });
}

QB3_API size_t qb3x_reindex(const void *src, size_t src_size, void *dst, size_t dst_cap, int level) {
    if (!src || !dst || level < 0 || level > 2) return 0;
    return abi_guard<size_t>(0, [&]() -> size_t {
        size_t dims[3];
        decsp p = read_start_impl(const_cast<void *>(src), src_size, src_size, dims);
        if (!p) return 0;
        size_t ret = 0;
        ReindexPlan rp;
        if (qb3_read_info(p) && reindex_plan(p, level, rp) && dst_cap >= rp.size) {
            if (!rp.table_bytes) {              // level 0, STORED containers, narrow images: the chunks are dropped on the host, no device
                uint8_t *d = (uint8_t *)dst;
                memcpy(d, rp.hdr.data(), rp.hdr.size());
                d[rp.hdr.size()] = 'D'; d[rp.hdr.size() + 1] = 'T';
                memcpy(d + rp.hdr.size() + 2, p->s_in, p->s_size);
                ret = rp.size;
            } else if (device_ok()) {           // the container goes up once, the new one comes down
                hipStream_t st = nullptr;
                const size_t up = (src_size + 3) & ~(size_t)3;
                if (p->d_wsrc.ensure(up + 8) && p->d_wout.ensure(rp.size) && upload(p->stager, p->d_wsrc.p, src, src_size, st) &&
                    hipMemsetAsync((uint8_t *)p->d_wsrc.p + src_size, 0, up + 8 - src_size, st) == hipSuccess &&      // (a stream that ends early reads as zeros behind its end)
                    reindex_device_body(p, p->d_wsrc.p, p->d_wout.p, rp.size, level, st) == rp.size &&
                    download(p->stager, dst, p->d_wout.p, rp.size, st)) ret = rp.size;
            }
        }
        qb3_destroy_decoder(p);
        return ret;
    });
}
