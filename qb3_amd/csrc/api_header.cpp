// qb3_amd/csrc/api_header.cpp -- container headers of the C ABI: the encoder's header writer; the decoder's parser (qb3_read_start,
// qb3_read_info and their device flavour), the plain getters, and what the kernels are told of a parsed header: the container's
// restart table (handle_table) and the geometry the raster decodes with (decoder_geometry).
#include <new>
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

static inline unsigned topbit(uint64_t v) { return 63u - (unsigned)__builtin_clzll(v); }

// ---------------------------------------------------------------- small host bit writer for headers
struct HdrWriter {
    uint8_t *d; size_t n = 0;
    explicit HdrWriter(uint8_t *dst) : d(dst) {}
    void put(uint64_t v, unsigned bytes) { for (unsigned i = 0; i < bytes; i++) d[n++] = (uint8_t)(v >> (8 * i)); }
    void sig(const char *s) { d[n++] = (uint8_t)s[0]; d[n++] = (uint8_t)s[1]; }
};

// reference QB3encode.cpp:189-268: main header, then CB / QV / SC chunks as needed, then DT.
// with_dt = false: the caller continues the header (the restart-table chunks and "DT" are written on the device)
size_t qb3api::write_headers(const encs *p, uint8_t *dst, bool with_dt) {
    HdrWriter w(dst);
    w.put(0x80334251u, 4);
    w.put(p->xsize - 1, 2); w.put(p->ysize - 1, 2); w.put(p->nbands - 1, 1);
    w.put((uint8_t)p->type, 1); w.put((uint8_t)p->mode, 1);
    bool diff = false;
    for (size_t c = 0; c < p->nbands; c++) diff |= p->cband[c] != c;
    if (p->mode != QB3M_STORED && diff) {
        w.sig("CB"); w.put(p->nbands, 2);
        for (size_t c = 0; c < p->nbands; c++) w.put(p->cband[c], 1);
    }
    if (p->quanta >= 2) {
        unsigned qb = 1 + topbit(p->quanta) / 8;
        w.sig("QV"); w.put(qb, 2); w.put(p->quanta, qb);
    }
    if (p->order != ZCURVE && p->mode != QB3M_STORED) {
        w.sig("SC"); w.put(8, 2); w.put(p->order ? p->order : HILBERT, 8);
    }
    if (with_dt) w.sig("DT");
    return w.n;
}

// ---------------------------------------------------------------- decoder: the plain getters, the parser
QB3_API size_t qb3_decoded_size(const decsp p) { return p->xsize * p->ysize * p->nbands * szof(p->type); }
QB3_API qb3_dtype qb3_get_type(const decsp p) { return p->type; }
QB3_API qb3_mode qb3_get_mode(const decsp p) { return (2 == p->stage) ? p->mode : QB3M_INVALID; }
QB3_API uint64_t qb3_get_quanta(const decsp p) { return (2 == p->stage) ? p->quanta : 0; }
QB3_API uint64_t qb3_get_order(const decsp p) { return (p->stage != 2) ? 0 : (p->order ? p->order : ZCURVE); }
QB3_API bool qb3_get_coreband(const decsp p, size_t *coreband) {
    if (p->stage != 2) return false;
    for (size_t c = 0; c < p->nbands; c++) coreband[c] = p->cband[c];
    return true;
}

// reference QB3decode.cpp:130-172.  hdr_avail: bytes readable at `source` (the device flavour may hand over a copy of
// the container's head only, with source_size still the size of the whole container)
decsp qb3api::read_start_impl(void *source, size_t hdr_avail, size_t source_size, size_t *image_size) {
    if (!source || source_size < 15 || hdr_avail < 15 || !image_size) return nullptr;
    const uint8_t *b = (const uint8_t *)source;
    if (b[0] != 'Q' || b[1] != 'B' || b[2] != '3' || b[3] != 0x80) return nullptr;
    const size_t nb = 1 + (size_t)b[8];
    const int type = b[9], mode = b[10];
    if (nb > QB3_MAXBANDS || (mode >= (int)QB3M_END && mode != (int)QB3M_STORED) || ((b[11] | b[12]) & 0x80) || type > (int)QB3_I64)
        return nullptr;
    decs *p = new decs();
    p->xsize = 1 + (size_t)(b[4] | (b[5] << 8));
    p->ysize = 1 + (size_t)(b[6] | (b[7] << 8));
    p->nbands = nb; p->type = (qb3_dtype)type; p->mode = (qb3_mode)mode;
    p->stride = 0; p->order = 0; p->quanta = 0; p->error = QB3E_OK; p->stage = 1;
    memset(p->cband, 0, sizeof(p->cband));
    p->s_start = (uint8_t *)source;
    p->s_in = p->s_start + 11; p->s_size = source_size - 11;
    p->hdr_avail = hdr_avail < source_size ? hdr_avail : source_size;
    p->saw_cb = false; p->compat = 0;
    p->ix_off = 0; p->ix_K = p->ix_blocks = p->ix_E = p->ix_per_chunk = 0; p->ix_pads = false; p->ix_bad = false; p->ix_bl = false;
    p->ix_ver = 0; p->ix_heads_unchecked = false; p->ix_need_off = 0; p->hdr_short = false;
    image_size[0] = p->xsize; image_size[1] = p->ysize; image_size[2] = p->nbands;
    if (mode <= (int)QB3M_CF_RLE) p->order = ZCURVE;
    return p;
}
QB3_API decsp qb3_read_start(void *source, size_t source_size, size_t *image_size) {
    return abi_guard<decsp>(nullptr, [&] { return read_start_impl(source, source_size, source_size, image_size); });
}
QB3_API decsp qb3x_read_start(void *header, size_t header_size, size_t stream_size, size_t *image_size) {
    return abi_guard<decsp>(nullptr, [&] { return read_start_impl(header, header_size, stream_size, image_size); });
}
// Upper bound of the bytes in front of the block stream of a container that starts with these (at least 11) bytes:
// the fixed header, the reference's chunks and this library's restart-table chunks for the worst mode.
QB3_API size_t qb3x_header_size_bound(const void *container, size_t avail) {
    const uint8_t *b = (const uint8_t *)container;
    if (!b || avail < 11 || b[0] != 'Q' || b[1] != 'B' || b[2] != '3' || b[3] != 0x80) return 0;
    const size_t w = 1 + (size_t)(b[4] | (b[5] << 8)), h = 1 + (size_t)(b[6] | (b[7] << 8)), nb = 1 + (size_t)b[8];
    const size_t tsz = szof(b[9]);
    if (!tsz || nb > QB3_MAXBANDS) return 0;
    // an entry covers at least 12 units (one common-factor segment) and takes at most 6 + bands * (1 + 2 * tsz) bytes
    const size_t units = ((w + 3) / 4) * ((h + 3) / 4) * nb, E = 6 + nb * (1 + 2 * tsz);
    const size_t K = units / 12 + 1;
    // ... and a table of 8-bit data may carry ten bits per block on top (an entry per 64 blocks)
    const size_t nblk = ((w + 3) / 4) * ((h + 3) / 4);
    const size_t bl = tsz == 1 ? (nblk / 64 + 1) * (64 * IX_BL_BEST_BYTES) : tsz == 2 ? (nblk * (nb / 4 + 1) / 64 + 1) * ((128 * IX_BL_BITS + 7) / 8)
                               : std::max((nblk * nb * IX_BL_BITS_WIDE) / 8 + (nblk / 12 + 1) * 2 + 64,      // (32/64-bit: a length per unit, an odd byte per entry)
                                          nblk * IX_BL_BEST_BYTES + 64);                                    // (... or, one band, common factor: a field per block)
    // ... and a table of the lane-per-unit decoder's rasters a field per UNIT: three bytes (common factor) or twelve bits
    const size_t blu = nblk * nb * IX_BL_BEST_BYTES + 64 * IX_BL_BEST_BYTES;
    const size_t bytes = K * E + std::max(bl, blu);
    return 128 + bytes + (bytes / 60000 + 1) * (IX_HEAD + IX_PAD);
}

static bool valid_curve(uint64_t v) {
    unsigned mask = 0;
    for (int i = 0; i < 16; i++, v >>= 4) mask |= 1u << (v & 15);
    return mask == 0xffff;
}

// reference QB3decode.cpp:176-264; chunks are byte aligned, so this walks bytes
QB3_API bool qb3_read_info(decsp p) {
    if (p->stage != 1 || p->error || !p->s_in || p->s_size < 4) {
        if (QB3E_OK == p->error) p->error = QB3E_EINV;
        return false;
    }
    const uint8_t *s = p->s_in;
    const size_t n = p->s_size;
    const size_t avail = p->hdr_avail > 11 ? p->hdr_avail - 11 : 0;           // bytes readable at s (<= n)
    size_t pos = 0;
    bool short_copy = false;                                                   // the head copy ends before the header does
    auto have = [&](size_t at) -> bool {                                       // is the byte on the host
        return at < avail || (at + 11 >= p->win2_off && at + 11 - p->win2_off < p->win2.size());
    };
    auto rd = [&](size_t at) -> unsigned {                                     // reads past the end give zeros
        if (at < avail) return s[at];
        if (at + 11 >= p->win2_off && at + 11 - p->win2_off < p->win2.size()) return p->win2[at + 11 - p->win2_off];
        if (at < n) short_copy = true;
        return 0u;
    };
    do {
        const unsigned c0 = rd(pos), c1 = rd(pos + 1), len = rd(pos + 2) | (rd(pos + 3) << 8);
        if (c0 == 'Q' && c1 == 'V') {
            if (len > 4 || len < 1) { p->error = QB3E_EINV; break; }
            pos += 4;
            uint64_t q = 0;
            for (unsigned i = 0; i < len; i++) q |= (uint64_t)rd(pos + i) << (8 * i);
            pos += len;
            p->quanta = q;
            if (p->quanta < 2) p->error = QB3E_EINV;
        } else if (c0 == 'C' && c1 == 'B') {
            if (len != p->nbands) { p->error = QB3E_EINV; break; }
            pos += 4;
            for (size_t i = 0; i < p->nbands; i++) {
                p->cband[i] = (uint8_t)rd(pos++);
                if (p->cband[i] >= p->nbands) p->error = QB3E_EINV;
            }
            p->saw_cb = true;
        } else if (c0 == 'D' && c1 == 'T') {
            pos += 2;
            if (pos > n) pos = n;
            if (p->s_size <= pos) { p->error = QB3E_EINV; break; }
            p->s_in += pos; p->s_size -= pos; p->stage = 2;
        } else if (c0 == 'S' && c1 == 'C') {
            if (len != 8) { p->error = QB3E_EINV; break; }
            if ((int)p->mode < (int)QB3M_BASE_H || p->mode == QB3M_STORED) { p->error = QB3E_EINV; break; }
            pos += 4;
            uint64_t o = 0;
            for (unsigned i = 0; i < 8; i++) o |= (uint64_t)rd(pos + i) << (8 * i);
            pos += 8;
            p->order = o;
            if (!valid_curve(o)) { p->error = QB3E_EINV; break; }
        } else {
            // the reference skips an ignorable (lower case) chunk by `len` bytes from the chunk start
            // (QB3decode.cpp:254-255); a zero length would never terminate there, treat it as an error
            if (c0 == 'i' && c1 == 'x' && len >= IX_HEAD && rd(pos + 4) >= 1 && rd(pos + 4) <= 3 && p->mode != QB3M_STORED) {
                // this library's restart table (include/qb3x.h): a run of such chunks, all but the last of the same
                // size, each followed by a 4-byte pad chunk (version 2).  Remember where it is, check it later.
                const size_t tsz = szof(p->type);
                const uint32_t blocks = rd(pos + 8) | (rd(pos + 9) << 8) | (rd(pos + 10) << 16) | (rd(pos + 11) << 24);
                const bool bl = (rd(pos + 5) & 2) != 0;     // entries end with their blocks' bit lengths
                const bool cfe = (rd(pos + 5) & 1) != 0;     // entries carry the common factors
                const uint32_t E = (uint32_t)(6 + p->nbands * (1 + tsz * (cfe ? 2 : 1))) + (bl && blocks <= 4096 ? ix_bl_bytes((uint32_t)tsz, (uint32_t)p->nbands, blocks, cfe) : 0);
                const size_t at = (size_t)(p->s_in - p->s_start) + pos;
                const unsigned ver = rd(pos + 4);
                const bool v2 = ver >= 2;
                if ((len - IX_HEAD) % E || pos + len > n) p->ix_bad = true;
                else if (!p->ix_K) {        // the first chunk
                    p->ix_off = at; p->ix_E = E; p->ix_blocks = blocks; p->ix_pads = v2; p->ix_bl = bl; p->ix_ver = ver;
                    p->ix_per_chunk = p->ix_K = (len - IX_HEAD) / E;
                    // A regular table -- every chunk but the last full, a pad behind each, "DT" behind the last -- is stepped over in
                    // one go when "DT" stands where such a table ends: the heads in between are then checked on the device
                    // (ix_check_kernel) and need not be on the host at all (a 16384 x 16384 raster's level 2 table is 24 MB)
                    const uint64_t nblk = (uint64_t)((p->xsize + 3) / 4) * ((p->ysize + 3) / 4);
                    const uint64_t Kexp = blocks ? (nblk + blocks - 1) / blocks : 0;
                    // -- only then: with the whole container on the host the chunks are walked one by one, as the reference's
                    // parser walks them (garbage between the first chunk and "DT" is an error, not a table)
                    const bool all_here = p->hdr_avail >= 11 + n;
                    if (!all_here && v2 && p->ix_per_chunk && Kexp > p->ix_per_chunk && Kexp < 0xffffffffull) {
                        const uint64_t nch = (Kexp + p->ix_per_chunk - 1) / p->ix_per_chunk;
                        const uint64_t total = nch * (IX_HEAD + IX_PAD) + Kexp * E;
                        if (pos + total + 2 < n) {
                            if (have(pos + total) && have(pos + total + 1)) {
                                if (rd(pos + total) == 'D' && rd(pos + total + 1) == 'T') {
                                    p->ix_K = (uint32_t)Kexp; p->ix_heads_unchecked = true;
                                    pos += total;
                                    continue;
                                }
                            } else p->ix_need_off = 11 + pos + total;
                        }
                    }
                } else {                    // a further one: in place, same shape, and only the last may be short
                    const size_t full = IX_HEAD + (size_t)p->ix_per_chunk * E + (p->ix_pads ? IX_PAD : 0);
                    const uint32_t here = (len - IX_HEAD) / E;
                    if (!v2 || !p->ix_pads || ver != p->ix_ver || E != p->ix_E || blocks != p->ix_blocks || bl != p->ix_bl || p->ix_K % p->ix_per_chunk ||
                        at != p->ix_off + (p->ix_K / p->ix_per_chunk) * full || here > p->ix_per_chunk) p->ix_bad = true;
                    else p->ix_K += here;
                }
            }
            if ((c0 & 0x20) && len) pos += len;
            else p->error = QB3E_UNKN;
        }
        if (pos > n) pos = n;
    } while (p->stage != 2 && QB3E_OK == p->error && pos < n);
    if (QB3E_OK == p->error && 2 != p->stage) p->error = QB3E_EINV;
    if (short_copy && QB3E_OK == p->error) p->error = QB3E_EINV;               // qb3x_read_start: the head copy is too short
    p->hdr_short = short_copy;
    if (p->ix_bad) p->ix_K = 0;
    return QB3E_OK == p->error;
}

// qb3_read_start + qb3_read_info for a container in DEVICE memory: the handle keeps its own host copy of the container's
// first bytes (up to 512), and when a restart table pushes the "DT" mark beyond them, of the few bytes where a regular
// table ends -- two small copies instead of the whole table (24 MB for a 16384 x 16384 x 3 raster at level 2), whose
// chunk heads and checks the device verifies before the table is used (ix_check_kernel).  A table that is not regular
// is read whole.  Returns a handle in the state qb3_read_info leaves, or NULL.
static decsp read_start_device_body(const void *d_container, size_t nbytes, size_t *image_size, void *stream) {
    if (!d_container || nbytes < 15 || !image_size || !device_ok()) return nullptr;
    hipStream_t st = (hipStream_t)stream;
    auto fetch = [&](std::vector<uint8_t> &dst, size_t off, size_t n) -> bool {
        dst.resize(n);
        return hipMemcpyAsync(dst.data(), (const uint8_t *)d_container + off, n, hipMemcpyDeviceToHost, st) == hipSuccess &&
               hipStreamSynchronize(st) == hipSuccess;
    };
    std::vector<uint8_t> head, win;
    size_t win_off = 0;
    if (!fetch(head, 0, std::min(nbytes, (size_t)512))) return nullptr;
    for (int turn = 0; turn < 3; turn++) {
        decs *p = read_start_impl(head.data(), head.size(), nbytes, image_size);
        if (!p) return nullptr;
        p->own_head.swap(head);                         // (the vector's buffer stays where it is: s_start stays valid)
        p->win2 = win; p->win2_off = win_off;
        if (qb3_read_info(p)) return p;
        const size_t need = p->ix_need_off;
        head.swap(p->own_head);
        const bool was_short = p->hdr_short;
        if (getenv("QB3_DEBUG_RS")) fprintf(stderr, "read_start_device turn %d: need %zu short %d err %d ix_off %zu K %u E %u per %u ver %u\n", turn, need, (int)was_short, p->error, p->ix_off, p->ix_K, p->ix_E, p->ix_per_chunk, p->ix_ver);
        qb3_destroy_decoder(p);
        if (!was_short) return nullptr;
        if (turn == 0 && need && need + 2 <= nbytes) {  // a regular table: the mark behind it (four bytes: the chunk loop reads a length field behind every tag)
            win_off = need;
            if (!fetch(win, need, std::min<size_t>(4, nbytes - need))) return nullptr;
        } else if (turn <= 1) {                         // something else: the whole head, as far as a table can reach
            const size_t bound = std::min(nbytes, qb3x_header_size_bound(head.data(), head.size()));
            if (bound <= head.size()) return nullptr;
            win.clear(); win_off = 0;
            if (!fetch(head, 0, bound)) return nullptr;
        } else return nullptr;
    }
    return nullptr;
}
QB3_API decsp qb3x_read_start_device(const void *d_container, size_t nbytes, size_t *image_size, void *stream) {
    return abi_guard<decsp>(nullptr, [&] { return read_start_device_body(d_container, nbytes, image_size, stream); });
}

QB3_API size_t qb3x_decoder_table_entries(const decsp p) { return (p && p->stage == 2) ? p->ix_K : 0; }

QB3_API size_t qb3x_decoder_index_size(const decsp p) {
    if (!p || p->stage != 2 || p->xsize < 4 || p->ysize < 4) return 0;
    Geometry g = make_geometry(p->xsize, p->ysize, p->nbands, p->type, 0, p->order, p->mode, nullptr, p->cband);
    return index_bytes(g);
}

// the container's restart table as qb3_read_info found it, its chunks at `base` in device memory
IxTable qb3api::handle_table(const decs *p, const uint8_t *base) {
    IxTable t;
    t.base = const_cast<uint8_t *>(base);
    t.K = p->ix_K; t.blocks = p->ix_blocks; t.entry_bytes = p->ix_E; t.per_chunk = p->ix_per_chunk; t.pads = p->ix_pads; t.block_lens = p->ix_bl;
    t.version = p->ix_ver; t.check_heads = p->ix_heads_unchecked;
    return t;
}

// the geometry a coded raster of w x h pixels (the container's, or a narrow image's stand-in) decodes with; stride in values, 0: tight rows
Geometry qb3api::decoder_geometry(const decs *p, size_t w, size_t h, size_t stride) {
    uint8_t cband[QB3_MAXBANDS];
    for (size_t c = 0; c < QB3_MAXBANDS; c++) cband[c] = p->cband[c];
    // no CB chunk means identity; the reference leaves the map zero filled instead
    if (!p->saw_cb && !(p->compat & QB3X_REF_CBAND0)) for (size_t c = 0; c < p->nbands; c++) cband[c] = (uint8_t)c;
    return make_geometry(w, h, p->nbands, p->type, stride, p->order, p->mode, nullptr, cband);
}
