// qb3_amd/csrc/api_ranged.cpp -- ranged window reads (include/qb3x.h: qb3x_open_ranged, qb3x_read_windows_ranged,
// qb3x_decode_windows_ranged): windows of a container that is read through a function of the caller's, fetching only the table chunks
// and the pieces of the stream that hold the rectangles.  The rules of what is read are stated in qb3x.h; the kernels that decode from
// the pieces are the ranged form of the family that takes the raster (qb3_dev.h: window_family; a family without that form is no
// shortcut here); everything the shortcut does not take goes, with the whole container, the way of api_window.cpp.
#include <new>
#include "qb3_host.h"

using namespace qb3dev;
using namespace qb3api;

namespace {

// one call of the caller's reader, counted; never for bytes outside the container
bool rg_read(decs *p, uint64_t off, void *dst, size_t n) {
    if (!n) return true;
    if (off > p->rg_size || n > p->rg_size - off) return false;
    p->rg_reads++; p->rg_bytes += n;
    return p->rg_rd(p->rg_ctx, off, dst, n) == 0;
}
uint64_t pos6(const uint8_t *q) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < 6; i++) v |= (uint64_t)q[i] << (8 * i);
    return v;
}

// ---------------------------------------------------------------- the table's chunks in the container
struct Chunks {
    uint64_t off = 0;               // of the first chunk
    uint32_t K = 0, N = 0, E = 0, count = 0;
    uint64_t at(uint32_t c) const { return off + (uint64_t)c * (IX_HEAD + IX_PAD + (uint64_t)N * E); }
    uint32_t entries(uint32_t c) const { return c + 1 < count ? N : K - c * N; }
    size_t size(uint32_t c) const { return IX_HEAD + (size_t)entries(c) * E + IX_PAD + (c + 1 == count ? 2 : 0); }
};

// does the shortcut take this handle's raster and table, and with which family's kernels (pure: no device, no reader); null: no
const WinKernels *ranged_shortcut(const decs *p, Geometry &g, DecPlan &plan, IxTable &ixt, Chunks &ch) {
    if (p->mode == QB3M_STORED || p->xsize < 4 || p->ysize < 4 || !p->ix_K || !p->ix_bl || p->ix_ver < 3 || !p->ix_pads || is_rle_mode(p->mode)) return nullptr;
    g = decoder_geometry(p, p->xsize, p->ysize, 0);
    plan = plan_decode(g);
    ixt = handle_table(p, (const uint8_t *)p);          // (the table is not in device memory: the base only has to be non-null)
    const WinKernels *family = window_family(g, plan, ixt, p->win_kernels);
    if (!family || !family->ranged) return nullptr;
    ch.off = p->ix_off; ch.K = p->ix_K; ch.N = p->ix_per_chunk; ch.E = p->ix_E; ch.count = (uint32_t)ix_chunks(ixt);
    return ch.at(ch.count - 1) + ch.size(ch.count - 1) <= p->rg_size ? family : nullptr;
}

std::vector<WinRect> window_rects(const qb3x_window *wins, size_t n) {      // (strides: filled where they matter)
    std::vector<WinRect> rects(n);
    for (size_t i = 0; i < n; i++) rects[i] = WinRect{ (uint32_t)wins[i].x0, (uint32_t)wins[i].y0, (uint32_t)wins[i].w, (uint32_t)wins[i].h, 0 };
    return rects;
}

// The host twin of ix_check_chunk (qb3_kernels.h): head (flag bit 0: common-factor entries; bit 1: block fields, which the shortcut
// requires), pad, the mark behind the last chunk, and the 16-bit check of the entries
bool chunk_sound(const decs *p, const Chunks &ch, uint32_t c, const uint8_t *b, uint32_t flags) {
    const uint32_t n = ch.entries(c) * ch.E, len = IX_HEAD + n;
    const uint32_t blocks = b[8] | (b[9] << 8) | (b[10] << 16) | ((uint32_t)b[11] << 24);
    if (b[0] != 'i' || b[1] != 'x' || (uint32_t)(b[2] | (b[3] << 8)) != len || b[4] != p->ix_ver || (b[5] & 3) != flags || blocks != p->ix_blocks) return false;
    if (b[len] != 'z' || b[len + 1] != 'z' || b[len + 2] != 4 || b[len + 3] != 0) return false;
    if (c + 1 == ch.count && (b[len + IX_PAD] != 'D' || b[len + IX_PAD + 1] != 'T')) return false;
    uint32_t s = 0;
    const uint8_t *e = b + IX_HEAD;
    for (uint32_t i = 0; i < n; i++) s += ((uint32_t)e[i] + 1u) * (i * 0x9e3779b1u + 1u);
    return ((s ^ (s >> 16)) & 0xffffu) == (uint32_t)(b[6] | (b[7] << 8));
}

// Stage 1: the chunks of the list, from the handle's cache or the reader (each whole, verified before it is kept).  data[i]: chunk
// chunks[i].  0: all sound; 1: a chunk failed its check; 2: the reader failed
int fetch_chunks(decs *p, const Chunks &ch, const std::vector<uint32_t> &chunks, std::vector<const uint8_t *> &data, uint32_t flags) {
    data.assign(chunks.size(), nullptr);
    for (size_t i = 0; i < chunks.size(); i++) {
        bool cached = false;
        for (const auto &kept : p->rg_chunks) cached = cached || kept.first == chunks[i];
        if (cached) continue;
        std::vector<uint8_t> b(ch.size(chunks[i]));
        if (!rg_read(p, ch.at(chunks[i]), b.data(), b.size())) return 2;
        if (!chunk_sound(p, ch, chunks[i], b.data(), flags)) return 1;
        p->rg_cache_bytes += b.size();
        p->rg_chunks.emplace_back(chunks[i], std::move(b));
    }
    for (size_t i = 0; i < chunks.size(); i++)
        for (const auto &kept : p->rg_chunks) if (kept.first == chunks[i]) data[i] = kept.second.data();
    return 0;
}
// ... and behind the call: the oldest leave until the cache is within its bound
void trim_cache(decs *p) {
    size_t drop = 0;
    while (drop < p->rg_chunks.size() && p->rg_cache_bytes > p->rg_cache_cap) p->rg_cache_bytes -= p->rg_chunks[drop++].second.size();
    p->rg_chunks.erase(p->rg_chunks.begin(), p->rg_chunks.begin() + drop);
}

struct Piece { uint32_t seg0, nseg, ent0, word0, sw0_lo, sw0_hi, nwords, pad_; };      // WinPiece of qb3_win.h, as uploaded
static_assert(sizeof(Piece) == WIN_PIECE_BYTES, "the piece list is uploaded as it is");
// The whole container through the reader, once, and the windows the way of qb3x_read_windows / qb3x_decode_windows_device
size_t whole_container(decsp p, const qb3x_window *wins, size_t n, uint8_t *paths, bool host, hipStream_t st) {
    const size_t csize = (size_t)p->rg_size, off = (size_t)(p->s_in - p->s_start);
    std::vector<uint8_t> whole(csize);
    if (!rg_read(p, 0, whole.data(), csize)) { p->error = QB3E_ERR; return 0; }
    uint8_t *const keep_start = p->s_start, *const keep_in = p->s_in;
    const size_t keep_avail = p->hdr_avail;
    p->s_start = whole.data(); p->s_in = whole.data() + off; p->hdr_avail = csize;
    size_t done = 0;
    if (host) done = windows_check(p, wins, n, true) ? windows_host(p, wins, n, paths, false) : 0;
    else if (!device_ok()) p->error = QB3E_LIBERR;
    else if (!p->d_wsrc.ensure(csize + 8) || !upload(p->stager, p->d_wsrc.p, whole.data(), csize, st) ||
             hipMemsetAsync((uint8_t *)p->d_wsrc.p + csize, 0, 8, st) != hipSuccess) p->error = QB3E_LIBERR;
    else {
        done = windows_device(p, p->d_wsrc.p, nullptr, wins, n, paths, false, st);
        (void)hipStreamSynchronize(st);                 // (the container's device copy is the handle's)
    }
    p->s_start = keep_start; p->s_in = keep_in; p->hdr_avail = keep_avail;
    return done;
}

// STORED: the windows' rows straight from their offsets (reference QB3decode.cpp:356-375); no table, and a device only for device destinations
size_t stored_windows(decsp p, const qb3x_window *wins, size_t n, uint8_t *paths, bool host, hipStream_t st) {
    const size_t tsz = szof(p->type), pix = p->nbands * tsz, line = p->xsize * pix, off = (size_t)(p->s_in - p->s_start);
    if (p->s_size != qb3_decoded_size(p)) { p->error = QB3E_EINV; return 0; }
    if (!host && !device_ok()) { p->error = QB3E_LIBERR; return 0; }
    std::vector<uint8_t> tmp;
    for (size_t i = 0; i < n; i++) {
        const qb3x_window &w = wins[i];
        const size_t wline = w.w * pix, dline = host ? win_stride(p, w) * tsz : wline;
        uint8_t *to = (uint8_t *)w.dst;
        if (!host) { tmp.resize(w.h * wline); to = tmp.data(); }
        bool ok;
        if (wline == line && dline == line) ok = rg_read(p, off + w.y0 * line, to, w.h * line);       // whole rows, tight: one piece
        else {
            ok = true;
            for (size_t y = 0; ok && y < w.h; y++) ok = rg_read(p, off + (w.y0 + y) * line + w.x0 * pix, to + y * dline, wline);
        }
        if (!ok) { p->error = QB3E_ERR; return 0; }
        if (!host) {
            if (hipMemcpy2DAsync(w.dst, win_stride(p, w) * tsz, to, wline, wline, w.h, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { p->error = QB3E_LIBERR; return 0; }
        }
        paths[i] = 3;
    }
    p->win_path = 3;
    return n;
}

// The shortcut.  Marks the windows it gave their pixels (paths[i] = 1) and counts their segments.  1: went through (fall back for the
// windows that are left); 0: the table is not to be trusted, nothing was written; -1: the call failed (p->error is set).  family:
// whose kernels -- a raster has its own blocks per segment (g.seg_blocks) and value size, a common-factor one its own entries (ch.E)
// and head flags; all else is one code
int pieces_windows(decsp p, const Geometry &g, const DecPlan &plan, const IxTable &ixt, const Chunks &ch, const qb3x_window *wins, size_t n,
                   uint8_t *paths, size_t *segs, bool host, hipStream_t st, const WinKernels &family) {
    const size_t tsz = szof(p->type), pix = p->nbands * tsz;
    const uint64_t csize = p->rg_size, off = (uint64_t)(p->s_in - p->s_start), base = off & ~(uint64_t)3, in_bits = (uint64_t)p->s_size * 8;
    const uint32_t in_bit0 = (uint32_t)(8 * (off & 3));
    // stage 1: the table chunks the windows' entries are in
    std::vector<uint32_t> chunks;
    std::vector<const uint8_t *> cdata;
    std::vector<WinRect> rects = window_rects(wins, n);
    window_chunk_list(g, ch.K, ch.N, rects.data(), n, chunks);
    const int got = fetch_chunks(p, ch, chunks, cdata, g.mode == CM_BEST ? 3u : 2u);
    if (got == 2) { p->error = QB3E_ERR; return -1; }
    if (got) return 0;
    auto entry = [&](uint32_t k) -> const uint8_t * {
        const uint32_t c = k / ch.N;
        const size_t i = (size_t)(std::lower_bound(chunks.begin(), chunks.end(), c) - chunks.begin());
        return cdata[i] + IX_HEAD + (size_t)(k - c * ch.N) * ch.E;
    };
    if (pos6(entry(ch.K - 1)) > in_bits) return 0;      // the tail check: a stream cut short is for the whole decode to judge
    // stage 2: runs of segments, one per block row of a window; merged where they overlap or follow each other
    std::vector<std::pair<uint32_t, uint32_t>> runs;    // [first, end)
    for (size_t i = 0; i < n; i++) {
        const WinBlocks b = window_blocks(g, wins[i].x0, wins[i].y0, wins[i].w, wins[i].h);
        for (uint64_t by = b.by0; by <= b.by1; by++) runs.emplace_back((uint32_t)((by * g.nbx + b.bx0) / g.seg_blocks), (uint32_t)((by * g.nbx + b.bx1) / g.seg_blocks + 1));
    }
    merge_ranges(runs);
    // a piece per run whose two ends make sense: inside the stream, no longer than its segments can be (px_cap_dw: the worst-case
    // segment of every family; a table that says otherwise is not this stream's; the waves of such a run find no piece and raise
    // their window's status)
    std::vector<Piece> pieces;
    std::vector<std::pair<uint64_t, uint64_t>> spans;  // container bytes [first, second) ...
    std::vector<size_t> span_at;                        // ... and where they start in the packed words (bytes)
    std::vector<uint64_t> piece_a;
    size_t nents = 0;
    for (const auto &r : runs) {
        const uint64_t P0 = pos6(entry(r.first)), P1 = r.second < ch.K ? pos6(entry(r.second)) : in_bits;
        if (P0 > P1 || P1 > in_bits) continue;
        const uint64_t w0 = (in_bit0 + P0) >> 5, w1 = (in_bit0 + P1 + 31) >> 5;
        if (w1 - w0 > (uint64_t)(r.second - r.first) * plan.px_cap_dw) continue;
        Piece pc = { r.first, r.second - r.first, (uint32_t)nents, 0, (uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)(w1 - w0), 0 };
        nents += pc.nseg + 1;
        const uint64_t a = std::min(base + 4 * w0, csize), b = std::min(base + 4 * w1, csize);
        pieces.push_back(pc);
        piece_a.push_back(a);
        if (b > a) spans.emplace_back(a, b);
    }
    if (pieces.empty() || nents > 0x7fffffffull) return 0;
    merge_ranges(spans, (uint64_t)p->rg_gap);
    uint64_t wbytes = 0;
    for (const auto &s : spans) { span_at.push_back((size_t)wbytes); wbytes += (s.second - s.first + 3) & ~(uint64_t)3; }
    if (wbytes >= ((uint64_t)1 << 32)) return 0;
    // what goes up, in one pinned area: descriptors, piece list, entries, words
    const size_t dbytes = n * WIN_DESC_BYTES, pbytes = pieces.size() * sizeof(Piece), ebytes = (nents * ch.E + 15) & ~(size_t)15;
    const size_t upbytes = dbytes + pbytes + ebytes + (size_t)wbytes + 4, stbytes = 4 * (n + 1);
    if (!device_ok()) { p->error = QB3E_LIBERR; return -1; }
    std::vector<void *> dsts(n);
    if (!p->h_rg.ensure(upbytes) || !p->d_rg.ensure(upbytes) || !p->h_wst.ensure(stbytes) || !p->d_wst.ensure(stbytes) || (host && !windows_out(p, wins, n, dsts))) {
        p->error = QB3E_LIBERR;
        return -1;
    }
    uint8_t *up = (uint8_t *)p->h_rg.p, *h_words = up + dbytes + pbytes + ebytes;
    for (size_t i = 0; i < n; i++) {
        rects[i].stride = host ? wins[i].w * p->nbands : win_stride(p, wins[i]);
        if (!host) dsts[i] = wins[i].dst;
    }
    std::vector<uint32_t> unused;
    uint64_t wsegs = 0;
    window_batch_plan(g, ixt, rects.data(), dsts.data(), n, up, unused, &wsegs);
    for (size_t k = 0; k < pieces.size(); k++) {        // every piece lies in one span: the last that starts at or in front of it
        Piece &pc = pieces[k];
        uint8_t *e = up + dbytes + pbytes + (size_t)pc.ent0 * ch.E;
        for (uint32_t j = 0; j <= pc.nseg; j++, e += ch.E) {
            if (pc.seg0 + j < ch.K) memcpy(e, entry(pc.seg0 + j), ch.E);
            else memset(e, 0, ch.E);                    // (behind the raster's last segment: the stream's length ends it)
        }
        size_t lo = 0, hi = spans.size();
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (spans[mid].first <= piece_a[k]) lo = mid; else hi = mid; }
        uint64_t avail = 0;
        if (!spans.empty() && spans[lo].first <= piece_a[k]) {
            const uint64_t rel = piece_a[k] - spans[lo].first, room = (spans[lo].second - spans[lo].first + 3) & ~(uint64_t)3;
            if (rel <= room) { pc.word0 = (uint32_t)((span_at[lo] + rel) / 4); avail = (room - rel) / 4; }
        }
        pc.nwords = (uint32_t)std::min<uint64_t>(pc.nwords, avail);        // never a word outside what was packed
    }
    memcpy(up + dbytes, pieces.data(), pbytes);
    for (size_t k = 0; k < spans.size(); k++) {
        const size_t len = (size_t)(spans[k].second - spans[k].first);
        if (!rg_read(p, spans[k].first, h_words + span_at[k], len)) { p->error = QB3E_ERR; return -1; }
        memset(h_words + span_at[k] + len, 0, (0 - len) & 3);
    }
    // one copy up, one launch, the status words back
    uint32_t *d_status = (uint32_t *)p->d_wst.p;
    const uint8_t *d_up = (const uint8_t *)p->d_rg.p;
    auto hip_fail = [&](const char *what, hipError_t e) { set_error(what, (int)e); (void)hipStreamSynchronize(st); p->error = QB3E_LIBERR; return -1; };
    hipError_t e = hipMemcpyAsync(p->d_rg.p, up, upbytes - 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, stbytes, st);
    if (e != hipSuccess) return hip_fail("ranged windows: upload", e);
    if (launch_decode_windows_ranged(family, g, plan, in_bit0, in_bits, up, d_up, n, d_up + dbytes, pieces.size(), d_up + dbytes + pbytes,
                                     (const uint32_t *)(d_up + dbytes + pbytes + ebytes), d_status, st, ixt)) return hip_fail("ranged windows: launch", hipSuccess);
    e = hipMemcpyAsync(p->h_wst.p, d_status, stbytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = wait_stream(st);
    if (e != hipSuccess) return hip_fail("ranged windows: kernel", e);
    const uint32_t *status = (const uint32_t *)p->h_wst.p;
    *segs = (size_t)wsegs;
    for (size_t i = 0; i < n; i++) {
        if (status[1 + i]) continue;
        paths[i] = 1;
        if (!window_dequantize(p, g, dsts[i], rects[i].w, rects[i].h, rects[i].stride, st)) return hip_fail("ranged windows: dequantize", hipSuccess);
        if (host) {
            const size_t wline = wins[i].w * pix;
            e = hipMemcpy2DAsync(wins[i].dst, win_stride(p, wins[i]) * tsz, dsts[i], wline, wline, wins[i].h, hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) return hip_fail("ranged windows: download", e);
        }
    }
    if ((host || p->quanta > 1) && (e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail("ranged windows: download", e);
    prof_collect();
    return 1;
}

size_t ranged_call(decsp p, const qb3x_window *wins, size_t n, bool host, hipStream_t st) {
    if (!p->rg_rd) { p->error = QB3E_EINV; return 0; }
    if (!windows_check(p, wins, n, false)) return 0;
    p->rg_bytes = p->rg_reads = 0;
    p->wins_path.assign(n, 0);
    p->win_path = 0; p->win_segs = 0;
    uint8_t *paths = p->wins_path.data();
    if (p->mode == QB3M_STORED) return stored_windows(p, wins, n, paths, host, st);
    Geometry g;
    DecPlan plan;
    IxTable ixt;
    Chunks ch;
    size_t segs = 0;
    // a family that stores halfwords or values: one device destination off its alignment and the call goes windows_device's way, which
    // applies the same test (host destinations are decoded into the handle's buffer, every window on a dword)
    const WinKernels *family = family_if_aligned(ranged_shortcut(p, g, plan, ixt, ch), g, wins, host ? 0 : n);
    if (family) {
        const int went = pieces_windows(p, g, plan, ixt, ch, wins, n, paths, &segs, host, st, *family);
        trim_cache(p);
        if (went < 0) return 0;
    }
    std::vector<qb3x_window> left;
    std::vector<size_t> which;
    for (size_t i = 0; i < n; i++) if (!paths[i]) { left.push_back(wins[i]); which.push_back(i); }
    if (left.empty()) {
        p->last_status = 0;
        p->win_path = paths[n - 1]; p->win_segs = segs;
        return n;
    }
    std::vector<uint8_t> lpaths(left.size(), 0);
    whole_container(p, left.data(), left.size(), lpaths.data(), host, st);
    size_t done = 0;
    for (size_t k = 0; k < left.size(); k++) paths[which[k]] = lpaths[k];
    for (size_t i = 0; i < n; i++) done += paths[i] != 0;
    p->win_path = paths[n - 1]; p->win_segs += segs;
    return done;
}

// qb3_read_start + qb3_read_info over the reader: the container's head chunk by chunk, a regular table stepped over (api_header.cpp)
decsp open_body(qb3x_read_fn rd, void *ctx, uint64_t size, size_t *image_size) {
    if (!rd || size < 15 || !image_size || size > (uint64_t)(~(size_t)0) / 2) return nullptr;
    std::vector<uint8_t> head, win;
    auto extend = [&](uint64_t upto) -> bool {          // the head up to this offset (or the container's end)
        upto = std::min(upto, size);
        const size_t have = head.size();
        if (upto <= have) return true;
        head.resize((size_t)upto);
        return rd(ctx, have, head.data() + have, (size_t)upto - have) == 0;
    };
    auto fetch = [&](std::vector<uint8_t> &dst, uint64_t at, size_t n) -> bool {
        dst.resize(n);
        return !n || rd(ctx, at, dst.data(), n) == 0;
    };
    if (!extend(15)) return nullptr;
    if (head[0] != 'Q' || head[1] != 'B' || head[2] != '3' || head[3] != 0x80) return nullptr;
    // the reference's chunks one by one, up to the mark or the head of the first table chunk: what qb3_read_info needs in one piece
    size_t pos = 11, tab_end = 0;
    for (int turn = 0; turn < 8; turn++) {
        if (!extend(pos + 4)) return nullptr;
        if (head.size() < pos + 4) break;
        const uint8_t c0 = head[pos], c1 = head[pos + 1];
        const size_t len = head[pos + 2] | (size_t)head[pos + 3] << 8;
        if ((c0 == 'Q' && c1 == 'V') || (c0 == 'C' && c1 == 'B') || (c0 == 'S' && c1 == 'C')) { pos += 4 + len; continue; }
        if (c0 == 'i' && c1 == 'x') {
            if (!extend(pos + IX_HEAD)) return nullptr;
            tab_end = pos + len;
        }
        break;                                          // "DT", a table, or something the parser has to judge
    }
    size_t win_off = 0;
    for (int turn = 0; turn < 3; turn++) {
        decs *p = read_start_impl(head.data(), head.size(), (size_t)size, image_size);
        if (!p) return nullptr;
        p->own_head.swap(head);                         // (the vector's buffer stays where it is: s_start stays valid)
        p->win2 = win; p->win2_off = win_off;
        if (qb3_read_info(p)) {
            p->rg_rd = rd; p->rg_ctx = ctx; p->rg_size = size;
            return p;
        }
        const size_t need = p->ix_need_off;
        head.swap(p->own_head);
        const bool was_short = p->hdr_short;
        qb3_destroy_decoder(p);
        if (!was_short) return nullptr;
        if (turn == 0 && need && need + 2 <= size) {    // a regular table: the mark behind it (and the two bytes the chunk loop reads behind a tag)
            win_off = need;
            if (!fetch(win, need, (size_t)std::min<uint64_t>(4, size - need))) return nullptr;
        } else if (turn == 0 && tab_end && tab_end + 6 <= size) {      // a table of one chunk: its pad and the mark
            win_off = tab_end;
            if (!fetch(win, tab_end, (size_t)std::min<uint64_t>(8, size - tab_end))) return nullptr;
        } else if (turn <= 1) {                         // something else: the whole head, as far as a table can reach
            const uint64_t bound = std::min<uint64_t>(size, qb3x_header_size_bound(head.data(), head.size()));
            if (bound <= head.size()) return nullptr;
            win.clear(); win_off = 0;
            if (!extend(bound)) return nullptr;
        } else return nullptr;
    }
    return nullptr;
}

}  // namespace

QB3_API decsp qb3x_open_ranged(qb3x_read_fn rd, void *ctx, uint64_t container_size, size_t *image_size) {
    return abi_guard<decsp>(nullptr, [&] { return open_body(rd, ctx, container_size, image_size); });
}
QB3_API size_t qb3x_read_windows_ranged(decsp p, const qb3x_window *wins, size_t n) {
    if (!p) return 0;
    return abi_guard<size_t>(0, [&]() -> size_t { return ranged_call(p, wins, n, true, nullptr); });
}
QB3_API size_t qb3x_decode_windows_ranged(decsp p, const qb3x_window *wins, size_t n, void *stream) {
    if (!p) return 0;
    return abi_guard<size_t>(0, [&]() -> size_t { return ranged_call(p, wins, n, false, (hipStream_t)stream); });
}
QB3_API uint64_t qb3x_ranged_bytes(const decsp p) { return p ? p->rg_bytes : 0; }
QB3_API uint64_t qb3x_ranged_reads(const decsp p) { return p ? p->rg_reads : 0; }
QB3_API void qb3x_set_ranged_gap(decsp p, size_t bytes) { if (p) p->rg_gap = bytes; }
QB3_API void qb3x_set_ranged_cache(decsp p, size_t bytes) {
    if (!p) return;
    p->rg_cache_cap = bytes;
    abi_guard<int>(0, [&] { trim_cache(p); return 0; });
}
QB3_API size_t qb3x_ranged_table_ranges(const decsp p, const qb3x_window *wins, size_t n, qb3x_range *out, size_t cap) {
    if (!p || !p->rg_rd || p->stage != 2 || !wins || !n) return 0;
    return abi_guard<size_t>(0, [&]() -> size_t {
        for (size_t i = 0; i < n; i++) {
            const qb3x_window &w = wins[i];
            if (!window_inside(p, w.x0, w.y0, w.w, w.h)) return 0;
        }
        Geometry g;
        DecPlan plan;
        IxTable ixt;
        Chunks ch;
        if (!ranged_shortcut(p, g, plan, ixt, ch)) return 0;
        std::vector<uint32_t> chunks;
        window_chunk_list(g, ch.K, ch.N, window_rects(wins, n).data(), n, chunks);
        for (size_t i = 0; out && i < chunks.size() && i < cap; i++) out[i] = qb3x_range{ ch.at(chunks[i]), ch.size(chunks[i]) };
        return chunks.size();
    });
}
