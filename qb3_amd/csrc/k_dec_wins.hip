// qb3_amd/csrc/k_dec_wins.hip -- a batch of windows of one raster in ONE launch: the single kernel's work (qb3_win.h, k_dec_win.hip) for
// many rectangles at once.  A tile server asks for tens of small windows of a raster it keeps in device memory; each is a hundred
// waves or so, far from filling the device, and each single call pays a launch, a status word and a wait.
//   * DESCRIPTORS  What the single kernel takes as arguments about its window (WinDesc) sits in an array in device memory, one
//     entry a window, with the exclusive prefix of the windows' wave counts.  Wave g of the launch finds its window by a binary
//     search for the last entry whose prefix is not above g; g and the search are wave uniform, the entry is read with scalar
//     loads, and from there on the wave is wave g - prefix of that window: mapping, de-duplication, clipping and stores are
//     the wave routine's.
//   * TRUST  The host merges the ranges of table chunks the windows read entries from into a sorted list without duplicates (the
//     table's last chunk is always in it); the launch's first workgroups check one chunk of the list each, one more compares the
//     table's last entry with the stream's length.  Their failures go to a call-wide status word: the table is then not this
//     stream's, for any window.
//   * STATUS  A word per window: a wave raises bits in the word of its window only, so one bad segment costs the windows that hold
//     it the shortcut and leaves the others alone.
// Here too, because this file is the one every window call links: the 8-bit family's record, the choice of the family and the three
// launchers every family goes through.
#include <string>
#include "qb3_win.h"

namespace qb3dev {

void win_u8_batch(const Geometry &g, const DecPlan &plan, const WinBatchArgs &ba, const WinLaunch &l) {
    win_u8_pick(g, plan, [&](auto f) { win_launch(f, ba, l); });
}
// 8-bit grey / RGB / RGBA rasters, FTL / BASE: dec_px_kernel's BL branch a segment, byte and dword stores to any address
const WinKernels &win_u8() {      // (in a function: host data, not for the device side of this file)
    static const WinKernels k = { decode_window_ok, 0, window_align_any, nullptr, window_lds_px, "", "dec_window", "dec_window_ranged", win_u8_one, win_u8_batch, win_u8_ranged,
                                  nullptr, win_u8_mosaic, "dec_window_mosaic" };
    return k;
}

const WinKernels *window_family(const Geometry &g, const DecPlan &plan, const IxTable &ix, unsigned mask) {
    for (const WinKernels *k : { &win_u8(), &win_u16(), &win_cf8(), &win_unit(), &win_cfu() })
        if ((!k->bit || (mask & k->bit)) && k->ok(g, plan, ix)) return k;
    return nullptr;
}

void window_chunk_list(const Geometry &g, uint32_t K, uint32_t per_chunk, const WinRect *rects, size_t n, std::vector<uint32_t> &chunks) {
    chunks.clear();
    for (size_t i = 0; i < n; i++) {
        uint32_t c0, c1;
        window_chunk_range(g, window_blocks(g, rects[i].x0, rects[i].y0, rects[i].w, rects[i].h), K, per_chunk, &c0, &c1);
        for (uint32_t c = c0; c <= c1; c++) chunks.push_back(c);
    }
    chunks.push_back((K - 1) / per_chunk);              // the tail check reads the table's last entry
    std::sort(chunks.begin(), chunks.end());
    chunks.erase(std::unique(chunks.begin(), chunks.end()), chunks.end());
}

size_t window_batch_plan(const Geometry &g, const IxTable &ix, const WinRect *rects, void *const *dsts, size_t n, void *descs,
                         std::vector<uint32_t> &chunks, uint64_t *segments) {
    WinDesc *d = (WinDesc *)descs;
    uint64_t waves = 0, segs = 0;
    for (size_t i = 0; i < n; i++) {
        window_desc(g, rects[i], dsts[i], &d[i]);
        // a launch ends in front of the window that would take it beyond WIN_LAUNCH_WAVES; the prefix starts again there
        if (waves && waves + d[i].nwaves > WIN_LAUNCH_WAVES) waves = 0;
        d[i].wave0 = (uint32_t)waves;
        waves += d[i].nwaves;
        segs += window_segments(g, rects[i]);
    }
    chunks.clear();
    if (ix.version >= 3 || ix.check_heads) window_chunk_list(g, ix.K, ix.per_chunk, rects, n, chunks);
    if (segments) *segments = segs;
    return chunks.size();
}

static int window_refused(const WinKernels &k, const char *form) {
    set_error((std::string(k.noun) + form + ": not for this raster").c_str(), 0);
    return -1;
}

int launch_decode_window(const WinKernels &k, const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                         void *dst, const WinRect &r, uint32_t *status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!k.ok(g, plan, ix) || !window_segments(g, r) || r.stride < (uint64_t)r.w * g.bands || ((uintptr_t)dst & (k.align(g) - 1)))
        return window_refused(k, "window decode");
    WinArgs wa = {};
    const uint32_t grid = window_launch_args(wa, g, plan, in32, in_bit0, in_bits, dst, r, status, ix);
    if (k.more_args) k.more_args(wa.d, plan);
    HIPCHK(hipMemsetAsync(status, 0, 4, st));
    {
        ProfScope ps(k.prof, st);
        k.one(g, plan, wa, WinLaunch{ grid, k.lds(g, plan), stream });
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_decode_windows(const WinKernels &k, const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                          const void *h_descs, const void *d_descs, size_t n, const uint32_t *d_chunks, size_t nchunks,
                          uint32_t *d_status, void *stream, const IxTable &ix, const uint8_t *sel, uint32_t nsel) {
    hipStream_t st = (hipStream_t)stream;
    if (!k.ok(g, plan, ix) || !n || (sel && (!nsel || nsel > (uint32_t)MAXBANDS || !window_sel_fused(&k, g, nsel)))) return window_refused(k, "window batch");
    WinBatchArgs ba = {};
    window_dec_args(ba.d, g, plan, in32, in_bit0, in_bits, d_status, ix);
    if (k.more_args) k.more_args(ba.d, plan);
    if (sel) window_sel_dec_args(ba.d, sel, nsel);
    ba.chunks = d_chunks;
    // in front of the first launch's waves: a workgroup for every chunk of the list and one for the tail check
    window_launches(ba, h_descs, d_descs, n, d_status, (uint32_t)nchunks + 1, [&](uint32_t grid, bool head) {
        ba.chk_n = head ? (uint32_t)nchunks : 0; ba.tail = head ? 1 : 0;
        ProfScope ps(k.prof, st);
        (sel ? k.batch_sel : k.batch)(g, plan, ba, WinLaunch{ grid, k.lds(g, plan), stream });
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_decode_windows_ranged(const WinKernels &k, const Geometry &g, const DecPlan &plan, uint32_t in_bit0, uint64_t in_bits, const void *h_descs,
                                 const void *d_descs, size_t n, const void *d_pieces, size_t npieces, const void *d_entries, const uint32_t *d_words,
                                 uint32_t *d_status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!k.ranged || !k.ok(g, plan, ix) || !n || !npieces || npieces > 0xffffffffull) return window_refused(k, "ranged window batch");
    WinRangedArgs ra = {};
    IxTable none = ix;
    none.base = nullptr;            // (the table is not in device memory)
    window_dec_args(ra.d, g, plan, nullptr, in_bit0, in_bits, d_status, none);
    if (k.more_args) k.more_args(ra.d, plan);
    ra.src.pieces = (const WinPiece *)d_pieces; ra.src.npieces = (uint32_t)npieces;
    ra.src.ents = (const uint8_t *)d_entries; ra.src.words = d_words;
    window_launches(ra, h_descs, d_descs, n, d_status, 0, [&](uint32_t grid, bool) {
        ProfScope ps(k.prof_ranged, st);
        k.ranged(g, plan, ra, WinLaunch{ grid, k.lds(g, plan), stream });
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
