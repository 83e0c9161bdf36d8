// qb3_amd/csrc/k_dec_win.hip -- window decode of 8-bit grey / RGB / RGBA rasters from the container's level-2 restart table:
// only the index segments that hold a block of the window are decoded, and only the window's bytes are written.
//
// The decoding itself is dec_px_kernel's BL branch (k_dec_px.hip): a wave per segment, a lane per block, the segment in registers
// -- the value entering a block is a wave scan over its segment, so a segment is the smallest unit that can be decoded alone.
// What is new is which segments run and where the pixels go:
//   * MAPPING  Block row `by` of the window needs the segments (by * nbx + bx0) / 64 .. (by * nbx + bx1) / 64.  The launch has
//     `per_row` waves for each of the window's block rows (per_row: the most segments a row's run of blocks can touch); wave
//     (r, k) takes segment s0(by0 + r) + k and leaves when that is behind the row's last one.  Segments wrap around block rows
//     whenever nbx % 64 != 0, so a segment may be reached from two (nbx < 64: several) block rows: it is DEDUPLICATED
//     arithmetically -- a wave also leaves when its segment is not behind the last segment of the row above, which is the
//     largest any earlier row reaches (both ends of a row's range grow with the row) -- so every segment is decoded once and
//     stores the blocks of all the window's rows it holds.  Nothing about the window but eight numbers travels to the device.
//   * CLIPPING  The raster's last block column / row is shifted, not padded: pixel x is held by block min(x / 4, nbx - 1).  A
//     lane stores when its block is one of the window's ([bx0, bx1] x [by0, by1] by that rule), clipped with the block's real
//     pixel origin to the window and to the pixels it holds by the rule, at window coordinates.  A block wholly inside the window's columns keeps the dword stores
//     (v_alignbit for rows that are not dword aligned); an edge block stores byte by byte under a mask.  No byte outside the
//     window's rows is written and none is read back: another stream may own the neighbours.
//   * TRUST  The launch's first workgroups check the table chunks from which an entry is read (ix_check_chunk: heads and 16-bit
//     checks) -- those between the chunk of the first segment's entry and the chunk of the entry behind the last segment, whose
//     position ends it.  A chunk holds about 700 entries, more than two block rows of the widest raster, so every chunk in that
//     range holds an entry the window uses.  Every consistency test of dec_px_kernel stays, and a segment that reaches beyond
//     the stream's end raises status bit 2: the host takes ANY nonzero status as "decode the whole raster and crop".
//     One more workgroup looks at the table's LAST entry (checking its chunk when the window's range does not hold it): a stream
//     that ends before its last segment starts was cut short, and what the whole decode makes of such a stream -- zeros behind
//     the end, or a failure -- is for the whole decode to say, also for a window in front of the cut.
#include "qb3_win.h"

namespace qb3dev {

// ... for the strip of block rows of a window call (path 2), whose launch has checked the whole table: one lane
__global__ void ix_tail_kernel(const DecArgs a) { if (threadIdx.x == 0) ix_tail_check(a); }

uint64_t window_segments(const Geometry &g, const WinRect &r) {
    if (!g.seg_blocks || !r.w || !r.h || (uint64_t)r.x0 + r.w > g.w || (uint64_t)r.y0 + r.h > g.h) return 0;
    const WinBlocks b = window_blocks(g, r.x0, r.y0, r.w, r.h);
    // both ends of a row's range of segments grow with the row: what a row adds lies behind the last segment of the row above
    uint64_t n = 0, next = 0;
    for (uint64_t by = b.by0; by <= b.by1; by++) {
        const uint64_t s0 = (by * g.nbx + b.bx0) / g.seg_blocks, s1 = (by * g.nbx + b.bx1) / g.seg_blocks;
        const uint64_t lo = std::max(s0, next);
        if (s1 >= lo) { n += s1 - lo + 1; next = s1 + 1; }
    }
    return n;
}

bool decode_window_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    return decode_strips_ok(g, plan, ix) && aligned_dec_kernel(g, plan) == DecKernel::px && g.seg_blocks == 64 && g.nblocks < (1ull << 31);
}

void window_dec_args(DecArgs &a, const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                     uint32_t *status, const IxTable &ix) {
    a.g = g; a.in32 = in32; a.in_bit0 = in_bit0; a.in_bits = in_bits; a.status = status;
    a.in_cap_dw = plan.px_cap_dw;
    a.ix = ix.base; a.ix_K = ix.K; a.ix_blocks = ix.blocks; a.ix_E = ix.entry_bytes; a.ix_per_chunk = ix.per_chunk;
    a.ix_pad = ix.pads ? IX_PAD : 0; a.ix_bl = 1; a.bl_mode = 1;
    a.ix_ver = ix.version; a.ix_check_heads = ix.check_heads ? 1u : 0u;
    a.ntiles = 1; a.seg0 = 0; a.seg_end = g.nseg;
}

uint32_t window_launch_args(WinArgs &wa, const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                            void *dst, const WinRect &r, uint32_t *status, const IxTable &ix) {
    DecArgs &a = wa.d;
    window_dec_args(a, g, plan, in32, in_bit0, in_bits, status, ix);
    window_desc(g, r, dst, &wa.w);
    uint32_t c0, c1;
    window_chunk_range(g, WinBlocks{ wa.w.bx0, wa.w.bx1, wa.w.by0, wa.w.by1 }, ix.K, ix.per_chunk, &c0, &c1);
    wa.chk0 = c0;
    const bool checked = a.ix_ver >= 3 || a.ix_check_heads;
    wa.chk_n = checked ? c1 - c0 + 1 : 0;
    wa.tail_chunk = checked && (ix.K - 1) / ix.per_chunk > c1;
    return wa.chk_n + 1 + (wa.w.nwaves + 3) / 4;
}

void win_u8_one(const Geometry &g, const DecPlan &plan, const WinArgs &wa, const WinLaunch &l) {
    win_u8_pick(g, plan, [&](auto f) { win_launch(f, wa, l); });
}

int launch_window_tail_check(const Geometry &g, uint64_t in_bits, uint32_t *status, void *stream, const IxTable &ix) {
    if (!ix.base || !ix.K || !ix.per_chunk) return 0;
    DecArgs a = {};
    a.g = g; a.in_bits = in_bits; a.status = status;
    a.ix = ix.base; a.ix_K = ix.K; a.ix_E = ix.entry_bytes; a.ix_per_chunk = ix.per_chunk; a.ix_pad = ix.pads ? IX_PAD : 0;
    hipLaunchKernelGGL(ix_tail_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
