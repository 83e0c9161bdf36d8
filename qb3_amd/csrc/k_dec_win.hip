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

template <int B, bool RGB, uint64_t ORDER, bool STEP>
__global__ void __launch_bounds__(256) dec_win_kernel(const WinArgs wa) {
    const DecArgs &a = wa.d;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (blockIdx.x < wa.chk_n) {                        // the launch's first workgroups: a chunk of the container's table each
        ix_check_chunk(a, wa.chk0 + blockIdx.x, (uint32_t *)smem);
        return;
    }
    if (blockIdx.x == wa.chk_n) {                       // ... and one for the table's end
        if (wa.tail_chunk) ix_check_chunk(a, (a.ix_K - 1) / a.ix_per_chunk, (uint32_t *)smem);
        if (threadIdx.x == 0) ix_tail_check(a);
        return;
    }
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // (wave uniform: what follows from it stays in scalar registers)
    win_decode_wave<B, RGB, ORDER, STEP>(a, wa.w, a.status, smem, wave, (blockIdx.x - wa.chk_n - 1) * 4 + wave);
}

uint64_t window_segments(const Geometry &g, const WinRect &r) {
    if (!g.seg_blocks || !r.w || !r.h || (uint64_t)r.x0 + r.w > g.w || (uint64_t)r.y0 + r.h > g.h) return 0;
    WinDesc d;
    window_desc(g, r, nullptr, &d);
    const uint32_t bx0 = d.bx0, bx1 = d.bx1, by0 = d.by0, by1 = d.by1;
    // both ends of a row's range of segments grow with the row: what a row adds lies behind the last segment of the row above
    uint64_t n = 0, next = 0;
    for (uint64_t by = by0; by <= by1; by++) {
        const uint64_t s0 = (by * g.nbx + bx0) / g.seg_blocks, s1 = (by * g.nbx + bx1) / g.seg_blocks;
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
    // table chunks an entry is read from: the first segment's to the one of the entry behind the last segment
    const uint64_t first = ((uint64_t)wa.w.by0 * g.nbx + wa.w.bx0) / g.seg_blocks, last = std::min<uint64_t>(((uint64_t)wa.w.by1 * g.nbx + wa.w.bx1) / g.seg_blocks + 1, ix.K - 1);
    wa.chk0 = (uint32_t)(first / ix.per_chunk);
    const bool checked = a.ix_ver >= 3 || a.ix_check_heads;
    wa.chk_n = checked ? (uint32_t)(last / ix.per_chunk) - wa.chk0 + 1 : 0;
    wa.tail_chunk = checked && (ix.K - 1) / ix.per_chunk > last / ix.per_chunk;
    return wa.chk_n + 1 + (wa.w.nwaves + 3) / 4;
}

template <int B, bool RGB>
static void launch_dec_win_b(const WinArgs &wa, dim3 grid, size_t lds, hipStream_t st) {
    const bool step = wa.d.g.mode != CM_FTL, z = wa.d.g.order == ZCURVE;
    const dim3 block(256);
    if (!z && !step) hipLaunchKernelGGL((dec_win_kernel<B, RGB, HILBERT, false>), grid, block, lds, st, wa);
    else if (!z && step) hipLaunchKernelGGL((dec_win_kernel<B, RGB, HILBERT, true>), grid, block, lds, st, wa);
    else if (z && !step) hipLaunchKernelGGL((dec_win_kernel<B, RGB, ZCURVE, false>), grid, block, lds, st, wa);
    else hipLaunchKernelGGL((dec_win_kernel<B, RGB, ZCURVE, true>), grid, block, lds, st, wa);
}

int launch_decode_window(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                         void *dst, const WinRect &r, uint32_t *status, void *stream, const IxTable &ix) {
    hipStream_t st = (hipStream_t)stream;
    if (!decode_window_ok(g, plan, ix) || !window_segments(g, r) || r.stride < (uint64_t)r.w * g.bands) { set_error("window decode: not for this raster", 0); return -1; }
    WinArgs wa = {};
    const dim3 grid(window_launch_args(wa, g, plan, in32, in_bit0, in_bits, dst, r, status, ix));
    HIPCHK(hipMemsetAsync(status, 0, 4, st));
    {
        ProfScope ps("dec_window", st);
        if (g.bands == 1) launch_dec_win_b<1, false>(wa, grid, plan.lds_px, st);
        else if (g.bands == 3) { if (plan.px_rgb) launch_dec_win_b<3, true>(wa, grid, plan.lds_px, st); else launch_dec_win_b<3, false>(wa, grid, plan.lds_px, st); }
        else { if (plan.px_rgb) launch_dec_win_b<4, true>(wa, grid, plan.lds_px, st); else launch_dec_win_b<4, false>(wa, grid, plan.lds_px, st); }
    }
    HIPCHK(hipGetLastError());
    return 0;
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
