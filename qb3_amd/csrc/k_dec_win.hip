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
#include "qb3_px.h"

namespace qb3dev {

struct WinArgs {
    DecArgs d;                      // stream, table, status word, staging capacity: as dec_px_kernel takes them
    uint8_t *dst;                   // the window's first byte
    uint64_t dstride;               // bytes between the window's rows
    uint32_t wx0, wy0, wx1, wy1;    // the window in raster pixels: [wx0, wx1) x [wy0, wy1)
    uint32_t bx0, bx1, by0, by1;    // ... in blocks, both ends included
    uint32_t per_row, nwaves;       // waves per block row of the window; rows * per_row
    uint32_t chk0, chk_n;           // table chunks the launch's first chk_n workgroups check, from chunk chk0
    uint32_t tail_chunk;            // the workgroup behind them checks the table's last chunk too (it is not one of those)
};

// position of the table's last entry against the stream's length: a stream that ends before its last segment starts was cut short
__device__ __forceinline__ void ix_tail_check(const DecArgs &a) {
    const uint8_t *e = ix_entry_at(a.ix, a.ix_per_chunk, a.ix_E, a.ix_pad, a.ix_K - 1);
    uint64_t v = 0;
#pragma unroll
    for (uint32_t i = 0; i < 6; i++) v |= (uint64_t)e[i] << (8 * i);
    if (v > a.in_bits) atomicOr(a.status, 4u);
}
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
    constexpr int NW = (B + 1) / 2;                     // 32-bit words of a scan packed 16 bits per band
    constexpr uint32_t NB = 64;                         // blocks of a segment
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));    // (wave uniform: what follows from it stays in scalar registers)
    const uint32_t nbx = a.g.nbx;

    uint32_t *tab = (uint32_t *)smem;                   // 4 KB, at LDS address 0 (the table addressing relies on it)
    uint32_t *stage = tab + 1024 + wave * (a.in_cap_dw + 8);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)smem;
    const uint32_t stage_bit0 = 8 * (lds0 + (uint32_t)((uint8_t *)stage - smem));
    // the wave's segment: k-th of block row by0 + r, unless the row has no such segment or a row above has it already
    const uint32_t wid = (blockIdx.x - wa.chk_n - 1) * 4 + wave;
    const uint32_t r = wid / wa.per_row, k = wid - r * wa.per_row;
    const uint32_t row0 = (wa.by0 + r) * nbx;           // (nblocks <= 2^28)
    const uint32_t seg = (row0 + wa.bx0) / NB + k;
    bool live = wid < wa.nwaves && seg <= (row0 + wa.bx1) / NB;
    if (r > 0 && seg <= (row0 - nbx + wa.bx1) / NB) live = false;
    const uint32_t segc = live ? seg : 0;
    const uint32_t g0 = segc * NB, nblocks = (uint32_t)a.g.nblocks;
    const uint32_t nb_here = (nblocks - g0 < NB) ? nblocks - g0 : NB;
    const bool act = live && lane < nb_here;
    uint64_t P0, P1;
    uint32_t rg0[B], pv0[B], blen = 0;
    {
        const uint8_t *e = ix_entry_at(a.ix, a.ix_per_chunk, a.ix_E, a.ix_pad, segc);
        auto pos6 = [](const uint8_t *q) { uint64_t v = 0;
#pragma unroll
            for (uint32_t i = 0; i < 6; i++) v |= (uint64_t)q[i] << (8 * i);
            return v; };
        P0 = pos6(e);
        P1 = ((uint64_t)segc + 1 < a.g.nseg) ? pos6(ix_entry_at(a.ix, a.ix_per_chunk, a.ix_E, a.ix_pad, segc + 1)) : a.in_bits;
#pragma unroll
        for (int c = 0; c < B; c++) { rg0[c] = e[6 + c] & 7u; pv0[c] = e[6 + B + c]; }
        const uint8_t *bl = e + 6 + 2 * B + ((IX_BL_BITS * lane) >> 3);
        blen = act ? (((uint32_t)bl[0] | (uint32_t)bl[1] << 8) >> ((IX_BL_BITS * lane) & 7)) & ((1u << IX_BL_BITS) - 1) : 0u;
    }
    for (uint32_t i = tid; i < 256; i += blockDim.x) ((uint4 *)tab)[i] = ((const uint4 *)px_dec_tab.e)[i];
    __syncthreads();                                    // the only workgroup barrier
    if (!live) return;
    const uint64_t w0 = (a.in_bit0 + P0) >> 5;
    const uint64_t endw_abs = (a.in_bit0 + a.in_bits + 31) >> 5;
    const uint64_t ndw64 = ((a.in_bit0 + P1 + 31) >> 5) - w0;
    // the staging area holds the longest valid segment; a table that says otherwise is not this stream's
    const bool fits = ndw64 <= a.in_cap_dw && lds0 == 0;
    const uint32_t ndw = fits ? (uint32_t)ndw64 : 0;
    for (uint32_t base = 0; base < ndw + 8; base += 512) {          // eight loads in flight per lane, then eight LDS stores
        uint32_t sw[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = base + lane + 64 * j;
            sw[j] = (i < ndw && w0 + i < endw_abs) ? a.in32[w0 + i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = base + lane + 64 * j;
            if (i < ndw + 8) stage[i] = sw[j];
        }
    }
    // the wave reads what its own lanes staged: LDS operations of a wave execute in order, the fence is for the compiler
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const uint32_t limit = stage_bit0 + 32 * ndw;       // no unit starts beyond the staged bits (8 zero words follow)
    const uint32_t cpos = stage_bit0 + (uint32_t)(a.in_bit0 + P0 - 32 * w0);
    bool bad = !fits;
    const uint32_t binc = wave_iscan32(blen);           // inclusive: lane 63 holds the bits of the segment
    uint32_t pos = cpos + binc - blen;
    uint32_t rp[B][8], spk[NW], sinc[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) spk[j] = 0;
    // band after band: the switch, the band's rungs across the segment (a scan of the switches), the unit, and where it
    // ended is where the next band's unit starts
    const uint32_t blk_end = pos + blen;
#pragma unroll
    for (int c = 0; c < B; c++) {
        pos = pos < limit ? pos : limit;
        bool sig; uint32_t csl;
        const uint32_t d = px_switch(pos, &csl, &sig);
        if (act && sig && STEP) bad = true;             // common-factor / index unit: not handled here
        const uint32_t rung = (rg0[c] + wave_iscan32(act ? d : 0u)) & 7u;
        uint32_t end;
        const uint32_t tot = px_group<STEP>(pos + csl, rung, rp[c], &end) & 0xffu;
        spk[c >> 1] |= (act ? tot : 0u) << (16 * (c & 1));
        pos = end;
    }
    if (act && pos != blk_end) bad = true;              // the table's lengths are not this stream's
#pragma unroll
    for (int j = 0; j < NW; j++) sinc[j] = wave_iscan32(spk[j]);

    const uint32_t g = g0 + lane, by = g / nbx, bx = g - by * nbx;
    if (act && bx >= wa.bx0 && bx <= wa.bx1 && by >= wa.by0 && by <= wa.by1) {
        // entering value, then the core band (reference QB3decode.h:560-567)
#pragma unroll
        for (int c = 0; c < B; c++) {
            const uint32_t pv = pv0[c] + (((sinc[c >> 1] - spk[c >> 1]) >> (16 * (c & 1))) & 0xffffu);
#pragma unroll
            for (int j = 0; j < 8; j++) rp[c][j] = pk_add16(rp[c][j], (pv & 0xffu) * 0x00010001u);
        }
#pragma unroll
        for (int c = 0; c < B; c++) {
            const int cb = core_of<B, RGB>(c);
            if (cb != c)
#pragma unroll
                for (int j = 0; j < 8; j++) rp[c][j] = pk_add16(rp[c][j], rp[cb][j]);
        }
        // the block's real pixel origin (last column / row shifted, not padded), clipped to the window
        const uint32_t xb = (4 * bx + 4 > a.g.w) ? a.g.w - 4 : 4 * bx;
        const uint32_t yb = (4 * by + 4 > a.g.h) ? a.g.h - 4 : 4 * by;
        // (a shifted last block repeats pixels of its neighbour, which holds them by the rule: it stores its own columns / rows only,
        // so that a stream whose two copies differ -- a damaged one -- still gives every pixel one value)
        const bool whole = xb == 4 * bx && xb >= wa.wx0 && xb + 4 <= wa.wx1;     // all four columns are the block's and the window's
        uint32_t colmask = 0;                                       // bit x: column xb + x is the block's and the window's
#pragma unroll
        for (uint32_t x = 0; x < 4; x++) colmask |= (xb + x >= 4 * bx && xb + x >= wa.wx0 && xb + x < wa.wx1) ? 1u << x : 0u;
        // byte offset of the block's first row in the window (an edge block starts left of or above it: only the bytes under
        // the masks are addressed)
        const int64_t off0 = ((int64_t)yb - (int64_t)wa.wy0) * (int64_t)wa.dstride + ((int64_t)xb - (int64_t)wa.wx0) * B;
#pragma unroll
        for (int y = 0; y < 4; y++) {
            uint32_t ow[B];
#pragma unroll
            for (int j = 0; j < B; j++) {
                // byte i of output dword j is band (4j+i)%B of pixel x = (4j+i)/B: low byte of a 16-bit lane
                uint32_t half2[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int b0 = 4 * j + 2 * h, b1 = b0 + 1;
                    const int i0 = curve_pos_of(ORDER, b0 / B, y), i1 = curve_pos_of(ORDER, b1 / B, y);
                    // v_perm_b32: selector bytes 0..3 pick from the second operand, 4..7 from the first
                    half2[h] = __builtin_amdgcn_perm(rp[b1 % B][i1 >> 1], rp[b0 % B][i0 >> 1],
                                                     (uint32_t)((4 + 2 * (i1 & 1)) << 8 | (2 * (i0 & 1))));
                }
                ow[j] = __builtin_amdgcn_perm(half2[1], half2[0], 0x05040100u);
            }
            if (yb + y < 4 * by || yb + y < wa.wy0 || yb + y >= wa.wy1) continue;     // the neighbour's row, or one above or below the window
            uint8_t *row = wa.dst + (off0 + (int64_t)y * (int64_t)wa.dstride);
            if (!whole) {           // edge block: the bytes of the window's columns, one by one
#pragma unroll
                for (int i = 0; i < 4 * B; i++)
                    if ((colmask >> (i / B)) & 1u) row[i] = (uint8_t)(ow[i >> 2] >> (8 * (i & 3)));
                continue;
            }
            const uint32_t al = (uint32_t)(uintptr_t)row & 3;
            if (al == 0) {
#pragma unroll
                for (int j = 0; j < B; j++) ((uint32_t *)row)[j] = ow[j];
            } else {        // unaligned row: head bytes, the aligned dwords inside it, tail bytes -- only the row's own 4*B bytes
                const uint32_t head = 4 - al, sh = 8 * head;            // bytes before the first aligned dword
#pragma unroll
                for (uint32_t t = 0; t < 3; t++) if (t < head) row[t] = (uint8_t)(ow[0] >> (8 * t));
                uint32_t *mid = (uint32_t *)(row + head);
#pragma unroll
                for (int j = 0; j + 1 < B; j++) mid[j] = __builtin_amdgcn_alignbit(ow[j + 1], ow[j], sh);
                uint8_t *tail = row + head + 4 * (B - 1);               // the last `al` bytes
                const uint32_t last = ow[B - 1] >> sh;
#pragma unroll
                for (uint32_t t = 0; t < 3; t++) if (t < al) tail[t] = (uint8_t)(last >> (8 * t));
            }
        }
    }
    if (bad) atomicOr(a.status, fits ? 1u : 8u);
    // a segment that reaches beyond the stream's end (a stream cut short): the whole-raster decode decides what its pixels are
    if (lane == 0 && (P1 > a.in_bits || P1 < P0)) atomicOr(a.status, 4u);
    if (lane == 63 && (uint64_t)seg == a.g.nseg - 1 && fits) {      // reference: more than 7 unused bits at the end is a failure
        const uint64_t used = (uint64_t)(cpos + binc - stage_bit0) + 32 * w0 - a.in_bit0;
        if (used > a.in_bits) atomicOr(a.status, 4u);
        else if (a.in_bits - used > 7) atomicOr(a.status, 2u);
    }
}

// the window's blocks by the geometry rule: pixel x is held by block min(x / 4, nbx - 1)
static void window_blocks(const Geometry &g, const WinRect &r, uint32_t *bx0, uint32_t *bx1, uint32_t *by0, uint32_t *by1) {
    *bx0 = std::min(r.x0 / 4, g.nbx - 1); *bx1 = std::min((r.x0 + r.w - 1) / 4, g.nbx - 1);
    *by0 = std::min(r.y0 / 4, g.nby - 1); *by1 = std::min((r.y0 + r.h - 1) / 4, g.nby - 1);
}

uint64_t window_segments(const Geometry &g, const WinRect &r) {
    if (!g.seg_blocks || !r.w || !r.h || (uint64_t)r.x0 + r.w > g.w || (uint64_t)r.y0 + r.h > g.h) return 0;
    uint32_t bx0, bx1, by0, by1;
    window_blocks(g, r, &bx0, &bx1, &by0, &by1);
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
    return decode_strips_ok(g, plan, ix) && g.mode != CM_BEST && g.tsz == 1 && plan.px && g.seg_blocks == 64 &&
           (g.order == HILBERT || g.order == ZCURVE) && g.nblocks < (1ull << 31);
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
    DecArgs &a = wa.d;
    a.g = g; a.in32 = in32; a.in_bit0 = in_bit0; a.in_bits = in_bits; a.status = status;
    a.in_cap_dw = plan.px_cap_dw;
    a.ix = ix.base; a.ix_K = ix.K; a.ix_blocks = ix.blocks; a.ix_E = ix.entry_bytes; a.ix_per_chunk = ix.per_chunk;
    a.ix_pad = ix.pads ? IX_PAD : 0; a.ix_bl = 1; a.bl_mode = 1;
    a.ix_ver = ix.version; a.ix_check_heads = ix.check_heads ? 1u : 0u;
    a.ntiles = 1; a.seg0 = 0; a.seg_end = g.nseg;
    wa.dst = (uint8_t *)dst; wa.dstride = r.stride;
    wa.wx0 = r.x0; wa.wy0 = r.y0; wa.wx1 = r.x0 + r.w; wa.wy1 = r.y0 + r.h;
    window_blocks(g, r, &wa.bx0, &wa.bx1, &wa.by0, &wa.by1);
    // the most segments the run of bx1 - bx0 + 1 blocks of a row touches: it starts anywhere in a segment, unless rows start where segments do
    const uint32_t n = wa.bx1 - wa.bx0 + 1;
    wa.per_row = (g.nbx % 64 == 0) ? (wa.bx0 % 64 + n - 1) / 64 + 1 : (n + 62) / 64 + 1;
    wa.nwaves = (wa.by1 - wa.by0 + 1) * wa.per_row;
    // table chunks an entry is read from: the first segment's to the one of the entry behind the last segment
    const uint64_t first = ((uint64_t)wa.by0 * g.nbx + wa.bx0) / 64, last = std::min<uint64_t>(((uint64_t)wa.by1 * g.nbx + wa.bx1) / 64 + 1, ix.K - 1);
    wa.chk0 = (uint32_t)(first / ix.per_chunk);
    const bool checked = a.ix_ver >= 3 || a.ix_check_heads;
    wa.chk_n = checked ? (uint32_t)(last / ix.per_chunk) - wa.chk0 + 1 : 0;
    wa.tail_chunk = checked && (ix.K - 1) / ix.per_chunk > last / ix.per_chunk;
    HIPCHK(hipMemsetAsync(status, 0, 4, st));
    const dim3 grid(wa.chk_n + 1 + (wa.nwaves + 3) / 4);
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
