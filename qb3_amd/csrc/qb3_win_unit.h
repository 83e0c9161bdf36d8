// qb3_amd/csrc/qb3_win_unit.h -- the wave's work of the window kernels of the lane-per-unit rasters and of one-band 32/64-bit rasters
// (k_dec_win_unit.hip): a segment decoded from its table entry as dec_pxu_kernel's BL branch decodes it (k_dec_pxu.hip: a lane per unit,
// lane = block * bands + band; with one band that is dec_pxw_kernel's lane per block, whose entry has the same layout), its blocks
// clipped to the window and stored from the wave's LDS tile.  Mapping, de-duplication, trust and status are win_decode_wave's
// (qb3_win.h), with the raster's own blocks per segment (64 / bands) in place of 64.
#pragma once
#include "qb3_pxu.h"
#include "qb3_win.h"

namespace qb3dev {

// Whole blocks of the wave's tile to the window: block L of the segment is described by lane L -- `off`: byte offset of its first pixel
// from the window's first byte (an edge block starts left of or above it), info: bit y: row y is the block's own and the window's,
// bit 4 + x: the same of column x, bit 8: all four columns are.  Only blocks with bit 8 are stored here, each row in pieces of N bytes.
template <int N, typename T>
__device__ __forceinline__ void winu_store_whole(uint8_t *dst, const uint8_t *tile, int64_t off, uint32_t info, uint64_t dstride, uint32_t n, uint32_t ppb,
                                                 uint32_t row_bytes, uint32_t row_pitch_bytes) {
    typedef typename PxuPiece<N>::v V;
    typedef V VU __attribute__((aligned(sizeof(T))));        // rows start at any value-aligned address
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t j0 = 0; j0 < n; j0 += 64) {               // (every lane takes every turn: the block's numbers come by a shuffle)
        const uint32_t j = j0 + lane, blk = j / ppb, part = j - blk * ppb;
        const uint32_t bi = pxu_shfl<uint32_t>(info, blk & 63u);
        const int64_t bo = (int64_t)pxu_shfl<uint64_t>((uint64_t)off, blk & 63u);
        if (j >= n || !(bi & 0x100u)) continue;
        uint8_t *p = dst + bo + (int64_t)part * N;
        const uint8_t *src = tile + (uint64_t)blk * row_bytes + (uint64_t)part * N;
#pragma unroll
        for (uint32_t y = 0; y < 4; y++)
            if ((bi >> y) & 1u) *(VU *)(p + (uint64_t)y * dstride) = *(const V *)(src + (uint64_t)y * row_pitch_bytes);
    }
}

// The wave's values to the window, once every lane holds its sixteen (o[i]: curve position i of the lane's unit, block blk of the segment,
// band c): through the wave's LDS tile at wmem, which takes the place of the staged words; g0: the segment's first block, nb_here: its
// blocks.  Whole blocks go row by row in pieces (winu_store_whole), edge blocks value by value under their column mask.  Both wave
// routines call it: winu_decode_wave below and winu_best_decode_wave (qb3_win_best_unit.h).
// SEL: a band-selected window (qb3x_decode_windows_bands_device): a pixel of the tile and of the window has a.nsel slots in place of the
// raster's bands, slot k holds band (a.sel_nibs >> 4k) & 15 (pxu_tile_fill_sel); everything behind the fill runs with the slots for B.
template <typename T, bool SEL = false>
__device__ __forceinline__ void winu_store_tile(const DecArgs &a, const WinDesc &w, uint8_t *wmem, const T (&o)[16], bool act, uint32_t blk, uint32_t c,
                                                uint32_t g0, uint32_t nb_here) {
    const uint32_t lane = threadIdx.x & 63, NB = a.g.seg_blocks, nbx = a.g.nbx, B = SEL ? a.nsel : a.g.bands;      // NB * B <= 64
    const uint32_t magic_B = SEL ? a.magic_nsel : a.magic_bands;
    // every lane holds its sixteen values in registers: the tile takes the place of the staged words
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t RP = NB * 4 * B;                     // tile elements per pixel row
    if constexpr (SEL) pxu_tile_fill_sel<T>((T *)wmem, o, act, blk, c, B, a.sel_nibs, RP, a.g.order);
    else pxu_tile_fill<T>((T *)wmem, o, act, blk, c, B, RP, a.g.order);

    // lane L describes block L of the segment: is it one of the window's, which of its rows and columns are its own (a shifted last
    // block repeats pixels of its neighbour, which holds them by the rule) and inside the window, where its first pixel goes
    uint32_t info = 0;
    int64_t off = 0;
    if (lane < nb_here) {
        const uint32_t g = g0 + lane, by = g / nbx, bx = g - by * nbx;
        if (bx >= w.bx0 && bx <= w.bx1 && by >= w.by0 && by <= w.by1) {
            const uint32_t xb = (4 * bx + 4 > a.g.w) ? a.g.w - 4 : 4 * bx;     // last column / row is shifted, not padded
            const uint32_t yb = (4 * by + 4 > a.g.h) ? a.g.h - 4 : 4 * by;
            uint32_t rows = 0, cols = 0;
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) {
                rows |= (yb + t >= 4 * by && yb + t >= w.wy0 && yb + t < w.wy1) ? 1u << t : 0u;
                cols |= (xb + t >= 4 * bx && xb + t >= w.wx0 && xb + t < w.wx1) ? 1u << t : 0u;
            }
            info = rows ? rows | cols << 4 | (cols == 15u ? 0x100u : 0u) : 0u;
            off = ((int64_t)yb - (int64_t)w.wy0) * (int64_t)w.dstride + ((int64_t)xb - (int64_t)w.wx0) * (int64_t)(B * sizeof(T));
        }
    }
    const uint32_t RB = 4 * B * (uint32_t)sizeof(T), RPB = RP * (uint32_t)sizeof(T);      // bytes of a block's row (a multiple of 4), of a tile row
    if (__any((int)(info & 0x100u))) {
        if ((RB & 15) == 0) winu_store_whole<16, T>(w.dst, wmem, off, info, w.dstride, nb_here * (RB >> 4), RB >> 4, RB, RPB);
        else if ((RB & 7) == 0) winu_store_whole<8, T>(w.dst, wmem, off, info, w.dstride, nb_here * (RB >> 3), RB >> 3, RB, RPB);
        else winu_store_whole<4, T>(w.dst, wmem, off, info, w.dstride, nb_here * (RB >> 2), RB >> 2, RB, RPB);
    }
    if (__any((int)(info && !(info & 0x100u)))) {       // edge blocks: the values of the window's columns, one by one
        const T *tile = (const T *)wmem;
        const uint32_t n = nb_here * 4 * B;
        for (uint32_t j0 = 0; j0 < n; j0 += 64) {
            const uint32_t j = j0 + lane, eb = j / (4 * B), rem = j - eb * 4 * B, x = fastdiv(rem, B, magic_B);
            const uint32_t bi = pxu_shfl<uint32_t>(info, eb & 63u);
            const int64_t bo = (int64_t)pxu_shfl<uint64_t>((uint64_t)off, eb & 63u);
            if (j >= n || (bi & 0x100u) || !((bi >> (4 + x)) & 1u)) continue;
#pragma unroll
            for (uint32_t y = 0; y < 4; y++)
                if ((bi >> y) & 1u) ((T *)(w.dst + bo + (int64_t)((uint64_t)y * w.dstride)))[rem] = tile[y * RP + j];
        }
    }
}

// Wave `wid` of window w (wave: its number in the workgroup of four; both wave uniform).  status: the word this window's failures go to.
// Every wave of the workgroup comes here (there is one workgroup barrier); smem: the launch's dynamic LDS: the 2 KB code table, then
// pxu_wave_bytes a wave, sized for the WORST-CASE segment (a.in_cap_dw = the plan's px_cap_dw): a segment that does not fit is not this
// stream's (status bit 3).  T: the value as an unsigned number; the curve, the band count and the band map are run-time values.
template <typename T, bool STEP, class SRC = WinSrcContig, bool SEL = false>
__device__ __forceinline__ void winu_decode_wave(const DecArgs &a, const WinDesc &w, uint32_t *status, uint8_t *smem, uint32_t wave, uint32_t wid, SRC src = SRC()) {
    constexpr uint32_t UB = UBits<T>::v, UMASK = (1u << UB) - 1;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t NB = a.g.seg_blocks, nbx = a.g.nbx, B = a.g.bands;         // NB * B <= 64
    uint16_t *dtab = (uint16_t *)smem;                  // 2 KB
    uint8_t *wmem = smem + 2048 + (size_t)wave * pxu_wave_bytes(a.in_cap_dw, (uint32_t)sizeof(T));
    uint32_t *stage = (uint32_t *)wmem;
    // the wave's segment: k-th of block row by0 + r, unless the row has no such segment or a row above has it already
    const uint32_t r = wid / w.per_row, k = wid - r * w.per_row;
    const uint32_t row0 = (w.by0 + r) * nbx;           // (nblocks < 2^31)
    const uint32_t seg = (row0 + w.bx0) / NB + k;
    bool live = wid < w.nwaves && seg <= (row0 + w.bx1) / NB;
    if (r > 0 && seg <= (row0 - nbx + w.bx1) / NB) live = false;
    const bool placed = src.find(live ? seg : 0, live);     // (a segment the source does not hold: the wave leaves behind the barrier)
    live = live && placed;
    const uint32_t segc = live ? seg : 0;
    const uint32_t g0 = segc * NB, nblocks = (uint32_t)a.g.nblocks;
    const uint32_t nb_here = (nblocks - g0 < NB) ? nblocks - g0 : NB;
    const uint32_t blk = fastdiv(lane, B, a.magic_bands), c = lane - blk * B;
    const bool act = live && blk < nb_here;
    // the entry: position, a rung byte and the entering value per band, a twelve-bit length per unit in lane order
    uint64_t P0, P1;
    uint32_t blen = 0, rg0 = 0;
    T pv0 = 0;
    {
        const uint8_t *e = src.entry(a, segc);
        P0 = pxu_le<T>(e, 6);
        P1 = ((uint64_t)segc + 1 < a.g.nseg) ? pxu_le<T>(src.entry(a, segc + 1), 6) : a.in_bits;
        if (act) {
            rg0 = e[6 + c] & UMASK;
            pv0 = (T)pxu_le<T>(e + 6 + B + c * sizeof(T), sizeof(T));
            const uint8_t *fl = e + 6 + B * (1 + sizeof(T)) + ((IX_BL_BITS_WIDE * lane) >> 3);
            blen = (((uint32_t)fl[0] | (uint32_t)fl[1] << 8) >> ((IX_BL_BITS_WIDE * lane) & 7)) & ((1u << IX_BL_BITS_WIDE) - 1);
        }
    }
    for (uint32_t i = tid; i < 128; i += blockDim.x) ((uint4 *)dtab)[i] = ((const uint4 *)wide_dec_tab.e)[i];
    __syncthreads();                                    // the only workgroup barrier
    if (!live) {
        if (!placed && lane == 0) atomicOr(status, 8u);
        return;
    }
    // the segment's words from the word its first bit is in, through the source: no word outside [w0, w0 + ndw) is read, whatever the
    // entries say, and none at or behind the container's end; PXU_PAD zero words follow (wide_values_lds reads ahead of its position)
    const uint64_t w0 = (a.in_bit0 + P0) >> 5;
    const uint64_t endw_abs = (a.in_bit0 + a.in_bits + 31) >> 5;
    const uint64_t ndw64 = ((a.in_bit0 + P1 + 31) >> 5) - w0;
    const bool fits = ndw64 <= a.in_cap_dw && src.holds(w0, ndw64);
    const uint32_t ndw = fits ? (uint32_t)ndw64 : 0;
    for (uint32_t base = 0; base < ndw + PXU_PAD; base += 512) {    // eight loads in flight per lane, then eight LDS stores
        uint32_t sw[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = base + lane + 64 * j;
            sw[j] = i < ndw ? src.word(a, w0 + i, endw_abs) : 0u;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = base + lane + 64 * j;
            if (i < ndw + PXU_PAD) stage[i] = sw[j];
        }
    }
    // the wave reads what its own lanes staged: LDS operations of a wave execute in order, the fence is for the compiler
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const uint32_t limit = 32 * ndw;                    // no unit starts beyond the staged bits (PXU_PAD zero words follow)
    const uint32_t cpos = (uint32_t)(a.in_bit0 + P0 - 32 * w0);
    bool bad = !fits;
    const uint32_t binc = wave_iscan32(blen);           // inclusive (units follow one another in lane order): the last lane holds the bits of the segment
    uint32_t pos = cpos + binc - blen, gpos = 0;
    pos = pos < limit ? pos : limit;
    bool sig = false;
    const LdsWords sw = (LdsWords)stage;
    const uint32_t d = dec3_switch<T, LdsWords>(sw, ndw + PXU_PAD, pos, &gpos, &sig);
    if (act && sig && STEP) bad = true;                 // common-factor / index unit in a BASE stream: not handled here
    const uint32_t dd = act ? d : 0u;
    const uint32_t rung = (rg0 + pxu_exscan_band<uint32_t>(dd, B) + dd) & UMASK;
    T run[16];
    uint32_t end = 0;
    dec3_group<T, STEP, LdsWords, sizeof(T) >= 4>(sw, ndw + PXU_PAD, gpos, rung, dtab, run, &end);
    if (act && end != pos + blen) bad = true;           // the table's lengths are not this stream's
    const T usum = act ? run[15] : (T)0;
    const T pv = (T)(pv0 + pxu_exscan_band<T>(usum, B));
    T o[16];
#pragma unroll
    for (int i = 0; i < 16; i++) o[i] = (T)(run[i] + pv);
    const uint64_t nibs = pxu_band_nibbles(a);
    bool mapped = false;
    for (uint32_t j = 0; j < B; j++) mapped = mapped || ((nibs >> (4 * j)) & 15u) != j;
    if (mapped) {           // the core band back on (core bands are themselves core: their lanes hold final values)
        const uint32_t cb = (uint32_t)(nibs >> (4 * c)) & 15u, from = (lane - c + cb) & 63u;
#pragma unroll
        for (int i = 0; i < 16; i++) { const T v = pxu_shfl<T>(o[i], from); if (cb != c) o[i] = (T)(o[i] + v); }
    }
    winu_store_tile<T, SEL>(a, w, wmem, o, act, blk, c, g0, nb_here);
    if (bad) atomicOr(status, fits ? 1u : 8u);
    // a segment that reaches beyond the stream's end (a stream cut short): the whole-raster decode decides what its pixels are
    if (lane == 0 && (P1 > a.in_bits || P1 < P0)) atomicOr(status, 4u);
    if (lane == 63 && (uint64_t)seg == a.g.nseg - 1 && fits) {      // reference: more than 7 unused bits at the end is a failure
        const uint64_t used = (uint64_t)(cpos + binc) + 32 * w0 - a.in_bit0;
        if (used > a.in_bits) atomicOr(status, 4u);
        else if (a.in_bits - used > 7) atomicOr(status, 2u);
    }
}

// what the lane-per-unit routine takes besides window_dec_args
inline void window_unit_dec_args(DecArgs &a, const DecPlan &plan) {
    a.magic_bands = magic_div(a.g.bands); a.in_cap_full = plan.px_cap_dw;
}
// the launch's LDS: the code table and four waves' worst-case staging (or, where that is larger, their tiles)
inline size_t window_unit_lds_bytes(const Geometry &g, const DecPlan &plan) { return 2048 + 4 * (size_t)pxu_wave_bytes(plan.px_cap_dw, g.tsz); }

// The family's instantiations (k_dec_win_unit.hip), by the raster's value size and mode
template <typename T, bool STEP>
struct WinUnit {
    static constexpr int waves = 0;
    static constexpr auto contig = &winu_decode_wave<T, STEP, WinSrcContig>;
    static constexpr auto pieces = &winu_decode_wave<T, STEP, WinSrcPieces>;
};
// ... and their band-selected variants: the batch form only (a.sel_nibs, a.nsel and a.magic_nsel are set)
template <typename T, bool STEP>
struct WinUnitSel {
    static constexpr int waves = 0;
    static constexpr auto contig = &winu_decode_wave<T, STEP, WinSrcContig, true>;
};
template <bool SEL = false, class Visit>
inline void win_unit_pick(const Geometry &g, const DecPlan &, Visit visit) {
    const bool step = g.mode != CM_FTL;
    auto go = [&](auto t) {
        typedef decltype(t) T;
        if constexpr (SEL) { if (step) visit(WinUnitSel<T, true>()); else visit(WinUnitSel<T, false>()); }
        else if (step) visit(WinUnit<T, true>());
        else visit(WinUnit<T, false>());
    };
    switch (g.tsz) {
    case 1: go(uint8_t()); break;
    case 2: go(uint16_t()); break;
    case 4: go(uint32_t()); break;
    default: go(uint64_t()); break;
    }
}

}  // namespace qb3dev
