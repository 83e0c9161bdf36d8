// qb3_amd/csrc/qb3_win_best_unit.h -- the wave's work of the window kernels of the common-factor rasters that decode a lane per unit and of
// one-band 16/32/64-bit common-factor rasters (k_dec_win_best_unit.hip): a segment decoded from its table entry as dec_pxu_best_kernel's BL
// branch decodes it (k_dec_pxu.hip: lane = block * bands + band; with one band that is dec_pxw_best_kernel's lane per block, whose entry
// has the same layout), its blocks clipped to the window and stored from the wave's LDS tile.  The frame -- mapping, de-duplication,
// staging, status -- is winu_decode_wave's (qb3_win_unit.h), the units are pxu_best_units' (qb3_pxu.h), the stores winu_store_tile's.
#pragma once
#include "qb3_win_unit.h"

namespace qb3dev {

// Wave `wid` of window w (wave: its number in the workgroup of four; both wave uniform).  status: the word this window's failures go to.
// smem: the launch's dynamic LDS: pxu_wave_bytes a wave, sized for the WORST-CASE segment (a.in_cap_dw = the plan's px_cap_dw): a segment
// that does not fit is not this stream's (status bit 3).  The common-factor parser reads no code table, so nothing is shared between the
// waves and there is no workgroup barrier: a wave without a segment leaves at once.  T: the value as an unsigned number; the curve, the
// band count and the band map are run-time values.  Every unit of the segment is parsed, whether the window holds its block or not: a
// lane's entering value and factor come from the lanes below it.
template <typename T, class SRC = WinSrcContig, bool SEL = false>
__device__ __forceinline__ void winu_best_decode_wave(const DecArgs &a, const WinDesc &w, uint32_t *status, uint8_t *smem, uint32_t wave, uint32_t wid, SRC src = SRC()) {
    constexpr uint32_t UB = UBits<T>::v, UMASK = (1u << UB) - 1;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t NB = a.g.seg_blocks, nbx = a.g.nbx, B = a.g.bands;         // NB * B <= 64
    uint8_t *wmem = smem + (size_t)wave * pxu_wave_bytes(a.in_cap_dw, (uint32_t)sizeof(T));
    uint32_t *stage = (uint32_t *)wmem;
    // the wave's segment: k-th of block row by0 + r, unless the row has no such segment or a row above has it already
    const uint32_t r = wid / w.per_row, k = wid - r * w.per_row;
    const uint32_t row0 = (w.by0 + r) * nbx;           // (nblocks < 2^31)
    const uint32_t seg = (row0 + w.bx0) / NB + k;
    bool live = wid < w.nwaves && seg <= (row0 + w.bx1) / NB;
    if (r > 0 && seg <= (row0 - nbx + w.bx1) / NB) live = false;
    const bool placed = src.find(live ? seg : 0, live);
    if (!live) return;
    if (!placed) {                                      // a segment the source does not hold
        if (lane == 0) atomicOr(status, 8u);
        return;
    }
    const uint32_t g0 = seg * NB, nblocks = (uint32_t)a.g.nblocks;
    const uint32_t nb_here = (nblocks - g0 < NB) ? nblocks - g0 : NB;
    const uint32_t blk = fastdiv(lane, B, a.magic_bands), c = lane - blk * B;
    const bool act = blk < nb_here;
    // the entry: position, a rung byte, the entering value and the factor in force per band, three bytes per unit in lane order (the
    // unit's bits | the rung it is entered with << 12; the rung bytes repeat the first units' fields, the fields are what is used)
    uint64_t P0, P1;
    uint32_t bt = 0;                                    // the unit's bits | entering rung << 16
    T pv0 = 0, cf0 = 0;
    {
        const uint8_t *e = src.entry(a, seg);
        P0 = pxu_le<T>(e, 6);
        P1 = ((uint64_t)seg + 1 < a.g.nseg) ? pxu_le<T>(src.entry(a, seg + 1), 6) : a.in_bits;
        if (act) {
            pv0 = (T)pxu_le<T>(e + 6 + B + c * sizeof(T), sizeof(T));
            cf0 = (T)pxu_le<T>(e + 6 + B + (B + c) * sizeof(T), sizeof(T));
            const uint8_t *fp = e + 6 + B * (1 + 2 * sizeof(T)) + IX_BL_BEST_BYTES * lane;
            const uint32_t fld = (uint32_t)fp[0] | (uint32_t)fp[1] << 8 | (uint32_t)fp[2] << 16;
            bt = (fld & 0xfffu) | ((fld >> 12) & UMASK) << 16;
        }
    }
    // the segment's words from the word its first bit is in, through the source: no word outside [w0, w0 + ndw) is read, whatever the
    // entries say, and none at or behind the container's end; PXU_PAD zero words follow (a unit is parsed from a position inside the
    // staged bits and is at most max_unit_bits long)
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

    const uint32_t cpos = (uint32_t)(a.in_bit0 + P0 - 32 * w0);
    bool bad = !fits;
    T run[16];
    const uint32_t binc = pxu_best_units<T>(stage, ndw, cpos, bt, cf0, act, blk, c, B, nb_here, run, bad);
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

// the launch's LDS: four waves' worst-case staging (or, where that is larger, their tiles); no code table
inline size_t window_best_unit_lds_bytes(const Geometry &g, const DecPlan &plan) { return 4 * (size_t)pxu_wave_bytes(plan.px_cap_dw, g.tsz); }

// The family's instantiations (k_dec_win_best_unit.hip), by the raster's value size
template <typename T>
struct WinCfu {
    static constexpr int waves = 0;
    static constexpr auto contig = &winu_best_decode_wave<T, WinSrcContig>;
    static constexpr auto pieces = &winu_best_decode_wave<T, WinSrcPieces>;
};
// ... and their band-selected variants (winu_store_tile's SEL): the batch form only
template <typename T>
struct WinCfuSel {
    static constexpr int waves = 0;
    static constexpr auto contig = &winu_best_decode_wave<T, WinSrcContig, true>;
};
template <bool SEL = false, class Visit>
inline void win_cfu_pick(const Geometry &g, const DecPlan &, Visit visit) {
    auto go = [&](auto t) {
        typedef decltype(t) T;
        if constexpr (SEL) visit(WinCfuSel<T>()); else visit(WinCfu<T>());
    };
    switch (g.tsz) {
    case 1: go(uint8_t()); break;
    case 2: go(uint16_t()); break;
    case 4: go(uint32_t()); break;
    default: go(uint64_t()); break;
    }
}

}  // namespace qb3dev
