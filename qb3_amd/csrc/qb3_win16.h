// qb3_amd/csrc/qb3_win16.h -- the wave's work of the 16-bit window kernels (k_dec_win16.hip): a segment decoded from its table entry as
// dec_px16_kernel's BL branch decodes it (k_dec_px16.hip: a lane per block and band group, BG bands a lane), its blocks clipped to the
// window and stored as win_decode_wave (qb3_win.h) clips and stores them.  Mapping, de-duplication, trust and status are that function's,
// with the raster's own blocks per segment (64 / band groups) in place of 64.
#pragma once
#include "qb3_px16.h"
#include "qb3_win.h"

namespace qb3dev {

// Wave `wid` of window w (wave: its number in the workgroup of four; both wave uniform).  status: the word this window's failures go to.
// Every wave of the workgroup comes here (there is one workgroup barrier); smem: the launch's dynamic LDS, at LDS address 0, sized for
// the WORST-CASE segment (a.in_cap_dw = the plan's px_cap_dw): a segment that does not fit is not this stream's (status bit 3).
template <int BG, bool RGB, uint64_t ORDER, bool STEP, class SRC = WinSrcContig>
__device__ __forceinline__ void win16_decode_wave(const DecArgs &a, const WinDesc &w, uint32_t *status, uint8_t *smem, uint32_t wave, uint32_t wid, SRC src = SRC()) {
    constexpr int NW = (BG + 1) / 2;                    // 32-bit words of a scan packed 16 bits per band
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t NB = a.g.seg_blocks, nbx = a.g.nbx, B = a.g.bands, NG = a.px_ng;    // NB * NG <= 64
    const uint32_t slot = fastdiv(lane, NG, a.px_magic_ng), grp = lane - slot * NG, band0 = grp * BG;

    uint32_t *tab = (uint32_t *)smem;                   // 4 KB, at LDS address 0 (the table addressing relies on it)
    uint32_t *stage = tab + 1024 + wave * (a.in_cap_dw + 16);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)smem;
    const uint32_t stage_bit0 = 8 * (lds0 + (uint32_t)((uint8_t *)stage - smem));
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
    const bool act = live && slot < nb_here;
    uint64_t P0, P1;
    uint32_t rg0[BG], pv0[BG], blen = 0, f0 = 0, f1 = 0;
    {
        const uint8_t *e = src.entry(a, segc);
        auto pos6 = [](const uint8_t *q) { uint64_t v = 0;
#pragma unroll
            for (uint32_t i = 0; i < 6; i++) v |= (uint64_t)q[i] << (8 * i);
            return v; };
        P0 = pos6(e);
        P1 = ((uint64_t)segc + 1 < a.g.nseg) ? pos6(src.entry(a, segc + 1)) : a.in_bits;
#pragma unroll
        for (int c = 0; c < BG; c++) {
            rg0[c] = e[6 + band0 + c] & 15u;
            const uint8_t *pv = e + 6 + B + 2 * (band0 + c);
            pv0[c] = (uint32_t)pv[0] | (uint32_t)pv[1] << 8;
        }
        constexpr uint32_t FPL = BG == 1 ? 1 : 2;       // fields a lane: two (band pairs; pair and band; two bands), or the one unit of a single band
        const uint32_t bit = FPL * IX_BL_BITS * lane;
        const uint8_t *fp = e + 6 + 3 * B + (bit >> 3);
        const uint32_t v = ((uint32_t)fp[0] | (uint32_t)fp[1] << 8 | (FPL == 2 ? (uint32_t)fp[2] << 16 : 0u)) >> (bit & 7);
        f0 = act ? v & ((1u << IX_BL_BITS) - 1) : 0u;
        f1 = act && FPL == 2 ? (v >> IX_BL_BITS) & ((1u << IX_BL_BITS) - 1) : 0u;
        blen = f0 + f1;
    }
    for (uint32_t i = tid; i < 256; i += blockDim.x) ((uint4 *)tab)[i] = ((const uint4 *)px_dec_tab.e)[i];
    __syncthreads();                                    // the only workgroup barrier
    if (!live) {
        if (!placed && lane == 0) atomicOr(status, 8u);
        return;
    }
    // the segment's words from the word its first bit is in, through the source: no word outside [w0, w0 + ndw) is read, whatever the
    // entries say, and none at or behind the container's end; 16 zero words follow (px16_groups_hi reads ahead of the unit it decodes)
    const uint64_t w0 = (a.in_bit0 + P0) >> 5;
    const uint64_t endw_abs = (a.in_bit0 + a.in_bits + 31) >> 5;
    const uint64_t ndw64 = ((a.in_bit0 + P1 + 31) >> 5) - w0;
    const bool fits = ndw64 <= a.in_cap_dw && lds0 == 0 && src.holds(w0, ndw64);
    const uint32_t ndw = fits ? (uint32_t)ndw64 : 0;
    for (uint32_t base = 0; base < ndw + 16; base += 512) {         // eight loads in flight per lane, then eight LDS stores
        uint32_t sw[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = base + lane + 64 * j;
            sw[j] = i < ndw ? src.word(a, w0 + i, endw_abs) : 0u;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = base + lane + 64 * j;
            if (i < ndw + 16) stage[i] = sw[j];
        }
    }
    // the wave reads what its own lanes staged: LDS operations of a wave execute in order, the fence is for the compiler
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const uint32_t limit = stage_bit0 + 32 * ndw;       // no unit starts beyond the staged bits (16 zero words follow)
    const uint32_t cpos = stage_bit0 + (uint32_t)(a.in_bit0 + P0 - 32 * w0);
    bool bad = !fits;
    const uint32_t binc = wave_iscan32(blen);           // lanes are in stream order
    uint32_t gpos[BG], pos = cpos + binc - blen;
    uint32_t rp[BG][8], spk[NW], sinc[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) spk[j] = 0;
    // the lane's units, as dec_px16_kernel's BL branch: the fields give the starts (a position the table made up is clamped to what was staged)
    uint32_t rungs[BG], tots[BG], ends[BG];
#pragma unroll
    for (int c = 0; c < BG; c++) { rungs[c] = 0; tots[c] = 0; ends[c] = 0; }
    const uint32_t lane0 = pos;
    auto round = [&](auto nc, auto rsc, auto c0c, uint32_t s0, uint32_t s1) {
        constexpr int N = decltype(nc)::value, RS = decltype(rsc)::value, C0 = decltype(c0c)::value;
        const uint32_t st[2] = { s0, s1 };
        uint32_t dd = 0;
#pragma unroll
        for (int h = 0; h < N; h++) {
            const int c = C0 + h * RS;
            uint32_t p0 = st[h];
            p0 = p0 < limit ? p0 : limit;
            bool sig; uint32_t csl;
            const uint32_t d = px16_switch(p0, &csl, &sig);
            gpos[c] = p0 + csl;
            if (act && sig && STEP) bad = true;         // common-factor / index unit: not handled here
            dd |= (act ? d : 0u) << (16 * h);
        }
        uint32_t dsc[1] = { dd };
        group_iscan<1>(dsc, NG);                        // inclusive, the bands' rung changes 16 bits each
        bool lane_hi = false, lane_lo = false;
#pragma unroll
        for (int h = 0; h < N; h++) {
            const int c = C0 + h * RS;
            rungs[c] = (rg0[c] + ((dsc[0] >> (16 * h)) & 0xffffu)) & 15u;
            lane_hi = lane_hi || rungs[c] >= 8; lane_lo = lane_lo || rungs[c] < 8;
        }
        if (__any(lane_hi)) px16_groups_hi<STEP, N, RS>(&gpos[C0], &rungs[C0], &rp[C0], &tots[C0], &ends[C0]);
        if (__any(lane_lo)) {
#pragma unroll
            for (int h = 0; h < N; h++) {
                const int c = C0 + h * RS;
                if (rungs[c] < 8) tots[c] = px_group<STEP>(gpos[c], rungs[c], rp[c], &ends[c]);
            }
        }
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
    bool ok;
    if constexpr (BG == 4) {            // the pairs (0,1) and (2,3): bands 0 and 2 in lockstep, then 1 and 3 from where those ended
        round(I2(), I2(), I0(), pos, pos + f0);
        round(I2(), I2(), I1(), ends[0], ends[2]);
        ok = ends[1] == lane0 + f0 && ends[3] == lane0 + f0 + f1;
    } else if constexpr (BG == 3) {     // (0,1) and band 2: bands 0 and 2, then band 1
        round(I2(), I2(), I0(), pos, pos + f0);
        round(I1(), I1(), I1(), ends[0], 0u);
        ok = ends[1] == lane0 + f0 && ends[2] == lane0 + f0 + f1;
    } else if constexpr (BG == 2) {     // a field per band, one round
        round(I2(), I1(), I0(), pos, pos + f0);
        ok = ends[0] == lane0 + f0 && ends[1] == lane0 + f0 + f1;
    } else {                            // a single band: the lane's unit starts where the scan of the lengths says
        round(I1(), I1(), I0(), pos, 0u);
        ok = ends[0] == lane0 + f0;
    }
    if (act && !ok) bad = true;                         // the table's lengths are not this stream's
#pragma unroll
    for (int c = 0; c < BG; c++) spk[c >> 1] |= (act ? tots[c] & 0xffffu : 0u) << (16 * (c & 1));
    {   // per-band scan of the unit totals modulo 2^16: the two halves of a word must not carry into each other
        uint32_t lo[NW], hi[NW];
#pragma unroll
        for (int j = 0; j < NW; j++) { lo[j] = spk[j] & 0xffffu; hi[j] = spk[j] >> 16; }
        group_iscan<NW>(lo, NG);
        group_iscan<NW>(hi, NG);
#pragma unroll
        for (int j = 0; j < NW; j++) sinc[j] = (lo[j] & 0xffffu) | (hi[j] << 16);
    }

    const uint32_t g = g0 + slot, by = g / nbx, bx = g - by * nbx;
    if (act && bx >= w.bx0 && bx <= w.bx1 && by >= w.by0 && by <= w.by1) {
#pragma unroll
        for (int c = 0; c < BG; c++) {
            const uint32_t excl = ((sinc[c >> 1] >> (16 * (c & 1))) - (spk[c >> 1] >> (16 * (c & 1)))) & 0xffffu;
            const uint32_t pv = (pv0[c] + excl) & 0xffffu;
#pragma unroll
            for (int j = 0; j < 8; j++) rp[c][j] = pk_add16(rp[c][j], pv * 0x00010001u);
        }
#pragma unroll
        for (int c = 0; c < BG; c++) {
            const int cb = core_of<BG, RGB>(c);
            if (cb != c)        // the R-G, G, B-G map applies to the first three bands of the image: group 0 only
#pragma unroll
                for (int j = 0; j < 8; j++) rp[c][j] = pk_add16(rp[c][j], grp == 0 ? rp[cb][j] : 0u);
        }
        // the block's real pixel origin (last column / row shifted, not padded), clipped to the window: a shifted block stores its own
        // columns / rows only, as in win_decode_wave
        const uint32_t xb = (4 * bx + 4 > a.g.w) ? a.g.w - 4 : 4 * bx;
        const uint32_t yb = (4 * by + 4 > a.g.h) ? a.g.h - 4 : 4 * by;
        const bool whole = xb == 4 * bx && xb >= w.wx0 && xb + 4 <= w.wx1;     // all four columns are the block's and the window's
        uint32_t colmask = 0;                                       // bit x: column xb + x is the block's and the window's
#pragma unroll
        for (uint32_t x = 0; x < 4; x++) colmask |= (xb + x >= 4 * bx && xb + x >= w.wx0 && xb + x < w.wx1) ? 1u << x : 0u;
        // byte offset of the lane's bands of the block's first pixel in the window (an edge block starts left of or above it: only the
        // halfwords under the masks are addressed)
        const int64_t off0 = ((int64_t)yb - (int64_t)w.wy0) * (int64_t)w.dstride + (((int64_t)xb - (int64_t)w.wx0) * B + band0) * 2;
        // N dwords to a halfword address: aligned dwords when it is dword aligned, else a head halfword, the aligned dwords inside and
        // a tail halfword -- never a byte outside the N dwords' own place.  The form is chosen from the address, row by row
        auto store_dw = [](uint16_t *p, const uint32_t *s, auto nconst) {
            constexpr int N = decltype(nconst)::value;
            if (!((uintptr_t)p & 2)) {
#pragma unroll
                for (int t = 0; t < N; t++) ((uint32_t *)p)[t] = s[t];
            } else {
                p[0] = (uint16_t)s[0];
                uint32_t *mid = (uint32_t *)(p + 1);
#pragma unroll
                for (int t = 0; t + 1 < N; t++) mid[t] = __builtin_amdgcn_alignbit(s[t + 1], s[t], 16);
                p[2 * N - 1] = (uint16_t)(s[N - 1] >> 16);
            }
        };
#pragma unroll
        for (int y = 0; y < 4; y++) {
            uint32_t ow[2 * BG];
#pragma unroll
            for (int j = 0; j < 2 * BG; j++) {          // halfwords 2j, 2j+1 of the lane's row: band h % BG of pixel h / BG
                const int h0 = 2 * j, h1 = 2 * j + 1;
                const int i0 = curve_pos_of(ORDER, h0 / BG, y), i1 = curve_pos_of(ORDER, h1 / BG, y);
                const uint32_t sel = (uint32_t)(2 * (i0 & 1)) | (uint32_t)(2 * (i0 & 1) + 1) << 8 |
                                     (uint32_t)(4 + 2 * (i1 & 1)) << 16 | (uint32_t)(4 + 2 * (i1 & 1) + 1) << 24;
                ow[j] = __builtin_amdgcn_perm(rp[h1 % BG][i1 >> 1], rp[h0 % BG][i0 >> 1], sel);
            }
            if (yb + y < 4 * by || yb + y < w.wy0 || yb + y >= w.wy1) continue;     // the neighbour's row, or one above or below the window
            uint16_t *rowp = (uint16_t *)(w.dst + (off0 + (int64_t)y * (int64_t)w.dstride));
            if (!whole) {           // edge block: the halfwords of the window's columns, one by one
#pragma unroll
                for (int i = 0; i < 4 * BG; i++)
                    if ((colmask >> (i / BG)) & 1u) rowp[(i / BG) * B + i % BG] = (uint16_t)(ow[i >> 1] >> (16 * (i & 1)));
                continue;
            }
            if constexpr (BG == 4) {
                // eight bands, the block's row on a 16-byte address (the two lanes of a block see the same address and both come here):
                // they swap halves -- the even lane takes pixels 0 and 1 whole, the odd lane pixels 2 and 3 -- and store 32 contiguous
                // bytes each, as dec_px16_kernel does.  Any other address: each lane stores its own half of every pixel
                if (NG == 2 && !((uintptr_t)(rowp - band0) & 15)) {
                    uint32_t rcv[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) rcv[j] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(grp ? ow[j] : ow[4 + j]), 0xb1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
                    const uint4 pa = grp ? make_uint4(rcv[0], rcv[1], ow[4], ow[5]) : make_uint4(ow[0], ow[1], rcv[0], rcv[1]);
                    const uint4 pb = grp ? make_uint4(rcv[2], rcv[3], ow[6], ow[7]) : make_uint4(ow[2], ow[3], rcv[2], rcv[3]);
                    uint4 *dst = (uint4 *)(rowp - band0 + (grp ? 2 * B : 0));
                    dst[0] = pa; dst[1] = pb;
                    continue;
                }
            }
            if constexpr (BG % 2 == 0) {
#pragma unroll
                for (int x = 0; x < 4; x++) store_dw(rowp + (uint64_t)x * B, &ow[x * (BG / 2)], std::integral_constant<int, BG / 2>());
            } else
                store_dw(rowp, &ow[0], std::integral_constant<int, 2 * BG>());      // (one or three bands: the lane's row is contiguous)
        }
    }
    if (bad) atomicOr(status, fits ? 1u : 8u);
    // a segment that reaches beyond the stream's end (a stream cut short): the whole-raster decode decides what its pixels are
    if (lane == 0 && (P1 > a.in_bits || P1 < P0)) atomicOr(status, 4u);
    if (lane == 63 && (uint64_t)seg == a.g.nseg - 1 && fits) {      // reference: more than 7 unused bits at the end is a failure
        const uint64_t used = (uint64_t)(cpos + binc - stage_bit0) + 32 * w0 - a.in_bit0;
        if (used > a.in_bits) atomicOr(status, 4u);
        else if (a.in_bits - used > 7) atomicOr(status, 2u);
    }
}

// The family's instantiations (k_dec_win16.hip, k_dec_wins16_ranged.hip), by the plan's bands per lane and band map, the raster's order
// and mode; four waves a SIMD asked for
template <int BG, bool RGB, uint64_t ORDER, bool STEP>
struct Win16 {
    static constexpr int waves = 4;
    static constexpr auto contig = &win16_decode_wave<BG, RGB, ORDER, STEP, WinSrcContig>;
    static constexpr auto pieces = &win16_decode_wave<BG, RGB, ORDER, STEP, WinSrcPieces>;
};
template <class Visit>
inline void win16_pick(const Geometry &g, const DecPlan &plan, Visit visit) {
    const bool step = g.mode != CM_FTL, z = g.order == ZCURVE;
    auto go = [&](auto bgc, auto rgbc) {
        constexpr int BG = decltype(bgc)::value;
        constexpr bool RGB = decltype(rgbc)::value;
        if (!z && !step) visit(Win16<BG, RGB, HILBERT, false>());
        else if (!z && step) visit(Win16<BG, RGB, HILBERT, true>());
        else if (z && !step) visit(Win16<BG, RGB, ZCURVE, false>());
        else visit(Win16<BG, RGB, ZCURVE, true>());
    };
    using T = std::true_type; using F = std::false_type;
    switch (plan.px16_bg) {
    case 1: go(WinInt<1>(), F()); break;
    case 2: go(WinInt<2>(), F()); break;
    case 3: if (plan.px_rgb) go(WinInt<3>(), T()); else go(WinInt<3>(), F()); break;
    default: if (plan.px_rgb) go(WinInt<4>(), T()); else go(WinInt<4>(), F()); break;
    }
}

void win16_ranged(const Geometry &g, const DecPlan &plan, const WinRangedArgs &ra, const WinLaunch &l);      // (k_dec_wins16_ranged.hip)

inline void window16_dec_args(DecArgs &a, const DecPlan &plan) {       // what dec_px16_kernel's lanes take besides window_dec_args
    a.px_ng = plan.px16_ng; a.px_magic_ng = magic_div(a.px_ng); a.in_cap_full = plan.px_cap_dw;
}

}  // namespace qb3dev
