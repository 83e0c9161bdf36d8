// qb3_amd/csrc/qb3_win_best.h -- the wave's work of the window kernels for 8-bit rasters in the common-factor modes (k_dec_win_best.hip):
// a segment decoded from its table entry as dec_px_best_kernel's BL branch decodes it (k_dec_px_best.hip: a lane per block, the bands one
// after the other, the factor in force found by a ballot of the segment's own lanes), its blocks clipped to the window and stored as
// win_decode_wave (qb3_win.h) clips and stores them.  Mapping, de-duplication, trust and status are that function's.
#pragma once
#include "qb3_px_best.h"
#include "qb3_win.h"

namespace qb3dev {

// The launch bound's second number: four bands are built for the five waves a SIMD dec_px_best_kernel<4, ...> reaches by its 92
// registers -- left to itself the compiler gives the four-band window kernels 98 and one step less; with the bound, 90 and no scratch.
// One and three bands reach the whole decoder's steps (8 and 6) unasked: asked for five, three bands take 82 registers and fall to
// five; asked for eight, one band spills.  These are one compiler version's register allocations, and the choice follows the whole
// decoder's occupancy step: that five waves at 90 registers outrun four at 98 on the GPU has NOT been measured
constexpr int win_best_waves(int B) { return B == 4 ? 5 : 1; }

// Wave `wid` of window w (wave: its number in the workgroup of four; both wave uniform).  status: the word this window's failures go to.
// Every wave of the workgroup comes here (there is one workgroup barrier); smem: the launch's dynamic LDS, at LDS address 0, sized as
// launch_dec_px_best sizes it (a.in_cap_dw = the plan's px_cap_dw, eight zero words behind a wave's segment): the readers reach as far
// behind the staged words as they do in dec_px_best_kernel.  All 64 lanes decode -- a block's entering value and the factor in force
// come from the lanes below it -- and the lanes whose block is the window's store.
template <int B, bool RGB, uint64_t ORDER, class SRC = WinSrcContig>
__device__ __forceinline__ void win_best_decode_wave(const DecArgs &a, const WinDesc &w, uint32_t *status, uint8_t *smem, uint32_t wave, uint32_t wid, SRC src = SRC()) {
    constexpr int NW = (B + 1) / 2;                     // 32-bit words of a scan packed 16 bits per band
    constexpr uint32_t NB = 64;                         // blocks of a segment
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t nbx = a.g.nbx;

    uint32_t *tab = (uint32_t *)smem;                   // 4 KB, at LDS address 0 (the table addressing relies on it)
    uint32_t *stage = tab + 1024 + wave * (a.in_cap_dw + 8);
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
    const bool act = live && lane < nb_here;
    uint64_t P0, P1;
    uint32_t bt = 0, pv0[B], cf0[B];                    // bt: the block's bits | entering rungs << 16 (four bits a band)
    {
        const uint8_t *e = src.entry(a, segc);
        auto pos6 = [](const uint8_t *q) { uint64_t v = 0;
#pragma unroll
            for (uint32_t i = 0; i < 6; i++) v |= (uint64_t)q[i] << (8 * i);
            return v; };
        P0 = pos6(e);
        P1 = ((uint64_t)segc + 1 < a.g.nseg) ? pos6(src.entry(a, segc + 1)) : a.in_bits;
#pragma unroll
        for (int c = 0; c < B; c++) { pv0[c] = e[6 + B + c]; cf0[c] = e[6 + 2 * B + c]; }
        const uint8_t *fp = e + 6 + 3 * B + IX_BL_BEST_BYTES * lane;
        const uint32_t f = act ? (uint32_t)fp[0] | (uint32_t)fp[1] << 8 | (uint32_t)fp[2] << 16 : 0u;
        bt = f & 0xfffu;
#pragma unroll
        for (int c = 0; c < 4; c++) bt |= ((f >> (12 + 3 * c)) & 7u) << (16 + 4 * c);
        // (the entry's own rung bytes e[6 + c] repeat block 0's field; the field is what is used, as in the whole decoder)
    }
    for (uint32_t i = tid; i < 256; i += blockDim.x) ((uint4 *)tab)[i] = ((const uint4 *)px_dec_tab.e)[i];
    __syncthreads();                                    // the only workgroup barrier
    if (!live) {
        if (!placed && lane == 0) atomicOr(status, 8u);
        return;
    }
    // the segment's words from the word its first bit is in, through the source: no word outside [w0, w0 + ndw) is read, whatever the
    // entries say, and none at or behind the container's end; eight zero words follow
    const uint64_t w0 = (a.in_bit0 + P0) >> 5;
    const uint64_t endw_abs = (a.in_bit0 + a.in_bits + 31) >> 5;
    const uint64_t ndw64 = ((a.in_bit0 + P1 + 31) >> 5) - w0;
    // the staging area holds the longest valid segment; a table that says otherwise is not this stream's
    const bool fits = ndw64 <= a.in_cap_dw && lds0 == 0 && src.holds(w0, ndw64);
    const uint32_t ndw = fits ? (uint32_t)ndw64 : 0;
    for (uint32_t base = 0; base < ndw + 8; base += 512) {          // eight loads in flight per lane, then eight LDS stores
        uint32_t sw[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = base + lane + 64 * j;
            sw[j] = i < ndw ? src.word(a, w0 + i, endw_abs) : 0u;
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
    const uint32_t blen = bt & 0xffffu;
    const uint32_t binc = wave_iscan32(blen);           // inclusive: lane 63 holds the bits of the segment
    uint32_t pos = cpos + binc - blen;
    const uint32_t blk_end = pos + blen;
    // the rungs the NEXT block is entered with are the rungs this block's units must leave: checked, not trusted
    const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(bt >> 16), 0x130, 0xf, 0xf, false);      // wave_shl:1
    uint32_t rp[B][8], spk[NW], sinc[NW];
    bool clamped = false;
#pragma unroll
    for (int j = 0; j < NW; j++) spk[j] = 0;
    // band after band, as dec_px_best_kernel (restated: sharing the loop changed that kernel's code): a unit without the signal is
    // QB3M_BASE's; one with it is parsed by the lane, multiplied by the band's factor in force, and leaves the band at the rung of the
    // multiplied values
#pragma unroll
    for (int c = 0; c < B; c++) {
        if (pos > limit) { pos = limit; clamped = true; }       // (a table's length that leads behind what was staged: the unit reads zeros)
        const uint32_t oldrung = (bt >> (16 + 4 * c)) & 7u;
        bool sig; uint32_t csl, sw;
        const uint32_t d = px_switch(pos, &csl, &sig, &sw);
        uint32_t rung = (oldrung + d) & 7u, end = pos, tot = 0;
        uint8_t g[16];
        uint32_t kind = 3, cfv = 0;
        const bool slow = act && sig;
        if (slow) { if (!best_slow_unit(pos + csl, oldrung, g, &kind, &cfv, &rung, &end)) bad = true; }
        else tot = px_group<true, true>(pos + csl, rung, rp[c], &end, sw) & 0xffu;
        if (__any(slow)) {
            // the factor in force: the nearest lane below with a unit that brought its own, else the segment entry's
            const uint64_t wm = __ballot(slow && kind == 0);
            const uint64_t below = wm & ((1ull << lane) - 1);
            const uint32_t from = below ? 63u - (uint32_t)__clzll((long long)below) : lane;
            const uint32_t got = (uint32_t)__shfl((int)cfv, (int)from, 64);
            if (slow) {
                if (kind == 1) cfv = below ? got : cf0[c];
                uint32_t acc = 0, used = 0;
                const uint32_t cf = (cfv + 2) & 0xffu;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    uint32_t v = g[i];
                    if (kind < 2) v = ((((v >> 1) + (v & 1)) * (cf << 1)) - (v & 1)) & 0xffu;     // magsmul (QB3decode.h:575)
                    used |= v;
                    acc += (v >> 1) ^ (0u - (v & 1u));                                          // mag-sign undone
                    if (i & 1) rp[c][i >> 1] |= acc << 16; else rp[c][i >> 1] = acc & 0xffffu;
                }
                tot = acc & 0xffu;
                if (kind < 2) {
                    // the band's rung is that of the multiplied values (QB3decode.h:664); a factor above them: malformed (:665)
                    if (rung == 0) rung = topbit32(((cf - 1) << 1) | 1);
                    else { rung = topbit32(used | 1); if (cf > used) bad = true; }
                }
            }
        }
        if (act && lane + 1 < nb_here && rung != ((nxt >> (4 * c)) & 7u)) bad = true;
        spk[c >> 1] |= (act ? tot : 0u) << (16 * (c & 1));
        pos = end;
    }
    // the table's lengths are not this stream's.  (The `clamped` exemption is dec_px_best_kernel's; a P1 beyond in_bits is not zeroed
    // here but raises 4 below, which is win_decode_wave's rule: either way the window goes to the whole decode)
    if (act && !clamped && pos != blk_end) bad = true;
#pragma unroll
    for (int j = 0; j < NW; j++) sinc[j] = wave_iscan32(spk[j]);

    const uint32_t g = g0 + lane, by = g / nbx, bx = g - by * nbx;
    if (act && bx >= w.bx0 && bx <= w.bx1 && by >= w.by0 && by <= w.by1) {      // clipping and stores: win_decode_wave's, byte for byte
        // entering value, then the core band (reference QB3decode.h:730-737)
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
        const bool whole = xb == 4 * bx && xb >= w.wx0 && xb + 4 <= w.wx1;     // all four columns are the block's and the window's
        uint32_t colmask = 0;                                       // bit x: column xb + x is the block's and the window's
#pragma unroll
        for (uint32_t x = 0; x < 4; x++) colmask |= (xb + x >= 4 * bx && xb + x >= w.wx0 && xb + x < w.wx1) ? 1u << x : 0u;
        // byte offset of the block's first row in the window (an edge block starts left of or above it: only the bytes under
        // the masks are addressed)
        const int64_t off0 = ((int64_t)yb - (int64_t)w.wy0) * (int64_t)w.dstride + ((int64_t)xb - (int64_t)w.wx0) * B;
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
            if (yb + y < 4 * by || yb + y < w.wy0 || yb + y >= w.wy1) continue;     // the neighbour's row, or one above or below the window
            uint8_t *row = w.dst + (off0 + (int64_t)y * (int64_t)w.dstride);
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
    if (bad) atomicOr(status, fits ? 1u : 8u);
    // a segment that reaches beyond the stream's end (a stream cut short): the whole-raster decode decides what its pixels are
    if (lane == 0 && (P1 > a.in_bits || P1 < P0)) atomicOr(status, 4u);
    if (lane == 63 && (uint64_t)seg == a.g.nseg - 1 && fits) {      // reference: more than 7 unused bits at the end is a failure
        const uint64_t used = (uint64_t)(cpos + binc - stage_bit0) + 32 * w0 - a.in_bit0;
        if (used > a.in_bits) atomicOr(status, 4u);
        else if (a.in_bits - used > 7) atomicOr(status, 2u);
    }
}

// The family's instantiations (k_dec_win_best.hip, k_dec_wins_best_ranged.hip), by the raster's bands, the plan's band map and the
// raster's order
template <int B, bool RGB, uint64_t ORDER>
struct WinCf8 {
    static constexpr int waves = win_best_waves(B);
    static constexpr auto contig = &win_best_decode_wave<B, RGB, ORDER, WinSrcContig>;
    static constexpr auto pieces = &win_best_decode_wave<B, RGB, ORDER, WinSrcPieces>;
};
template <class Visit>
inline void win_cf8_pick(const Geometry &g, const DecPlan &plan, Visit visit) {
    auto go = [&](auto bc, auto rgbc) {
        constexpr int B = decltype(bc)::value;
        constexpr bool RGB = decltype(rgbc)::value;
        if (g.order == ZCURVE) visit(WinCf8<B, RGB, ZCURVE>());
        else visit(WinCf8<B, RGB, HILBERT>());
    };
    using T = std::true_type; using F = std::false_type;
    switch (g.bands) {
    case 1: go(WinInt<1>(), F()); break;
    case 3: if (plan.px_rgb) go(WinInt<3>(), T()); else go(WinInt<3>(), F()); break;
    default: if (plan.px_rgb) go(WinInt<4>(), T()); else go(WinInt<4>(), F()); break;
    }
}
void win_cf8_ranged(const Geometry &g, const DecPlan &plan, const WinRangedArgs &ra, const WinLaunch &l);    // (k_dec_wins_best_ranged.hip)

}  // namespace qb3dev
