// qb3_amd/csrc/qb3_pxu.h -- what the lane-per-unit decoders share (k_dec_pxu.hip: the whole raster; qb3_win_unit.h and qb3_win_best_unit.h:
// the window kernels): the shuffle and the scan along a band, the band map as nibbles, the pieces a block's row is stored in, the
// little-endian fields of a table entry, the LDS a wave needs, the fill of the wave's tile, and the common-factor units of a segment.
#pragma once
#include "qb3_wide.h"

namespace qb3dev {

template <typename T> __device__ __forceinline__ T pxu_shfl(T v, uint32_t src) {
    if constexpr (sizeof(T) == 8) return (T)__shfl((unsigned long long)v, (int)src, 64);
    else return (T)__shfl((unsigned)v, (int)src, 64);
}
// exclusive scan along the lanes `stride` apart (a band's units)
template <typename T> __device__ __forceinline__ T pxu_exscan_band(T v, uint32_t stride) {
    const uint32_t lane = threadIdx.x & 63;
    T x = v;
    for (uint32_t d = stride; d < 64; d <<= 1) {
        T y;
        if constexpr (sizeof(T) == 8) y = (T)__shfl_up((unsigned long long)x, d, 64);
        else y = (T)__shfl_up((unsigned)x, d, 64);
        if (lane >= d) x = (T)(x + y);
    }
    return (T)(x - v);
}
// the band map, four bits a band (a lane indexes it by its band: kernel arguments live in scalar registers)
__device__ __forceinline__ uint64_t pxu_band_nibbles(const DecArgs &a0) {
    uint64_t n = 0;
    for (uint32_t c = 0; c < (uint32_t)MAXBANDS; c++) n |= (uint64_t)(a0.g.cband[c] & 15u) << (4 * c);
    return n;
}
// a piece of a block's row: sixteen, eight or four bytes, whichever divides the row's 4 x bands x value size bytes
template <int N> struct PxuPiece;
template <> struct PxuPiece<16> { typedef uint32_t v __attribute__((ext_vector_type(4))); };
template <> struct PxuPiece<8> { typedef uint32_t v __attribute__((ext_vector_type(2))); };
template <> struct PxuPiece<4> { typedef uint32_t v; };

// The wave's tile, laid out like the image ([row][block][x][band], RP elements a pixel row): o[i] is the value of curve position i of
// the lane's unit (block blk of the segment, band c of B).  The tile takes the place of the staged words, which are dead once every
// lane holds its values; behind the fill the wave may read what any of its lanes wrote.
template <typename T>
__device__ __forceinline__ void pxu_tile_fill(T *tile, const T (&o)[16], bool act, uint32_t blk, uint32_t c, uint32_t B, uint32_t RP, uint64_t order) {
    if (act) {
        const uint32_t e0 = blk * 4 * B + c;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t nib = curve_nib(order, i);
            tile[e0 + (nib >> 2) * RP + (nib & 3) * B] = o[i];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The same for a band-selected window: the tile holds S output slots a pixel ([row][block][x][slot], RP = blocks * 4 * S elements a pixel
// row), slot k takes band (nibs >> 4k) & 15.  A lane writes its sixteen values to every slot that names its band -- the slots are a mask
// it computes once and walks bit by bit -- and a lane whose band no slot names writes nothing.  blocks * S <= 64: the tile stays inside
// pxu_wave_bytes.  Slots are one value apart, as bands are in pxu_tile_fill: the stores read the tile as rows of bytes, and a slot
// stride with a gap would cost them their pieces; at most as many lanes as there write into one dword (fewer slots than bands: fewer).
template <typename T>
__device__ __forceinline__ void pxu_tile_fill_sel(T *tile, const T (&o)[16], bool act, uint32_t blk, uint32_t c, uint32_t S, uint64_t nibs, uint32_t RP, uint64_t order) {
    uint32_t slots = 0;
    for (uint32_t k = 0; k < S; k++) slots |= (((uint32_t)(nibs >> (4 * k)) & 15u) == c) ? 1u << k : 0u;
    if (!act) slots = 0;
    while (slots) {
        const uint32_t k = (uint32_t)__builtin_ctz(slots);
        slots &= slots - 1;
        const uint32_t e0 = blk * 4 * S + k;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t nib = curve_nib(order, i);
            tile[e0 + (nib >> 2) * RP + (nib & 3) * S] = o[i];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bytes of LDS a wave needs: the staged words and, in their place afterwards, the tile; then a slot per block
// (PXU_PAD zero words behind the staged ones: what wide_values_lds reads beyond a position inside the staged bits, qb3_wide.h)
constexpr uint32_t PXU_PAD = WIDE_PAD_DW;
__host__ __device__ inline uint32_t pxu_wave_bytes(uint32_t in_cap_dw, uint32_t tsz) {
    const uint32_t st = 4 * (in_cap_dw + PXU_PAD), tl = 16 * 64 * tsz;
    return (((st > tl ? st : tl) + 15u) & ~15u) + 8 * 32;
}

template <typename T> __device__ __forceinline__ uint64_t pxu_le(const uint8_t *q, uint32_t n) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < n; i++) v |= (uint64_t)q[i] << (8 * i);
    return v;
}

// The common-factor units of a wave's segment, a lane a unit (lane = blk * B + c; with one band a lane a block), out of the staged words
// (ndw of them, PXU_PAD zero words behind): bt is the unit's bits | the rung it is entered with << 16, cpos the segment's first bit in
// the staged words (units follow one another in lane order: a scan of their bits places each, and no unit starts beyond the staged bits),
// cf0 the factor its band enters the segment with.  A lane parses its unit assuming cf0; the band's units that brought a factor are
// found by ballot, the nearest one below the lane gives the factor in force, and only a lane that assumed wrongly parses again.
// run: the running sums of the unit's sixteen values; returned: the inclusive scan of the units' bits (the last lane holds the bits of
// the segment).  bad is raised for a malformed unit, one that does not end where its length says, and one that leaves its band at
// another rung than the band's next unit of the segment is entered with.
template <typename T>
__device__ __forceinline__ uint32_t pxu_best_units(const uint32_t *stage, uint32_t ndw, uint32_t cpos, uint32_t bt, T cf0, bool act, uint32_t blk, uint32_t c,
                                                   uint32_t B, uint32_t nb_here, T (&run)[16], bool &bad) {
    constexpr uint32_t UB = UBits<T>::v, UMASK = (1u << UB) - 1;
    const uint32_t lane = threadIdx.x & 63, limit = 32 * ndw;
    const uint32_t blen = bt & 0xffffu, oldrung = (bt >> 16) & UMASK;
    const uint32_t binc = wave_iscan32(blen);
    uint32_t pos = cpos + binc - blen;
    pos = pos < limit ? pos : limit;
    // the rung the band's NEXT unit is entered with is the rung this unit must leave: checked, not trusted
    const uint32_t nxt = (uint32_t)__shfl_down((unsigned)(bt >> 16), B, 64);
    uint64_t period = 0;                                            // lanes 0, B, 2B, ...: shifted by its band, a lane's band
    for (uint32_t k = 0; k < 64; k += B) period |= 1ull << k;
    T g[16], pcf = cf0, cf_in = cf0;
#pragma unroll
    for (int i = 0; i < 16; i++) g[i] = 0;
    uint32_t rung = oldrung, flags = 0, end = pos;
    bool ok = true, need = act;
#pragma nounroll
    for (int pass = 0; pass < 2; pass++) {
        if (need) {
            ReaderT<LdsWords> rd;
            rd.init((LdsWords)stage, pos, 32ull * (ndw + PXU_PAD));
            rung = oldrung; pcf = cf_in; flags = 0;
            ok = parse_unit<T, CM_BEST, ReaderT<LdsWords>>(rd, rung, pcf, g, &flags);
            end = (uint32_t)rd.position();
        }
        if (pass) break;
        // the factor in force for a unit that takes the band's: the nearest lane of the band below whose unit brought one
        const uint64_t wm = __ballot(act && (flags & 2u));
        if (!wm) break;                                             // (no writer in the segment: every lane assumed right)
        const uint64_t below = wm & (period << c) & ((1ull << lane) - 1);
        const uint32_t src = below ? 63u - (uint32_t)__clzll((long long)below) : lane;
        const T got = pxu_shfl<T>(pcf, src);
        need = act && (flags & 1u) && below && got != cf0;
        cf_in = got;
        if (!__any(need)) break;
    }
    if (act && (!ok || end != pos + blen)) bad = true;              // malformed unit, or the lengths are not this stream's
    if (act && blk + 1 < nb_here && rung != (nxt & UMASK)) bad = true;
    T acc = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) { acc = (T)(acc + smag_t<T>(g[i])); run[i] = acc; }
    return binc;
}

}  // namespace qb3dev
