// qb3_amd/csrc/qb3_px16.h -- what the 16-bit lane-per-(block, band group) decoders share (k_dec_px16.hip: the whole raster; qb3_win16.h: the
// window kernels): the rung switch, the units above the table's rungs, the scan over the lanes of a band group.
#pragma once
#include "qb3_px.h"

namespace qb3dev {

__device__ __forceinline__ uint32_t px16_switch(uint32_t pos, uint32_t *cslen, bool *signal) {
    uint32_t x = lds_bits(pos);
    *signal = false;
    if (!(x & 1)) { *cslen = 1; return 0; }
    x >>= 1;                                            // code at rung 3 (reference QB3decode.h:97-116)
    uint32_t m, len;
    if (!(x & 1)) { m = (x & 7) >> 1; len = 3; }
    else if (!(x & 2)) { m = ((x >> 2) & 3) | 4; len = 4; }
    else { m = ((x >> 2) & 7) | 8; len = 5; }
    *cslen = 1 + len;
    if (m == 14) { *signal = true; return 0; }
    return (m & 1) ? (16 - (m + 1) / 2) & 15 : m / 2 + 1;
}

// The units of a lane's BG bands whose rung is 8 or more, by the code rule (values do not fit the 8-bit tables): 16
// values each from bit gpos[c]; rp[c][k] = running sums of values 2k, 2k+1 (16-bit halves); tot[c] = the unit's total.
// The BG walks are independent chains of data-dependent LDS reads and shifts, so they advance in LOCKSTEP, code by
// code: several reads in flight instead of one (the kernel is bound by that latency, not by issue: SQ_INSTS_VALU x 2 /
// SIMD = 28 % of its duration when the bands were walked one after the other).  A band whose rung is below 8 walks
// along with a harmless result (its reads stay inside the staged words and their zero margin); the caller overwrites it.
// RS: the N bands are RS apart in the caller's arrays; endp (when given): the bit behind each unit.
template <bool STEP, int N, int RS = 1>         // N bands at a time: two is what the registers hold without spilling
__device__ __forceinline__ void px16_groups_hi(const uint32_t *gpos, const uint32_t *rung, uint32_t (*rp)[8], uint32_t *tot, uint32_t *endp = nullptr) {
    constexpr int BG = N;
    uint32_t pos[BG], acc[BG], fl[BG], top[BG], half[BG];
    uint64_t buf[BG];
#pragma unroll
    for (int c = 0; c < BG; c++) { pos[c] = gpos[c * RS]; acc[c] = 0; fl[c] = 0; top[c] = 1u << rung[c * RS]; half[c] = top[c] >> 1; buf[c] = 0; }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (i % 3 == 0) {                               // three codes are at most 51 bits
#pragma unroll
            for (int c = 0; c < BG; c++) {
                LdsWords p = lds_at((pos[c] >> 3) & ~3u);
                const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
                buf[c] = ((uint64_t)__builtin_amdgcn_alignbit(d2, d1, pos[c]) << 32) | __builtin_amdgcn_alignbit(d1, d0, pos[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < BG; c++) {
            const uint32_t x = (uint32_t)buf[c];
            const bool c1 = x & 1, c2 = (x & 3) == 3;
            const uint32_t len = rung[c * RS] + c1 + c2;
            const uint32_t v = c2 ? (((x >> 2) & (top[c] - 1)) | top[c]) : c1 ? (((x >> 2) & (half[c] - 1)) | half[c]) : ((x & (top[c] - 1)) >> 1);
            buf[c] >>= len; pos[c] += len;
            acc[c] += (v >> 1) ^ (0u - (v & 1u));       // undo mag-sign, accumulate (mod 2^16 in the packed halves)
            if (STEP) fl[c] |= ((uint32_t)c2 | ((v & 1u) << 1)) << (2 * i);
            if (i & 1) rp[c * RS][i >> 1] |= acc[c] << 16; else rp[c * RS][i >> 1] = acc[c] & 0xffffu;
        }
    }
#pragma unroll
    for (int c = 0; c < BG; c++) {
        if (endp) endp[c * RS] = pos[c];
        if (STEP) {                                     // undo the step (reference QB3decode.h:285-289), as in px_group
            const uint32_t tb = fl[c] & 0x55555555u, u = tb | (tb << 1);
            const uint32_t m = __popc(tb);
            if ((u & (u + 1)) == 0 && m < 16) {
                const uint32_t c16 = ((fl[c] >> (2 * m + 1)) & 1u) ? (0u - half[c]) & 0xffffu : half[c];
                const uint32_t ge = 0xffff0000u >> (16 - m);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint32_t pair = (ge >> (2 * k)) & 3u;
                    rp[c * RS][k] = pk_add16(rp[c * RS][k], ((pair | (pair << 15)) & 0x00010001u) * c16);
                }
                acc[c] += c16;
            }
        }
        tot[c * RS] = acc[c];
    }
}

// inclusive scan over the lanes of the same band group (stride NG), NW words per lane
template <int NW>
__device__ __forceinline__ void group_iscan(uint32_t (&v)[NW], uint32_t NG) {
    if (NG == 1) {
#pragma unroll
        for (int k = 0; k < NW; k++) v[k] = wave_iscan32(v[k]);
        return;
    }
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t d = NG; d < 64; d <<= 1) {
#pragma unroll
        for (int k = 0; k < NW; k++) {
            const uint32_t y = __shfl_up(v[k], d, 64);
            if (lane >= d) v[k] += y;
        }
    }
}

}  // namespace qb3dev
