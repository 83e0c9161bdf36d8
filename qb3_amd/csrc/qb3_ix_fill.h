// qb3_amd/csrc/qb3_ix_fill.h -- the restart table's chunks ("ix", include/qb3x.h) from a decode index (IndexView, qb3_dev.h): the
// entries of every layout ix_layout knows, the chunk heads and pads, the checks.  Device code shared by the encoder's table kernels
// (k_enc_post.hip: the index is the one the coding kernels left) and the reindex kernels (k_reindex.hip: the index is the one the walk
// of a plain stream rebuilt in the decoder's workspace).  Both write the same bytes for the same index.
#pragma once
#include "qb3_kernels.h"

namespace qb3dev {

// what the fill and seal code needs to know: the index, where the first chunk goes, the table's layout (IxTable), the raster's shape
struct IxFill {
    IndexView idx;
    uint8_t *dst;               // the first chunk's first byte; "DT" goes right behind the last chunk's pad
    uint64_t nblocks;
    uint32_t bands, tsz, ulen_sz;
    uint32_t best;              // a common-factor stream: entries carry the factors in force
    uint32_t K, E, per_chunk, blocks;   // entries, bytes an entry, entries a chunk, blocks an entry
    uint32_t spe;               // index segments per entry
    uint32_t bl;                // entries end with block / unit fields
    uint32_t px16_bg;           // 16-bit rasters: bands a lane of the decoder owns (what the fields are counted by)
};
__device__ __forceinline__ IxFill ix_fill_of(const EncArgs &a) {
    IxFill f;
    f.idx = a.idx; f.dst = a.ix_dst; f.nblocks = a.g.nblocks; f.bands = a.g.bands; f.tsz = a.g.tsz; f.ulen_sz = a.g.ulen_sz;
    f.best = a.g.mode == CM_BEST ? 1u : 0u;
    f.K = a.ix_K; f.E = a.ix_E; f.per_chunk = a.ix_per_chunk; f.blocks = a.ix_blocks; f.spe = a.ix_spe; f.bl = a.ix_bl; f.px16_bg = a.px16_bg;
    return f;
}

__device__ __forceinline__ uint32_t ix_entries_here(const IxFill &f, uint32_t c) {       // entries of chunk c
    return (f.K - c * f.per_chunk < f.per_chunk) ? f.K - c * f.per_chunk : f.per_chunk;
}
__device__ __forceinline__ uint8_t *ix_chunk_ptr(const IxFill &f, uint32_t c) { return f.dst + (uint64_t)c * (IX_HEAD + IX_PAD + (uint64_t)f.per_chunk * f.E); }
__device__ __forceinline__ uint8_t *ix_entry_ptr(const IxFill &f, uint64_t k) {
    const uint32_t c = (uint32_t)(k / f.per_chunk), jj = (uint32_t)(k - (uint64_t)c * f.per_chunk);
    return ix_chunk_ptr(f, c) + IX_HEAD + (uint64_t)jj * f.E;
}

// Chunk c's head -- "ix", length (the whole chunk: the reference skips unknown chunks by that many bytes from the chunk start,
// QB3decode.cpp:254-255), version 3, flags (bit 0: entries carry the common factors, bit 1: block lengths), the chunk's check, blocks per
// entry -- the "zz" pad chunk behind it and, behind the last chunk, "DT".  One thread.
__device__ __forceinline__ void ix_write_head(const IxFill &f, uint32_t c, uint32_t check) {
    const uint32_t here = ix_entries_here(f, c), len = IX_HEAD + here * f.E;
    uint8_t *chunk = ix_chunk_ptr(f, c);
    chunk[0] = 'i'; chunk[1] = 'x'; chunk[2] = (uint8_t)len; chunk[3] = (uint8_t)(len >> 8);
    chunk[4] = 3; chunk[5] = (uint8_t)((f.best ? 1 : 0) | (f.bl ? 2 : 0)); chunk[6] = (uint8_t)check; chunk[7] = (uint8_t)(check >> 8);
    for (uint32_t i = 0; i < 4; i++) chunk[8 + i] = (uint8_t)(f.blocks >> (8 * i));
    uint8_t *pad = chunk + len;
    pad[0] = 'z'; pad[1] = 'z'; pad[2] = 4; pad[3] = 0;
    if (c * f.per_chunk + here == f.K) { pad[4] = 'D'; pad[5] = 'T'; }
}

// An entry without fields, of index segment sgi (a multiple of spe) whose first unit stands at stream bit bp: position, a rung byte per
// band, the entering values, the factors in force (common-factor streams).  One thread.
__device__ __forceinline__ void ix_plain_entry(const IxFill &f, uint64_t sgi, uint64_t bp) {
    const uint32_t B = f.bands, tsz = f.tsz;
    uint8_t *e = ix_entry_ptr(f, sgi / f.spe);
    for (uint32_t i = 0; i < 6; i++) e[i] = (uint8_t)(bp >> (8 * i));
    e += 6;
    for (uint32_t c2 = 0; c2 < B; c2++) e[c2] = f.idx.rung[sgi * B + c2];
    e += B;
    const uint8_t *pv = (const uint8_t *)f.idx.prev + sgi * B * tsz;
    for (uint32_t i = 0; i < B * tsz; i++) e[i] = pv[i];
    if (f.best) {
        e += B * tsz;
        const uint8_t *cf = (const uint8_t *)f.idx.cf + sgi * B * tsz;
        for (uint32_t i = 0; i < B * tsz; i++) e[i] = cf[i];
    }
}

// Block lengths behind the entries' fixed fields (tables of level 2).  A block's bit length is the sum of its units'
// lengths (the index has them).  Four ten-bit fields are five whole bytes and an entry's 64 blocks are sixteen such
// groups: a thread per group of four blocks reads their 4 * B length bytes (whole dwords) and writes five bytes of
// the entry -- no two threads share a byte.  grp: blocks 4 * grp .. 4 * grp + 3
__device__ __forceinline__ void ix_bl_fill(const IxFill &f, uint64_t grp) {
    static_assert(IX_BL_BITS == 10, "groups of four fields are five bytes");
    const uint32_t B = f.bands;
    const uint64_t k = grp >> 4;                                                // 16 groups an entry
    if (k >= f.K) return;
    const uint64_t nblocks = f.nblocks, blk0 = 4 * grp;
    uint32_t len[4] = {0, 0, 0, 0};
    if (blk0 + 4 <= nblocks && ((uintptr_t)f.idx.ulen & 3) == 0) {
        const uint32_t *ul = (const uint32_t *)((const uint8_t *)f.idx.ulen + blk0 * B);    // 4 * B bytes: B dwords
        if (B == 1) { const uint32_t v = ul[0]; len[0] = v & 255; len[1] = (v >> 8) & 255; len[2] = (v >> 16) & 255; len[3] = v >> 24; }
        else if (B == 3) {
            const uint32_t v0 = ul[0], v1 = ul[1], v2 = ul[2];
            len[0] = (v0 & 255) + ((v0 >> 8) & 255) + ((v0 >> 16) & 255);
            len[1] = (v0 >> 24) + (v1 & 255) + ((v1 >> 8) & 255);
            len[2] = ((v1 >> 16) & 255) + (v1 >> 24) + (v2 & 255);
            len[3] = ((v2 >> 8) & 255) + ((v2 >> 16) & 255) + (v2 >> 24);
        } else {
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) { const uint32_t v = ul[q]; len[q] = (v & 255) + ((v >> 8) & 255) + ((v >> 16) & 255) + (v >> 24); }
        }
    } else {
        const uint8_t *ul = (const uint8_t *)f.idx.ulen + blk0 * B;
        for (uint32_t q = 0; q < 4; q++)
            if (blk0 + q < nblocks) for (uint32_t c = 0; c < B; c++) len[q] += ul[q * B + c];
    }
    const uint64_t bits = (uint64_t)len[0] | (uint64_t)len[1] << 10 | (uint64_t)len[2] << 20 | (uint64_t)len[3] << 30;
    uint8_t *e0 = ix_entry_ptr(f, k);
    uint8_t *e = e0 + 6 + 2 * B + 5 * (uint32_t)(grp & 15);
#pragma unroll
    for (uint32_t i = 0; i < 5; i++) e[i] = (uint8_t)(bits >> (8 * i));
    // the entry's fixed fields (an entry per segment: spe == 1, 8-bit values, no factors): at most 14 bytes, one per thread of
    // the entry's sixteen
    const uint32_t t = (uint32_t)(grp & 15);
    if (t < 6) e0[t] = (uint8_t)(f.idx.bitpos[k] >> (8 * t));
    else if (t < 6 + B) e0[t] = f.idx.rung[k * B + (t - 6)];
    else if (t < 6 + 2 * B) e0[t] = ((const uint8_t *)f.idx.prev)[k * B + (t - 6 - B)];
}

// four 24-bit fields as three dwords at any byte address (global memory takes unaligned dword stores)
__device__ __forceinline__ void ix_store12(uint8_t *e, const uint32_t (&f)[4]) {
    typedef uint32_t u32_a1 __attribute__((aligned(1)));
    u32_a1 *d = (u32_a1 *)e;
    d[0] = f[0] | f[1] << 24; d[1] = f[1] >> 8 | f[2] << 16; d[2] = f[2] >> 16 | f[3] << 8;
}
// The same for common-factor streams with a block table (8-bit grey / RGB / RGBA; 32/64-bit, one band): a three-byte field per
// block -- its bits (12) and the rungs its units are entered with (8-bit data: 3 bits a band; wide data: the band's whole rung)
// -- from the index's block table; a thread per four blocks writes twelve bytes and its share of the entry's fixed part
// (position, rungs, entering values, factors in force: 6 + bands * (1 + 2 * value size) bytes)
__device__ __forceinline__ void ix_bl_best_fill(const IxFill &f, uint64_t grp) {
    const uint32_t B = f.bands, tsz = f.tsz;
    const uint64_t k = grp >> 4;                                                // 16 groups an entry (64 blocks)
    if (k >= f.K) return;
    const uint64_t nblocks = f.nblocks, blk0 = 4 * grp;
    uint8_t *e0 = ix_entry_ptr(f, k);
    const uint32_t t = (uint32_t)(grp & 15), fixed = 6 + B * (1 + 2 * tsz);
    uint8_t *e = e0 + fixed + 4 * IX_BL_BEST_BYTES * t;
    uint32_t fl[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t bt = blk0 + q < nblocks ? ((const uint32_t *)f.idx.ulen)[blk0 + q] : 0u;
        uint32_t fd = bt & 0xfffu;
        if (tsz == 1) {
#pragma unroll
            for (uint32_t cc = 0; cc < 4; cc++) fd |= ((bt >> (16 + 4 * cc)) & 7u) << (12 + 3 * cc);
        } else fd |= ((bt >> 16) & 63u) << 12;
        fl[q] = fd;
    }
    ix_store12(e, fl);          // (four three-byte fields: three dwords at whatever address the entry puts them)
    for (uint32_t i = t; i < fixed; i += 16) {
        uint8_t v;
        if (i < 6) v = (uint8_t)(f.idx.bitpos[k] >> (8 * i));
        else if (i < 6 + B) v = f.idx.rung[k * B + (i - 6)];
        else if (i < 6 + B + B * tsz) v = ((const uint8_t *)f.idx.prev)[k * B * tsz + (i - 6 - B)];
        else v = ((const uint8_t *)f.idx.cf)[k * B * tsz + (i - 6 - B - B * tsz)];
        e0[i] = v;
    }
}

// The same for 16-bit rasters of four or eight bands: a field is the bit length of a band PAIR (two units), two fields per
// lane of the decoder's wave (lane = block of the segment x band group of four), 128 fields an entry.  A thread per four
// fields (two lanes): five whole bytes; the entry's first 6 + 3 * bands threads also write one byte each of its fixed part.
// grp: fields 4 * grp .. 4 * grp + 3 of entry grp / 32 (a single band: one field per lane -- the unit's length -- 64 fields an
// entry, 16 threads)
__device__ __forceinline__ void ix_bl16_fill(const IxFill &f, uint64_t grp) {
    static_assert(IX_BL_BITS == 10, "groups of four fields are five bytes");
    const uint32_t B = f.bands, BG = f.px16_bg, FPL = B == 1 ? 1 : 2, NG = B / BG, NB = 64 / NG, tpe = 16 * FPL;
    const uint64_t k = grp / tpe;
    if (k >= f.K) return;
    const uint32_t t = (uint32_t)(grp - k * tpe);
    uint64_t bits = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t field = 4 * t + q, lane = field / FPL, pair = field - lane * FPL;
        const uint32_t slot = lane / NG, g4 = lane - slot * NG;
        const uint64_t blk = k * NB + slot;
        uint32_t len = 0;
        if (slot < NB && blk < f.nblocks) {         // (lanes behind the segment's blocks x groups: nothing)
            // the lane's bands: BG from band BG * g4; four: the pairs (0,1), (2,3); three: (0,1) and band 2; two: a field a band; one: the unit
            const uint16_t *ul = (const uint16_t *)f.idx.ulen + blk * B + BG * g4;
            if (BG == 1) len = ul[0];
            else if (BG == 2) len = ul[pair];
            else if (BG == 3) len = pair ? (uint32_t)ul[2] : (uint32_t)ul[0] + ul[1];
            else len = (uint32_t)ul[2 * pair] + ul[2 * pair + 1];
        }
        bits |= (uint64_t)len << (IX_BL_BITS * q);
    }
    uint8_t *e0 = ix_entry_ptr(f, k);
    uint8_t *e = e0 + 6 + 3 * B + 5 * t;
#pragma unroll
    for (uint32_t i = 0; i < 5; i++) e[i] = (uint8_t)(bits >> (8 * i));
    // fixed part: bit position, a rung byte per band, the entering values (two bytes a band): 6 + 3 * B <= 30 bytes
    if (t < 6) e0[t] = (uint8_t)(f.idx.bitpos[k] >> (8 * t));
    else if (t < 6 + B) e0[t] = f.idx.rung[k * B + (t - 6)];
    else if (t < 6 + 3 * B) e0[t] = ((const uint8_t *)f.idx.prev)[k * 2 * B + (t - 6 - B)];
}

// 32/64-bit rasters: a twelve-bit length per UNIT of the segment (the unit-parallel decoder wants every unit's place).
// A thread per two fields: three whole bytes; the entry's threads share its fixed part a byte each.  tpe: threads per entry
__device__ __forceinline__ void ix_blw_fill(const IxFill &f, uint64_t idx, uint32_t tpe) {
    static_assert(IX_BL_BITS_WIDE == 12, "pairs of fields are three bytes");
    const uint32_t B = f.bands, tsz = f.tsz, upe = f.blocks * B;                // units per entry
    const uint64_t k = idx / tpe;
    if (k >= f.K) return;
    const uint32_t t = (uint32_t)(idx - k * tpe);
    const uint64_t u0 = k * upe, nunits = f.nblocks * B;
    uint32_t len[2] = {0, 0};
    for (uint32_t q = 0; q < 2; q++) {
        const uint32_t fd = 2 * t + q;
        if (fd < upe && u0 + fd < nunits) len[q] = f.ulen_sz == 1 ? (uint32_t)((const uint8_t *)f.idx.ulen)[u0 + fd] : (uint32_t)((const uint16_t *)f.idx.ulen)[u0 + fd];
    }
    const uint32_t bits = len[0] | len[1] << 12;
    uint8_t *e0 = ix_entry_ptr(f, k);
    const uint32_t fixed = 6 + B * (1 + tsz), nbytes = (upe * 12 + 7) / 8;
    uint8_t *e = e0 + fixed + 3 * t;
    for (uint32_t i = 0; i < 3; i++) if (3 * t + i < nbytes) e[i] = (uint8_t)(bits >> (8 * i));
    for (uint32_t i = t; i < fixed; i += tpe) {         // bit position, a rung byte per band, the entering values
        if (i < 6) e0[i] = (uint8_t)(f.idx.bitpos[k] >> (8 * i));
        else if (i < 6 + B) e0[i] = f.idx.rung[k * B + (i - 6)];
        else e0[i] = ((const uint8_t *)f.idx.prev)[k * B * tsz + (i - 6 - B)];
    }
}

// Common-factor streams of the lane-per-unit decoder (k_dec_pxu.hip): a three-byte field per UNIT of the entry's segment -- its bits (12)
// | the rung it is entered with << 12 -- from the index's unit table; a thread per four units, sixteen threads an entry (a segment is at
// most 64 units), which also share the entry's fixed part
__device__ __forceinline__ void ix_blu_best_fill(const IxFill &f, uint64_t idx) {
    const uint32_t B = f.bands, tsz = f.tsz, upe = f.blocks * B;                // units per entry
    const uint64_t k = idx >> 4;
    if (k >= f.K) return;
    const uint32_t t = (uint32_t)(idx & 15);
    const uint64_t u0 = k * upe, nunits = f.nblocks * B;
    uint8_t *e0 = ix_entry_ptr(f, k);
    const uint32_t fixed = 6 + B * (1 + 2 * tsz);
    if (4 * t + 4 <= upe) {     // four whole fields: three dwords
        uint32_t fl[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t fd = 4 * t + q;
            const uint32_t bt = u0 + fd < nunits ? ((const uint32_t *)f.idx.ulen)[u0 + fd] : 0u;
            fl[q] = (bt & 0xfffu) | ((bt >> 16) & 63u) << 12;
        }
        ix_store12(e0 + fixed + IX_BL_BEST_BYTES * 4 * t, fl);
    } else
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t fd = 4 * t + q;
            if (fd >= upe) break;
            const uint32_t bt = u0 + fd < nunits ? ((const uint32_t *)f.idx.ulen)[u0 + fd] : 0u;
            const uint32_t fld = (bt & 0xfffu) | ((bt >> 16) & 63u) << 12;
            uint8_t *e = e0 + fixed + IX_BL_BEST_BYTES * fd;
            e[0] = (uint8_t)fld; e[1] = (uint8_t)(fld >> 8); e[2] = (uint8_t)(fld >> 16);
        }
    for (uint32_t i = t; i < fixed; i += 16) {
        uint8_t v;
        if (i < 6) v = (uint8_t)(f.idx.bitpos[k] >> (8 * i));
        else if (i < 6 + B) v = f.idx.rung[k * B + (i - 6)];
        else if (i < 6 + B + B * tsz) v = ((const uint8_t *)f.idx.prev)[k * B * tsz + (i - 6 - B)];
        else v = ((const uint8_t *)f.idx.cf)[k * B * tsz + (i - 6 - B - B * tsz)];
        e0[i] = v;
    }
}

// The 16-bit check of chunk c's entries (ix_sum_part) by a workgroup of 256; part: four words of LDS.  Thread 0 gets the check.
__device__ __forceinline__ uint32_t ix_chunk_check(const IxFill &f, uint32_t c, uint32_t *part) {
    uint32_t s = ix_sum_part(ix_chunk_ptr(f, c) + IX_HEAD, ix_entries_here(f, c) * f.E, threadIdx.x, 256);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += (uint32_t)__shfl_xor((int)s, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    return ix_sum_fold(part[0] + part[1] + part[2] + part[3]);
}

}  // namespace qb3dev
