// qb3_amd/csrc/qb3_win.h -- what the window kernels of every family share (qb3_dev.h lists the families): the per-window numbers, the
// arguments and the split of a batch into launches, the two sources a wave reads from, the check of the table's end, and -- at the
// end -- the kernel SHELLS, one per form, that every family instantiates over its wave routine (three every family has, and the mosaic
// shell, which a family has once it is instantiated for it: the 8-bit one, k_dec_wins_mosaic.hip).  Then the 8-bit family's own:
// the wave's work (a segment decoded from its table entry, its blocks clipped to the window and stored) and its instantiations.
// The comment at the head of k_dec_win.hip describes mapping, clipping and trust.
#pragma once
#include <type_traits>
#include "../../include/qb3x.h"
#include "qb3_px.h"

namespace qb3dev {

// A window on the device: 64 bytes.  The single call passes it as a kernel argument, a batch as an array in device memory
struct WinDesc {
    uint8_t *dst;                   // the window's first byte
    uint64_t dstride;               // bytes between the window's rows
    uint32_t wx0, wy0, wx1, wy1;    // the window in raster pixels: [wx0, wx1) x [wy0, wy1)
    uint32_t bx0, bx1, by0, by1;    // ... in blocks, both ends included
    uint32_t per_row, nwaves;       // waves per block row of the window; rows * per_row
    uint32_t wave0;                 // a batch: waves of the launch in front of this window's (the exclusive prefix of nwaves)
    uint32_t pad_;
};
static_assert(sizeof(WinDesc) == 64, "WinDesc is read with scalar loads of sixteen dwords");

// the window's blocks by the geometry rule (pixel x is held by block min(x / 4, nbx - 1)) and the waves that decode them; the
// caller has checked that the window is not empty and lies inside the raster
inline void window_desc(const Geometry &g, const WinRect &r, void *dst, WinDesc *w) {
    w->dst = (uint8_t *)dst; w->dstride = r.stride * g.tsz;
    w->wx0 = r.x0; w->wy0 = r.y0; w->wx1 = r.x0 + r.w; w->wy1 = r.y0 + r.h;
    const WinBlocks b = window_blocks(g, r.x0, r.y0, r.w, r.h);
    w->bx0 = b.bx0; w->bx1 = b.bx1; w->by0 = b.by0; w->by1 = b.by1;
    // the most segments the run of bx1 - bx0 + 1 blocks of a row touches: it starts anywhere in a segment, unless rows start where segments do
    // (NB blocks a segment: 64 for the two 8-bit families, 64 / band groups for the 16-bit one, 64 / bands for the lane-per-unit ones)
    const uint32_t n = w->bx1 - w->bx0 + 1, NB = g.seg_blocks;
    w->per_row = (g.nbx % NB == 0) ? (w->bx0 % NB + n - 1) / NB + 1 : (n + NB - 2) / NB + 1;
    w->nwaves = (w->by1 - w->by0 + 1) * w->per_row;
    w->wave0 = 0; w->pad_ = 0;
}
// what a window kernel takes from the raster, the stream and the table (status: the word ix_check_chunk and ix_tail_check raise bits in)
void window_dec_args(DecArgs &a, const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                     uint32_t *status, const IxTable &ix);
// ... and the selection of a band-selected batch (sel: nsel band numbers, 1 <= nsel <= 16), for the SEL instantiations of qb3_win_unit.h
inline void window_sel_dec_args(DecArgs &a, const uint8_t *sel, uint32_t nsel) {
    a.sel_nibs = 0;
    for (uint32_t k = 0; k < nsel; k++) a.sel_nibs |= (uint64_t)(sel[k] & 15u) << (4 * k);
    a.nsel = nsel; a.magic_nsel = magic_div(nsel);
}

// what the single shell takes (win_one_kernel) ...
struct WinArgs {
    DecArgs d;                      // stream, table, status word, staging capacity: as dec_px_kernel takes them
    WinDesc w;                      // the window: destination, rectangle in pixels and blocks, waves (qb3_win.h)
    uint32_t chk0, chk_n;           // table chunks the launch's first chk_n workgroups check, from chunk chk0
    uint32_t tail_chunk;            // the workgroup behind them checks the table's last chunk too (it is not one of those)
};
// ... and the batch shell (win_batch_kernel)
struct WinBatchArgs {
    DecArgs d;                      // stream, table, staging capacity; d.status: the call-wide word
    const WinDesc *wins;            // the launch's windows, wave0 counted from the launch's first window
    uint32_t *wstatus;              // ... their status words
    const uint32_t *chunks;         // table chunks to check, chk_n of them (the first launch of a call only)
    uint32_t nwin, chk_n, tail;     // tail: a workgroup behind the chunk checks does the tail check
};
// fills wa for one window (status: zeroed by the caller's launch) and returns the launch's workgroups: the chunk checks, the table's end, the waves
uint32_t window_launch_args(WinArgs &wa, const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                            void *dst, const WinRect &r, uint32_t *status, const IxTable &ix);
// the launches of a batch, ranged or not (one, unless the waves exceed WIN_LAUNCH_WAVES: window_batch_plan's prefixes start again there):
// the windows of each are put into args, then launch(grid, head) makes it -- `front` workgroups in the first launch of the call (head:
// the table's checks), none in the later ones, then a workgroup for every four waves
template <class Args, class Launch>
inline void window_launches(Args &args, const void *h_descs, const void *d_descs, size_t n, uint32_t *d_status, uint32_t front, Launch launch) {
    const WinDesc *h = (const WinDesc *)h_descs;
    for (size_t first = 0; first < n;) {
        size_t end = first + 1;
        while (end < n && h[end].wave0 != 0) end++;
        const uint64_t waves = (uint64_t)h[end - 1].wave0 + h[end - 1].nwaves;
        args.wins = (const WinDesc *)d_descs + first; args.wstatus = d_status + 1 + first; args.nwin = (uint32_t)(end - first);
        launch((uint32_t)((first ? 0 : front) + (waves + 3) / 4), first == 0);
        first = end;
    }
}

// position of the table's last entry against the stream's length: a stream that ends before its last segment starts was cut short
__device__ __forceinline__ void ix_tail_check(const DecArgs &a) {
    const uint8_t *e = ix_entry_at(a.ix, a.ix_per_chunk, a.ix_E, a.ix_pad, a.ix_K - 1);
    uint64_t v = 0;
#pragma unroll
    for (uint32_t i = 0; i < 6; i++) v |= (uint64_t)e[i] << (8 * i);
    if (v > a.in_bits) atomicOr(a.status, 4u);
}

// Where a wave's table entries and stream words come from: a SOURCE POLICY, the one thing the window kernels differ in.
//   find(seg, wanted)   wave uniform, before any entry is read: true when the source holds segment seg (wanted: the wave is live);
//   entry(a, k)         entry k of the table, for k = seg and seg + 1 of a segment find() said yes to (and for segment 0 of any wave);
//   holds(w0, ndw)      are the stream words [w0, w0 + ndw) (counted from a.in32's word) the source's to read;
//   word(a, w, endw)    stream word w of a range holds() said yes to; zero at and behind word endw, the container's end.
// The contiguous source: the whole container in device memory (dec_win_kernel, dec_wins_kernel) -- every segment, every word.
struct WinSrcContig {
    __device__ __forceinline__ bool find(uint32_t, bool) { return true; }
    __device__ __forceinline__ const uint8_t *entry(const DecArgs &a, uint32_t k) const { return ix_entry_at(a.ix, a.ix_per_chunk, a.ix_E, a.ix_pad, k); }
    __device__ __forceinline__ bool holds(uint64_t, uint64_t) const { return true; }
    __device__ __forceinline__ uint32_t word(const DecArgs &a, uint64_t w, uint64_t endw) const { return w < endw ? a.in32[w] : 0u; }
};
// The ranged source (k_dec_wins_ranged.hip): PIECES of the stream packed back to back, a compact array of the entries their segments
// use, and a list of the pieces sorted by first segment.  A piece is a run of consecutive segments whose bytes were fetched as one
// range: eight dwords { first segment, segments, index of its first entry in the compact array (it has segments + 1: the entry behind
// the run ends it), index of its first word in the packed buffer, the stream word that word is (low, high), words, 0 }.  Nothing is
// read outside the piece and the piece's entries, whatever the entries say: a segment that is not wholly inside its piece does not
// "hold" and stages zeros, as one that exceeds the staging area does.
struct WinPiece { uint32_t seg0, nseg, ent0, word0, sw0_lo, sw0_hi, nwords, pad_; };
static_assert(sizeof(WinPiece) == 32, "WinPiece is read with scalar loads of eight dwords");
struct WinSrcPieces {
    const WinPiece *pieces;         // npieces >= 1 of them, seg0 growing strictly
    const uint8_t *ents;            // the compact array, entries of a.ix_E bytes
    const uint32_t *words;          // the packed pieces
    uint32_t npieces;
    WinPiece pc;                    // the wave's piece (after find)
    __device__ __forceinline__ bool find(uint32_t seg, bool wanted) {
        // the last piece whose first segment is not behind seg: wave uniform, as the window search of k_dec_wins.hip
        uint32_t lo = 0, hi = npieces;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pieces[mid].seg0 <= seg) lo = mid; else hi = mid;
        }
        lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
        pc = pieces[lo];
        const bool in = seg >= pc.seg0 && seg - pc.seg0 < pc.nseg;
        if (!in) { pc = pieces[0]; pc.nwords = 0; }      // (entry() then gives the array's first two entries: inside it, never used)
        return in || !wanted;
    }
    __device__ __forceinline__ const uint8_t *entry(const DecArgs &a, uint32_t k) const {
        const uint32_t j = k - pc.seg0;                 // 0 .. nseg for a segment of the piece
        return ents + (uint64_t)(pc.ent0 + (j <= pc.nseg ? j : 0u)) * a.ix_E;
    }
    __device__ __forceinline__ bool holds(uint64_t w0, uint64_t ndw) const {
        const uint64_t sw0 = (uint64_t)pc.sw0_hi << 32 | pc.sw0_lo;
        return w0 >= sw0 && w0 - sw0 <= pc.nwords && ndw <= pc.nwords - (w0 - sw0);
    }
    __device__ __forceinline__ uint32_t word(const DecArgs &, uint64_t w, uint64_t) const {
        return words[pc.word0 + (uint32_t)(w - ((uint64_t)pc.sw0_hi << 32 | pc.sw0_lo))];      // (behind the container's end a piece has no words: holds() said no)
    }
};
// what the ranged shell takes (win_ranged_kernel)
struct WinRangedArgs {
    DecArgs d;                      // geometry, stream length, staging capacity, entry size; d.in32 and d.ix are not used
    const WinDesc *wins;            // the launch's windows, wave0 counted from the launch's first window
    uint32_t *wstatus;              // ... their status words
    WinSrcPieces src;               // pieces, entries, packed words
    uint32_t nwin;
};

// The SHELLS (the mosaic one stands with its arguments, further down): what surrounds a family's wave routine in each form.  F names one instantiation of a family (WinU8 below, Win16,
// WinCf8, WinUnit, WinCfu next to their wave routines): F::contig and F::pieces are the routine with the instantiation's template
// arguments over the two sources, F::waves is the second number of the launch bounds (0: none given, the attributes are those of
// __launch_bounds__(256)).  The two are constants of function type, so a shell calls the routine itself: with a forwarding function
// in between, the four-band kernels of the 8-bit common-factor family took 96 registers and 8 bytes of scratch where they have 90
// and none.
// A family's pick(g, plan, visit) calls visit(F()) for the instantiation the geometry and the plan select; win_launch(f, args, l)
// launches the shell over it that takes args.

// the last window whose first wave is not behind gw (wave0 grows strictly: every window has a wave; window 0 starts at 0); gw and all
// of the search are wave uniform.  A wave behind the last window's waves lands in the last window and leaves there (wid >= nwaves).
__device__ __forceinline__ uint32_t win_search(const WinDesc *wins, uint32_t nwin, uint32_t gw) {
    uint32_t lo = 0, hi = nwin;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (wins[mid].wave0 <= gw) lo = mid; else hi = mid;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
}
// one window, as kernel arguments (no descriptor goes up for a single call)
template <class F>
__global__ void __launch_bounds__(256, F::waves) win_one_kernel(const WinArgs wa) {
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
    F::contig(a, wa.w, a.status, smem, wave, (blockIdx.x - wa.chk_n - 1) * 4 + wave, WinSrcContig());
}
// a batch: the window found in the descriptor array, a status word per window
template <class F>
__global__ void __launch_bounds__(256, F::waves) win_batch_kernel(const WinBatchArgs ba) {
    const DecArgs &a = ba.d;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (blockIdx.x < ba.chk_n) {                        // the launch's first workgroups: a chunk of the container's table each
        ix_check_chunk(a, ba.chunks[blockIdx.x], (uint32_t *)smem);
        return;
    }
    if (blockIdx.x < ba.chk_n + ba.tail) {              // ... and one for the table's end
        if (threadIdx.x == 0) ix_tail_check(a);
        return;
    }
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t gw = (blockIdx.x - ba.chk_n - ba.tail) * 4 + wave;
    const uint32_t i = win_search(ba.wins, ba.nwin, gw);
    const WinDesc w = ba.wins[i];                       // sixteen dwords, read before anything is stored
    F::contig(a, w, ba.wstatus + i, smem, wave, gw - w.wave0, WinSrcContig());
}
// a batch from pieces: no check workgroups (the host verified the chunks before a byte of the stream was asked for)
template <class F>
__global__ void __launch_bounds__(256, F::waves) win_ranged_kernel(const WinRangedArgs ra) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t gw = blockIdx.x * 4 + wave;
    const uint32_t i = win_search(ra.wins, ra.nwin, gw);
    const WinDesc w = ra.wins[i];
    F::pieces(ra.d, w, ra.wstatus + i, smem, wave, gw - w.wave0, ra.src);
}
// What the mosaic shell takes (win_mosaic_kernel): a batch whose windows are PIECES, each in a container of its own (qb3_dev.h, "Mosaic windows")
struct WinMosaicArgs {
    DecArgs d;                      // tile 0's: geometry, table shape, in_bit0, staging capacity; d.in32, d.in_bits, d.ix and d.status are not used
    const WinDesc *wins;            // the launch's pieces, wave0 counted from the launch's first piece; pad_: the piece's tile
    uint32_t *wstatus;              // ... their status words
    const WinTile *tiles;           // stream, stream length and table of every tile a piece names
    uint32_t *tstatus;              // ... their status words (a failed check)
    const WinTileCheck *checks;     // (tile, table chunk) pairs to check, chk_n of them (the first launch of a call only)
    uint32_t nwin, chk_n;
    uint32_t ix_off, mode_byte;     // tile 0's: offset of the first "ix" chunk in a container, the mode byte
};
// A batch over many containers of one shape: the batch shell with the three fields of DecArgs that differ between tiles taken from the
// piece's tile, in a LOCAL copy of the arguments (DecArgs does not grow for it).  The piece's tile number and the tile's record are wave
// uniform: scalar loads.
// (Launch bounds: a family that gives none gets 8 waves a SIMD here.  Left to itself the compiler takes 69 vector registers and 7 waves for
// the 8-bit family where the batch shell has 64 and 8; asked for 8 it needs 53 to 62 and no scratch.)
template <class F>
__global__ void __launch_bounds__(256, F::waves ? F::waves : 8) win_mosaic_kernel(const WinMosaicArgs ma) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (blockIdx.x < ma.chk_n) {                        // the launch's first workgroups: a chunk of one tile's table each
        const WinTileCheck c = ma.checks[blockIdx.x];
        const WinTile t = ma.tiles[c.tile];
        DecArgs a = ma.d;
        a.in32 = t.in32; a.in_bits = t.in_bits; a.ix = t.ix; a.status = ma.tstatus + c.tile;
        // (with check_heads on this also holds the tile to tile 0's "ix" tag at every chunk checked and to the "DT" mark behind the last)
        ix_check_chunk(a, c.chunk & ~WIN_TILE_TAIL, (uint32_t *)smem);
        if ((c.chunk & WIN_TILE_TAIL) && threadIdx.x == 0) {    // ... with the tile's last chunk: the table's end, and the one thing the chunks do not say -- the mode byte
            ix_tail_check(a);
            if ((t.ix - ma.ix_off)[10] != ma.mode_byte) atomicOr(a.status, 64u);
        }
        return;
    }
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t gw = (blockIdx.x - ma.chk_n) * 4 + wave;
    const uint32_t i = win_search(ma.wins, ma.nwin, gw);
    const WinDesc w = ma.wins[i];                       // sixteen dwords, read before anything is stored
    const WinTile t = ma.tiles[w.pad_];
    DecArgs a = ma.d;
    a.in32 = t.in32; a.in_bits = t.in_bits; a.ix = t.ix;
    F::contig(a, w, ma.wstatus + i, smem, wave, gw - w.wave0, WinSrcContig());
}
template <class F> inline void win_launch(F, const WinMosaicArgs &ma, const WinLaunch &l) {
    hipLaunchKernelGGL((win_mosaic_kernel<F>), dim3(l.grid), dim3(256), l.lds, (hipStream_t)l.stream, ma);
}
template <class F> inline void win_launch(F, const WinArgs &wa, const WinLaunch &l) {
    hipLaunchKernelGGL((win_one_kernel<F>), dim3(l.grid), dim3(256), l.lds, (hipStream_t)l.stream, wa);
}
template <class F> inline void win_launch(F, const WinBatchArgs &ba, const WinLaunch &l) {
    hipLaunchKernelGGL((win_batch_kernel<F>), dim3(l.grid), dim3(256), l.lds, (hipStream_t)l.stream, ba);
}
template <class F> inline void win_launch(F, const WinRangedArgs &ra, const WinLaunch &l) {
    hipLaunchKernelGGL((win_ranged_kernel<F>), dim3(l.grid), dim3(256), l.lds, (hipStream_t)l.stream, ra);
}
// for the picks: a band count and a band map as types
template <int N> using WinInt = std::integral_constant<int, N>;
// for the records: destinations on any address, on a value; the LDS of the families that bring dec_px_kernel's
inline uint32_t window_align_any(const Geometry &) { return 1; }
inline uint32_t window_align_value(const Geometry &g) { return g.tsz; }
inline size_t window_lds_px(const Geometry &, const DecPlan &plan) { return plan.lds_px; }

// Wave `wid` of window w (wave: its number in the workgroup of four; both wave uniform): the k-th segment of one of the window's block
// rows, decoded as dec_px_kernel's BL branch does, stored where the window's blocks go.  status: the word this window's failures go to.
// Every wave of the workgroup comes here (there is one workgroup barrier); smem: the launch's dynamic LDS, at LDS address 0.
template <int B, bool RGB, uint64_t ORDER, bool STEP, class SRC = WinSrcContig>
__device__ __forceinline__ void win_decode_wave(const DecArgs &a, const WinDesc &w, uint32_t *status, uint8_t *smem, uint32_t wave, uint32_t wid, SRC src = SRC()) {
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
    const uint32_t row0 = (w.by0 + r) * nbx;           // (nblocks <= 2^28)
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
    uint32_t rg0[B], pv0[B], blen = 0;
    {
        const uint8_t *e = src.entry(a, segc);
        auto pos6 = [](const uint8_t *q) { uint64_t v = 0;
#pragma unroll
            for (uint32_t i = 0; i < 6; i++) v |= (uint64_t)q[i] << (8 * i);
            return v; };
        P0 = pos6(e);
        P1 = ((uint64_t)segc + 1 < a.g.nseg) ? pos6(src.entry(a, segc + 1)) : a.in_bits;
#pragma unroll
        for (int c = 0; c < B; c++) { rg0[c] = e[6 + c] & 7u; pv0[c] = e[6 + B + c]; }
        const uint8_t *bl = e + 6 + 2 * B + ((IX_BL_BITS * lane) >> 3);
        blen = act ? (((uint32_t)bl[0] | (uint32_t)bl[1] << 8) >> ((IX_BL_BITS * lane) & 7)) & ((1u << IX_BL_BITS) - 1) : 0u;
    }
    for (uint32_t i = tid; i < 256; i += blockDim.x) ((uint4 *)tab)[i] = ((const uint4 *)px_dec_tab.e)[i];
    __syncthreads();                                    // the only workgroup barrier
    if (!live) {
        if (!placed && lane == 0) atomicOr(status, 8u);
        return;
    }
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
    const uint32_t binc = wave_iscan32(blen);           // inclusive: lane 63 holds the bits of the segment
    uint32_t pos = cpos + binc - blen;
    uint32_t rp[B][8], spk[NW], sinc[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) spk[j] = 0;
    // band after band: the switch, the band's rungs across the segment (a scan of the switches), the unit, and where it
    // ended is where the next band's unit starts
    const uint32_t blk_end = pos + blen;
    // (the unit decodes from what the switch left of its bits -- not with four bands and no step: that kernel takes 72 registers
    // with it, 7 waves a SIMD, and 64 without)
    constexpr bool CARRY = B != 4 || STEP;
#pragma unroll
    for (int c = 0; c < B; c++) {
        pos = pos < limit ? pos : limit;
        bool sig; uint32_t csl, sw;
        const uint32_t d = px_switch(pos, &csl, &sig, &sw);
        if (act && sig && STEP) bad = true;             // common-factor / index unit: not handled here
        const uint32_t rung = (rg0[c] + wave_iscan32(act ? d : 0u)) & 7u;
        uint32_t end;
        const uint32_t tot = px_group<STEP, CARRY>(pos + csl, rung, rp[c], &end, sw) & 0xffu;
        spk[c >> 1] |= (act ? tot : 0u) << (16 * (c & 1));
        pos = end;
    }
    if (act && pos != blk_end) bad = true;              // the table's lengths are not this stream's
#pragma unroll
    for (int j = 0; j < NW; j++) sinc[j] = wave_iscan32(spk[j]);

    const uint32_t g = g0 + lane, by = g / nbx, bx = g - by * nbx;
    if (act && bx >= w.bx0 && bx <= w.bx1 && by >= w.by0 && by <= w.by1) {
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

// The 8-bit family's instantiations (k_dec_win.hip, k_dec_wins.hip, k_dec_wins_ranged.hip), by the raster's bands, the plan's band
// map, the raster's order and mode
template <int B, bool RGB, uint64_t ORDER, bool STEP>
struct WinU8 {
    static constexpr int waves = 0;
    static constexpr auto contig = &win_decode_wave<B, RGB, ORDER, STEP, WinSrcContig>;
    static constexpr auto pieces = &win_decode_wave<B, RGB, ORDER, STEP, WinSrcPieces>;
};
template <class Visit>
inline void win_u8_pick(const Geometry &g, const DecPlan &plan, Visit visit) {
    const bool step = g.mode != CM_FTL, z = g.order == ZCURVE;
    auto go = [&](auto bc, auto rgbc) {
        constexpr int B = decltype(bc)::value;
        constexpr bool RGB = decltype(rgbc)::value;
        if (!z && !step) visit(WinU8<B, RGB, HILBERT, false>());
        else if (!z && step) visit(WinU8<B, RGB, HILBERT, true>());
        else if (z && !step) visit(WinU8<B, RGB, ZCURVE, false>());
        else visit(WinU8<B, RGB, ZCURVE, true>());
    };
    if (g.bands == 1) go(WinInt<1>(), std::false_type());
    else if (g.bands == 3) { if (plan.px_rgb) go(WinInt<3>(), std::true_type()); else go(WinInt<3>(), std::false_type()); }
    else { if (plan.px_rgb) go(WinInt<4>(), std::true_type()); else go(WinInt<4>(), std::false_type()); }
}
// ... and its dispatchers, one a file
void win_u8_one(const Geometry &g, const DecPlan &plan, const WinArgs &wa, const WinLaunch &l);
void win_u8_batch(const Geometry &g, const DecPlan &plan, const WinBatchArgs &ba, const WinLaunch &l);
void win_u8_ranged(const Geometry &g, const DecPlan &plan, const WinRangedArgs &ra, const WinLaunch &l);
void win_u8_mosaic(const Geometry &g, const DecPlan &plan, const WinMosaicArgs &ma, const WinLaunch &l);

}  // namespace qb3dev
