// qb3_amd/csrc/k_reindex.hip -- reindex: a restart table for a container that exists, without coding its stream again (qb3x_reindex_device).
// The walk of the plain stream has left a complete index in the decoder's workspace; reindex_fill_kernel writes the table's entries from it
// (the encoder's own fill code, qb3_ix_fill.h), reindex_finish_kernel everything else of the new container in ONE launch: the header bytes
// that are kept, every table chunk's head, pad and check, "DT", and the coded bytes moved from their old offset to their new one.
#include <cstring>
#include "qb3_kernels.h"
#include "qb3_ix_fill.h"

namespace qb3dev {

enum ReindexFill { RF_PLAIN = 0, RF_BL8, RF_BL_BEST, RF_BL16, RF_BLW, RF_BLU_BEST };

// the entries, a thread per piece of an entry as the layout's fill code counts them (tpe: ix_blw_fill's threads per entry)
__global__ void __launch_bounds__(256) reindex_fill_kernel(const IxFill f, const uint32_t kind, const uint32_t tpe) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    switch (kind) {         // (uniform)
    case RF_PLAIN: if (i < f.K) ix_plain_entry(f, i * f.spe, f.idx.bitpos[i * f.spe]); break;
    case RF_BL8: ix_bl_fill(f, i); break;
    case RF_BL_BEST: ix_bl_best_fill(f, i); break;
    case RF_BL16: ix_bl16_fill(f, i); break;
    case RF_BLW: ix_blw_fill(f, i, tpe); break;
    default: ix_blu_best_fill(f, i); break;
    }
}

// the same choice of layout as the encoder's (launch_enc_tables, k_enc_post.hip)
int launch_reindex_fill(const Geometry &g, void *index, const IxTable &ix, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!ix.base || !ix.K || !ix.per_chunk || !g.seg_blocks) { set_error("reindex: no table layout", 0); return -1; }
    IxFill f;
    f.idx = index_view(g, index); f.dst = ix.base; f.nblocks = g.nblocks; f.bands = g.bands; f.tsz = g.tsz; f.ulen_sz = g.ulen_sz;
    f.best = g.mode == CM_BEST ? 1u : 0u;
    f.K = ix.K; f.E = ix.entry_bytes; f.per_chunk = ix.per_chunk; f.blocks = ix.blocks; f.spe = ix.blocks / g.seg_blocks; f.bl = ix.block_lens ? 1u : 0u;
    f.px16_bg = g.tsz == 2 ? px16_bands_per_lane(g) : 0;
    uint32_t kind = RF_PLAIN, tpe = 1;
    uint64_t threads = ix.K;
    if (ix.block_lens) {
        if (lane_per_unit_shape(g.tsz, g.mode, g.bands)) {
            if (g.mode == CM_BEST) { kind = RF_BLU_BEST; threads = (uint64_t)ix.K * 16; }
            else { kind = RF_BLW; tpe = (ix.blocks * g.bands + 1) / 2; threads = (uint64_t)ix.K * tpe; }
        } else if (g.mode == CM_BEST) { kind = RF_BL_BEST; threads = (uint64_t)ix.K * 16; }
        else if (g.tsz == 1) { kind = RF_BL8; threads = (uint64_t)ix.K * 16; }
        else if (g.tsz == 2) { kind = RF_BL16; threads = (uint64_t)ix.K * (g.bands == 1 ? 16 : 32); }
        else { kind = RF_BLW; tpe = (ix.blocks * g.bands + 1) / 2; threads = (uint64_t)ix.K * tpe; }
    }
    ProfScope ps("reindex_fill", st);
    hipLaunchKernelGGL(reindex_fill_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, f, kind, tpe);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- the finish launch
constexpr uint32_t RX_HDR_MAX = 192;        // header bytes that travel in the kernel's arguments
constexpr int RX_NQ = 4;                    // sixteen-byte loads a lane has in flight
constexpr uint32_t RX_WG_LINES = 256 * RX_NQ;   // sixteen-byte lines of the destination a workgroup moves
struct ReindexArgs {
    IxFill f;                   // the table (f.K == 0: none)
    uint32_t nch;               // its chunks: the launch's first nch workgroups, one each
    uint32_t hdr_len;
    uint8_t *dst;               // the new container's first byte
    const uint8_t *src;         // the coded bytes' old place ...
    uint8_t *pay;               // ... and their new one
    uint64_t n;                 // how many
    uint8_t hdr[RX_HDR_MAX];
};

// bytes r .. r + 15 of the 32 bytes (lo, hi): r = 4 * ds + bs / 8
__device__ __forceinline__ uint4 rx_funnel(const uint4 &lo, const uint4 &hi, uint32_t ds, uint32_t bs) {
    uint32_t w[5];
    switch (ds) {           // (uniform: one shift for the whole launch)
    case 0: w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[4] = hi.x; break;
    case 1: w[0] = lo.y; w[1] = lo.z; w[2] = lo.w; w[3] = hi.x; w[4] = hi.y; break;
    case 2: w[0] = lo.z; w[1] = lo.w; w[2] = hi.x; w[3] = hi.y; w[4] = hi.z; break;
    default: w[0] = lo.w; w[1] = hi.x; w[2] = hi.y; w[3] = hi.z; w[4] = hi.w; break;
    }
    return make_uint4(__builtin_amdgcn_alignbit(w[1], w[0], bs), __builtin_amdgcn_alignbit(w[2], w[1], bs),
                      __builtin_amdgcn_alignbit(w[3], w[2], bs), __builtin_amdgcn_alignbit(w[4], w[3], bs));
}

// Workgroup c < nch: chunk c of the table, whose entries reindex_fill_kernel wrote -- their check, the head, the pad, "DT" behind the last.
// Workgroup nch: the header bytes, and the few coded bytes in front of and behind the destination's whole sixteen-byte lines.
// The others: the coded bytes, as enc_concat_kernel moves a chunk: old and new offset differ by the table's size, so the source of an
// aligned line of the destination stands at any byte; a lane loads aligned sixteen bytes (RX_NQ loads in flight), takes the sixteen
// behind them from the next lane, funnel-shifts the 32 by the byte distance and stores a whole line.
__global__ void __launch_bounds__(256) reindex_finish_kernel(const ReindexArgs a) {
    __shared__ uint32_t part[4];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < a.nch) {
        const uint32_t check = ix_chunk_check(a.f, blockIdx.x, part);
        if (tid == 0) ix_write_head(a.f, blockIdx.x, check);
        return;
    }
    // lines: the destination's aligned sixteen-byte pieces that lie wholly inside the coded bytes
    const uint64_t head = a.n < 16 ? a.n : (uint64_t)((16 - ((uintptr_t)a.pay & 15)) & 15);     // bytes in front of the first line
    const uint64_t nlines = (a.n - head) >> 4;
    if (blockIdx.x == a.nch) {
        for (uint32_t i = tid; i < a.hdr_len; i += blockDim.x) a.dst[i] = a.hdr[i];
        const uint64_t tail0 = head + 16 * nlines;
        for (uint64_t i = tid; i < head; i += blockDim.x) a.pay[i] = a.src[i];
        for (uint64_t i = tail0 + tid; i < a.n; i += blockDim.x) a.pay[i] = a.src[i];
        return;
    }
    const uint8_t *s0 = a.src + head;               // the first line's source
    const uint32_t r = (uint32_t)((uintptr_t)s0 & 15), ds = r >> 2, bs = 8 * (r & 3);
    const uint4 *src4 = (const uint4 *)(s0 - r);    // aligned vector v holds source bytes 16 v - r .. of the lines
    uint4 *dst4 = (uint4 *)(a.pay + head);
    const uint64_t nvec = (16 * nlines + r + 15) >> 4;      // vectors that hold a byte of the lines: none is loaded behind them
    const uint32_t lane = tid & 63;
    const uint64_t base = (uint64_t)(blockIdx.x - a.nch - 1) * RX_WG_LINES + (uint64_t)(tid >> 6) * (64 * RX_NQ);
    if (base >= nlines) return;                     // (wave uniform)
    uint4 cur[RX_NQ], last = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < RX_NQ; q++) {
        const uint64_t v = base + 64 * q + lane;
        cur[q] = v < nvec ? src4[v] : make_uint4(0, 0, 0, 0);
    }
    if (lane == 63 && base + 64 * RX_NQ < nvec) last = src4[base + 64 * RX_NQ];      // the vector behind the wave's last
#pragma unroll
    for (int q = 0; q < RX_NQ; q++) {
        const uint4 wrap = q + 1 < RX_NQ ? cur[q + 1 < RX_NQ ? q + 1 : q] : last;   // lane 63's neighbour: lane 0 of the next round
        uint4 nxt;
        nxt.x = (uint32_t)__shfl_down((int)cur[q].x, 1, 64); nxt.y = (uint32_t)__shfl_down((int)cur[q].y, 1, 64);
        nxt.z = (uint32_t)__shfl_down((int)cur[q].z, 1, 64); nxt.w = (uint32_t)__shfl_down((int)cur[q].w, 1, 64);
        uint4 w0;
        w0.x = (uint32_t)__shfl((int)wrap.x, q + 1 < RX_NQ ? 0 : 63, 64); w0.y = (uint32_t)__shfl((int)wrap.y, q + 1 < RX_NQ ? 0 : 63, 64);
        w0.z = (uint32_t)__shfl((int)wrap.z, q + 1 < RX_NQ ? 0 : 63, 64); w0.w = (uint32_t)__shfl((int)wrap.w, q + 1 < RX_NQ ? 0 : 63, 64);
        if (lane == 63) nxt = w0;
        const uint64_t line = base + 64 * q + lane;
        if (line < nlines) dst4[line] = r ? rx_funnel(cur[q], nxt, ds, bs) : cur[q];
    }
}

// hdr: the kept header bytes (host memory; "DT" included when there is no table); ix: the table at ix.base = d_dst + hdr_len, K == 0: none;
// d_pay: where the n coded bytes at d_src go.  Does not synchronise.
int launch_reindex_finish(const Geometry &g, const IxTable &ix, const uint8_t *hdr, size_t hdr_len, void *d_dst, const void *d_src, void *d_pay, uint64_t n, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    ReindexArgs a;
    memset(&a, 0, sizeof(a));
    a.nch = 0;
    if (ix.base && ix.K) {
        a.f.dst = ix.base; a.f.K = ix.K; a.f.E = ix.entry_bytes; a.f.per_chunk = ix.per_chunk; a.f.blocks = ix.blocks; a.f.bl = ix.block_lens ? 1u : 0u;
        a.f.best = g.mode == CM_BEST ? 1u : 0u;
        a.nch = (uint32_t)ix_chunks(ix);
    }
    a.dst = (uint8_t *)d_dst; a.src = (const uint8_t *)d_src; a.pay = (uint8_t *)d_pay; a.n = n;
    if (hdr_len <= RX_HDR_MAX) { a.hdr_len = (uint32_t)hdr_len; memcpy(a.hdr, hdr, hdr_len); }
    else HIPCHK(hipMemcpyAsync(d_dst, hdr, hdr_len, hipMemcpyHostToDevice, st));      // (foreign chunks in the header: a copy of its own)
    const uint64_t head = n < 16 ? n : (uint64_t)((16 - ((uintptr_t)d_pay & 15)) & 15), nlines = (n - head) >> 4;
    const uint64_t wgs = (nlines + RX_WG_LINES - 1) / RX_WG_LINES;
    if (a.nch + 1 + wgs > 0x7fffffffull) { set_error("reindex: container too large for one launch", 0); return -1; }
    ProfScope ps("reindex_finish", st);
    hipLaunchKernelGGL(reindex_finish_kernel, dim3((uint32_t)(a.nch + 1 + wgs)), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
