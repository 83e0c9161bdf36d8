// qb3_amd/csrc/k_dec_launch.hip -- the decoder's route, decided once: which kernel decodes the units (DecKernel), what runs in front of
// it to make the index it needs (DecFront), and launch_decode, which makes the launches in that order.  The predicates the host asks
// before it calls (decode_strips_ok, walk_table_applies; decode_window_ok in k_dec_win.hip) are answers of the same two functions.
// tests/test_decode_routes.py pins every route on the CPU.
#include "qb3_kernels.h"
#include "qb3_walk.h"

namespace qb3dev {

// ---- the kernel.  plan_decode says which kernels apply to the geometry; their shapes do not overlap, so at most one FTL / BASE and one
// common-factor flag is set.  What is left to say here is the alignment each needs: the 16-bit kernel a halfword-aligned image pointer
// (it does not look at the tile pitch), the 32/64-bit and the lane-per-unit kernels value-aligned pointer and pitch.
DecKernel pick_dec_kernel(const Geometry &g, const DecPlan &plan, const void *img, uint64_t pitch) {
    const bool ptr_aligned = ((uintptr_t)img & (g.tsz - 1)) == 0, val_aligned = ptr_aligned && !(pitch & (g.tsz - 1));
    if (g.mode == CM_BEST) {
        if (plan.pxw_best && val_aligned) return DecKernel::pxw_best;
        if (plan.pxu_best && val_aligned) return DecKernel::pxu_best;
        return plan.px_best && g.tsz == 1 ? DecKernel::px_best : DecKernel::generic;
    }
    if (plan.px && g.tsz == 1) return DecKernel::px;
    if (plan.px16 && g.tsz == 2 && ptr_aligned) return DecKernel::px16;
    if (plan.pxw && val_aligned) return DecKernel::pxw;
    if (plan.pxu && plan.fast && val_aligned) return DecKernel::pxu;
    return DecKernel::generic;
}

// the only place the unit decoders' launchers are named.  scope: the profile name (null: "dec_units", or "dec_segments" where the
// generic kernel gives a lane a segment)
static void launch_dec_kernel(DecKernel k, const DecArgs &a, const DecPlan &plan, hipStream_t st, const char *scope = nullptr) {
    ProfScope ps(scope ? scope : k != DecKernel::generic || (plan.fast && a.g.mode != CM_BEST) ? "dec_units" : "dec_segments", st);
    static void (*const launcher[])(const DecArgs &, const DecPlan &, hipStream_t) = {       // in DecKernel's order
        launch_dec_generic, launch_dec_px, launch_dec_px16, launch_dec_pxw, launch_dec_pxu, launch_dec_px_best, launch_dec_pxw_best, launch_dec_pxu_best };
    launcher[(int)k](a, plan, st);
}

// ---- the front.  What a container's restart table is to the decoder: usable (it matches this geometry and this library's segments), an
// entry per index segment, and with block fields that no switch forbids (then the wave-per-segment decoders work from the entries alone)
struct TableShape { bool usable = false, per_segment = false, block_fields = false; };
static TableShape table_shape(const Geometry &g, const IxTable &ix) {
    TableShape t;
    t.usable = ix.base && ix.blocks && ix.per_chunk && ix.blocks % g.seg_blocks == 0 && ix.entry_bytes == ix_entry_bytes(g, ix.block_lens) &&
               (!ix.block_lens || (ix_block_lens_ok(g) && ix.blocks == g.seg_blocks)) && ix.K == (g.nblocks + ix.blocks - 1) / ix.blocks;
    t.per_segment = t.usable && ix.blocks == g.seg_blocks;
    t.block_fields = t.per_segment && ix.block_lens && !tuning().slow_index && !tuning().no_bl;
    return t;
}

// what runs in front of the unit decoder when no index is handed in
enum class DecFront {
    none,           // an index was handed in
    pieces,         // nothing either: the lane-per-segment decoder takes the pieces between the table's entries as its segments (DecArgs::from_ix)
    entries,        // nothing either: the decoder works from the table's entries and their block fields (DecArgs::bl_mode)
    table_lanes,    // a lane per table entry walks the unit lengths (launch_dec_walk); entering values by totals + scan unless an entry is a segment
    table_walk,     // plain FTL / BASE stream with walk memory: the table of lengths by position (launch_dec_walk_table), then totals + scan
    // plain common-factor streams, a ladder: every rung may pass to the next one at run time
    best_exits,     //   the walk by exits (launch_dec_walk_best; false: not taken), then the scan
    best_chain,     //   the chain, the walking lane parsing the signal units (needs walk_chain_lds_ok()), then totals + scan
    best_wave,      //   one wave walks the lengths (launch_dec_index_walk_best), then totals + scan
    serial          // one lane parses the stream, values included
};
// plain common-factor streams of several bands that walk by the chain (k_dec_walk_chain.hip, walk_chainN_kernel<UB, true>): 8- and 16-bit
// rasters of the lane-per-unit decoder, and 8-bit RGBA (grey and RGB go by exits)
static bool best_chain_applies(const Geometry &g, const DecPlan &plan) {
    return g.mode == CM_BEST && g.tsz <= 2 && g.bands >= 2 && (plan.pxu_best || (plan.px_best && g.tsz == 1 && g.bands == 4));
}
// the first rung of that ladder at or below `from` that applies (exits: one band of any width, two or three bands of 8-bit data)
static DecFront best_rung(DecFront from, const Geometry &g, const DecPlan &plan, bool walk_memory_ok, bool wave_ok) {
    if (from <= DecFront::best_exits && walk_memory_ok && (g.bands == 1 || ((g.bands == 3 || g.bands == 2) && g.tsz == 1))) return DecFront::best_exits;
    if (from <= DecFront::best_chain && walk_memory_ok && best_chain_applies(g, plan)) return DecFront::best_chain;
    return from <= DecFront::best_wave && wave_ok ? DecFront::best_wave : DecFront::serial;
}
// walk_memory_ok: the caller brought enough table memory and QB3_SLOW_WALK is off; wave_ok: dec_index_walk_best_ok
static DecFront pick_dec_front(const Geometry &g, const DecPlan &plan, DecKernel k, bool have_index, const TableShape &t, bool walk_memory_ok, bool wave_ok) {
    const bool best = g.mode == CM_BEST, unit_parallel = plan.fast && !best;
    const bool wide = unit_parallel && g.tsz >= 4;          // 32/64-bit FTL / BASE: whatever kernel decodes, it takes unit lengths from entries and walks
    if (have_index) return DecFront::none;
    if (t.block_fields && (k != DecKernel::generic || wide)) return DecFront::entries;
    if (tuning().slow_index) return DecFront::serial;
    if (t.usable && !unit_parallel) return DecFront::pieces;
    if (t.usable) return k == DecKernel::px || k == DecKernel::px16 || (wide && t.per_segment && g.ulen_sz == 2) ? DecFront::table_lanes : DecFront::serial;
    if (best) return best_rung(DecFront::best_exits, g, plan, walk_memory_ok, wave_ok);
    return walk_memory_ok && (k == DecKernel::px || k == DecKernel::px16 || wide || (k == DecKernel::pxu && g.tsz <= 2)) ? DecFront::table_walk : DecFront::serial;
}

// can a container's table be decoded strip by strip: one launch of a wave-per-segment decoder per range of segments, nothing else
bool decode_strips_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix) {
    const DecKernel k = aligned_dec_kernel(g, plan);
    return k != DecKernel::generic && pick_dec_front(g, plan, k, false, table_shape(g, ix), false, false) == DecFront::entries;
}
// does a plain stream of this raster walk through table memory when the host brings some
bool walk_table_applies(const Geometry &g, const DecPlan &plan) {
    const DecFront f = pick_dec_front(g, plan, aligned_dec_kernel(g, plan), false, TableShape(), !tuning().slow_walk, false);
    // (two bands of 8-bit common-factor data: the exits are the chain's alternative; for a raster the chain does not take no memory is brought)
    if (f == DecFront::best_exits && g.bands == 2) return best_chain_applies(g, plan);
    return f == DecFront::table_walk || f == DecFront::best_exits || f == DecFront::best_chain;
}

// A restart table is untrusted input that the decoder takes positions, rungs and values from: its chunks are checked (ix_check_chunk,
// qb3_kernels.h) -- by this kernel in front of the decoder, or by workgroups of the decoder's own launch (dec_px_kernel, DecArgs::chk_wgs).
// A mismatch raises status bit 5; the host then decodes the call again without the table.  A workgroup per chunk.
__global__ void __launch_bounds__(256) ix_check_kernel(const DecArgs a0) {
    const DecArgs a = dec_for_tile(a0, blockIdx.y);
    __shared__ uint32_t part[4];
    ix_check_chunk(a, blockIdx.x, part);
}

static int launch_decode_all(DecArgs a, const DecPlan &plan, DecKernel k, DecFront front, const TableShape &table, hipStream_t st,
                             void *walk_tab, size_t walk_tab_bytes, bool walk_memory_ok, uint64_t max_bits, const DecStrip *strip) {
    // the table's check: the wave-per-segment decoders that work from the entries alone make it with the first workgroups of their own
    // launch (DecArgs::chk_wgs: one launch, not two); everything else, and the first strip, has ix_check_kernel in front
    if (front != DecFront::none && a.ix && a.ix_K && (a.ix_ver >= 3 || a.ix_check_heads) && (!strip || strip->first)) {
        const uint32_t chunks = (a.ix_K + a.ix_per_chunk - 1) / a.ix_per_chunk;
        if (front == DecFront::entries && k != DecKernel::generic && !strip) a.chk_wgs = chunks;
        else hipLaunchKernelGGL(ix_check_kernel, dim3(chunks, a.ntiles), dim3(256), 0, st, a);
    }
    if (strip && (front != DecFront::entries || k == DecKernel::generic)) { set_error("decode: strips need the container's table", 0); return -1; }
    // a rung that declines at run time passes to the next one: the route says "try", it does not predict the answer
    if (front == DecFront::best_exits && !launch_dec_walk_best(a, st, walk_tab, walk_tab_bytes, max_bits)) front = best_rung(DecFront::best_chain, a.g, plan, walk_memory_ok, dec_index_walk_best_ok(a));
    if (front == DecFront::best_chain && !walk_chain_lds_ok()) front = best_rung(DecFront::best_wave, a.g, plan, walk_memory_ok, dec_index_walk_best_ok(a));
    bool totals = false;        // the decoder itself adds up the values of every segment (totals_only); a scan makes entering values of the sums
    switch (front) {
    case DecFront::none: case DecFront::pieces: case DecFront::best_exits: break;
    case DecFront::entries: a.bl_mode = 1; break;
    case DecFront::table_lanes: { ProfScope ps("dec_index_serial", st); launch_dec_walk(a, st); } totals = !table.per_segment; break;      // (an entry per segment: the walk copied the entering values)
    case DecFront::table_walk: launch_dec_walk_table(a, st, walk_tab, walk_tab_bytes, max_bits); totals = true; break;
    case DecFront::best_chain: {
        // the factors in force start from zero (the lane writes them from the first unit that brings one on); the block table is added up
        const size_t cfb = (size_t)a.g.nseg * a.g.bands * a.g.tsz, ulb = a.g.ulen_sz == 4 ? (size_t)a.g.nblocks * 4 : 0;
        if (a.ntiles > 1) { (void)hipMemset2DAsync(a.idx.cf, a.ts_idx, 0, cfb, a.ntiles, st); if (ulb) (void)hipMemset2DAsync(a.idx.ulen, a.ts_idx, 0, ulb, a.ntiles, st); }
        else { (void)hipMemsetAsync(a.idx.cf, 0, cfb, st); if (ulb) (void)hipMemsetAsync(a.idx.ulen, 0, ulb, st); }
        if (a.g.tsz == 2) walk_chain_16bit(a, st, walk_tab, walk_tab_bytes, max_bits); else walk_chain_8bit_any(a, st, walk_tab, walk_tab_bytes, max_bits);
        totals = true; break;
    }
    case DecFront::best_wave: { ProfScope ps("dec_index_serial", st); launch_dec_index_walk_best(a, st); } totals = true; break;
    case DecFront::serial: { ProfScope ps("dec_index_serial", st); launch_dec_index_serial(a, st); } break;
    }
    // (the totals of common-factor streams: by the lane-per-unit decoder where it decodes, else by the generic one)
    if (totals) { DecArgs t = a; t.totals_only = 1; launch_dec_kernel(a.g.mode != CM_BEST || k == DecKernel::pxu_best ? k : DecKernel::generic, t, plan, st, "dec_index_prev"); }
    if (totals || front == DecFront::best_exits) { ProfScope ps("dec_index_scan", st); launch_prev_scan(a, st); }
    launch_dec_kernel(k, a, plan, st);
    HIPCHK(hipGetLastError());
    return 0;
}

// Staging of a wave-per-segment decoder (dwords, at most `worst`): four worst-case segments a workgroup cost resident workgroups, so it is sized for THIS stream's
// average segment and 1 / margin of it more; a segment that does not fit raises status bit 4 and the caller runs the call again with full_staging
static uint32_t staging_cap_dw(uint32_t worst, uint64_t bits, uint64_t nseg, uint32_t margin) {
    uint64_t cap = bits / 32 / nseg;
    cap = (cap + cap / margin + 64 + 3) & ~(uint64_t)3;
    return bits && cap < worst ? (uint32_t)cap : worst;
}

int launch_decode(const Geometry &g, const DecPlan &plan_in, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                  void *img, const void *index, void *ws, uint32_t **status_out, void *stream, const TileBatch &tb,
                  const uint64_t *tile_bits, const IxTable &ix, void *walk_tab, size_t walk_tab_bytes, bool full_staging, uint32_t wide_band, const DecStrip *strip) {
    hipStream_t st = (hipStream_t)stream;
    DecArgs a = {};
    a.g = g;
    a.ntiles = tb.n ? tb.n : 1;
    const uint64_t bits = tb.n ? tb.max_bits : in_bits;     // the (longest) stream
    const TableShape table = table_shape(g, ix);
    const bool walk_memory_ok = walk_tab && walk_tab_bytes >= walk_table_min_bytes(a.ntiles, g.tsz) && !tuning().slow_walk;
    const TileGridRule tg = make_tile_grid(tb);      // (a decoder's "dst" is the image)
    const DecKernel picked = pick_dec_kernel(g, plan_in, img, tile_pitch_bits(tg, true));
    const DecFront front = pick_dec_front(g, plan_in, picked, index != nullptr, table, walk_memory_ok, dec_index_walk_best_ok(a));
    const DecKernel k = front == DecFront::pieces ? DecKernel::generic : picked;
    // the staging of the kernels that have one: a third above the average for 16-bit data (worst case 278 bits a unit), half for
    // 32/64-bit data (worst case: 4.3 / 8.4 KB a wave) and the lane-per-unit kernels
    DecPlan plan = plan_in;
    const bool wide_staging = plan.pxw || plan.pxw_best, unit_staging = plan.pxu || plan.pxu_best;
    if ((plan.px16 || wide_staging || unit_staging) && !full_staging && g.nseg) {
        plan.px_cap_dw = staging_cap_dw(plan.px_cap_dw, bits, g.nseg, plan.px16 ? 3 : 2);
        if (plan.px16) plan.lds_px = px16_lds_bytes(plan.px_cap_dw);
        if (wide_staging) plan.lds_pxw = pxw_lds_bytes(plan.px_cap_dw, plan.pxw);
    }
    a.in_cap_full = plan_in.px_cap_dw;
    if (table.usable) {      // (else no table: the fields stay zero)
        a.ix = ix.base; a.ix_K = ix.K; a.ix_blocks = ix.blocks; a.ix_E = ix.entry_bytes; a.ix_per_chunk = ix.per_chunk; a.ix_pad = ix.pads ? IX_PAD : 0;
        a.ix_bl = ix.block_lens; a.ix_ver = ix.version; a.ix_check_heads = ix.check_heads ? 1u : 0u;
    }
    // lane-per-segment decoder: LDS for the stream words of a workgroup's segments, half as much again as the average, when that is
    // at most 24 KB (more would cost more in resident workgroups than the staging saves; a longer span is read from global memory).
    // From the table's pieces no index is rebuilt at all.  (from_ix is also set where a common-factor stream is decoded from the
    // entries' block fields: those kernels do not read it)
    a.from_ix = front == DecFront::pieces || (front == DecFront::entries && g.mode == CM_BEST) ? 1u : 0u;
    if (g.nseg && !(plan.fast && g.mode != CM_BEST)) {
        uint64_t cap = bits / 32 * plan.threads / (a.from_ix ? a.ix_K : g.nseg);
        cap = (cap + cap / 2 + 64 + 3) & ~(uint64_t)3;
        if (bits && cap <= 24 * 1024 / 4) a.seg_cap_dw = (uint32_t)cap;
    }
    a.in32 = in32; a.in_bit0 = in_bit0; a.in_bits = in_bits; a.img = img; a.ts_in = tg.src; a.ts_img = tg.dst; a.tile_bits = tile_bits;
    a.tcols = tg.cols; a.tmagic = tg.magic; a.tr_in = tg.src_row; a.tr_img = tg.dst_row;
    uint8_t *w = (uint8_t *)ws;
    const bool rebuild = index == nullptr;
    // workspace: [status words, 64 bytes per 16 tiles][rebuilt indices, one per tile]
    const size_t status_bytes = ((4 * (size_t)a.ntiles + 63) / 64) * 64;
    *status_out = a.status = (uint32_t *)w;
    a.idx = index_view(g, rebuild ? (void *)(w + status_bytes) : const_cast<void *>(index));
    a.ts_idx = rebuild ? align8(index_bytes(g)) : tg.idx;
    a.tr_idx = rebuild ? a.tcols * a.ts_idx : tg.idx_row;         // (the rebuilt indices stand in the workspace, one a launch tile)
    // a strip is one launch of a wave-per-segment decoder; where one applies but the memory is not aligned for it the generic kernel was
    // picked, which does not decode ranges of segments: refused before anything is enqueued.  (The host's strips go to pool memory.)
    if (strip && picked == DecKernel::generic && aligned_dec_kernel(g, plan_in) != DecKernel::generic) {
        set_error("decode: strips need value-aligned memory", 0);
        return -1;
    }
    if (!strip || strip->first) HIPCHK(hipMemsetAsync(a.status, 0, status_bytes, st));
    a.seg0 = strip ? strip->seg0 : 0;
    a.seg_end = strip ? std::min<uint64_t>(g.nseg, strip->seg0 + strip->nseg) : g.nseg;
    a.lane_dw = dec_lane_dwords(g); a.dpr = g.bands * g.tsz;
    a.bpp = plan.bpp; a.passes = plan.passes; a.in_cap_dw = (plan.px || plan.px16 || plan.px_best || plan.pxw || plan.pxw_best || plan.pxu || plan.pxu_best) ? plan.px_cap_dw : plan.in_cap_dw;
    a.px_ng = plan.px16 ? plan.px16_ng : 1; a.px_magic_ng = magic_div(a.px_ng);
    a.wide_band = tuning().wide_band ? (uint32_t)tuning().wide_band : wide_band;
    a.px_aligned = !(g.w & 3) && !((g.stride * g.tsz) & 3) && !((uintptr_t)img & 3) && !(tile_pitch_bits(tg, true) & 3);
    a.magic_bpp = magic_div(plan.bpp); a.magic_dpr = magic_div(a.dpr); a.magic_bands = magic_div(g.bands);
    if (g.tsz != 1 && g.tsz != 2 && g.tsz != 4 && g.tsz != 8) { set_error("decode: bad value size", 0); return -1; }
    return launch_decode_all(a, plan, k, front, table, st, walk_tab, walk_tab_bytes, walk_memory_ok, bits, strip);
}

}  // namespace qb3dev
