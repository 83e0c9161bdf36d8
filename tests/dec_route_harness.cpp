// tests/dec_route_harness.cpp -- which launches a decode makes, and which an encode, found out on the CPU.
//
// The host half of the decoder (plan_decode, launch_decode and the predicates next to them) decides which kernel decodes the units
// and what runs in front of it.  It links without a device once the launchers of the kernel translation units and the dozen HIP
// entry points it calls exist, so this program defines all of them as RECORDERS, calls launch_decode over a grid of rasters,
// tables, alignments and walk memory, and prints what was recorded: one block of lines per case.  tests/test_decode_routes.py
// builds it against the objects make produced, runs it once per debugging switch (tuning() is read once per process) and compares
// the output with tests/golden/dec_routes.txt and dec_routes.fnv.
//
//   dec_route_harness LABEL     prints "fnv ..." lines (one FNV-1a64 of the complete output per value size and mode) and, for the
//                               first case of every distinct launch sequence, the case itself
//
// The complete output is: a "geometry" line per raster (what plan_decode says of it), a "table" line per raster and table (what the
// predicates say), and every case: its "case" line, a line per recorded call, the return value.  A printed case repeats the
// geometry and table lines under its "case" line.
//
// The grid is the cross product of the dimensions below, less the combinations that cannot differ (said where they are dropped).
//
//   dec_route_harness enc LABEL   the same for the encoder: plan_encode, then launch_encode, or launch_encode_strip (first, middle, last
//                               strip) and launch_encode_tail, over a grid of rasters, pointers, tile batches, indexes and tables.  The
//                               encoder's launchers (which a decode must never reach) record in this mode: a "geometry" line per raster,
//                               and every case -- its "case" line, a line per launcher with the plan it was handed and the arguments that
//                               follow from the plan's kernel (workspace pointers as offsets), the "enc_units" scope, the return value.
//                               tests/test_encode_routes.py compares with tests/golden/enc_routes.txt and enc_routes.fnv.  Behind the
//                               grid, "refusal" lines: plans made for value-aligned memory, launched with memory that is not.
//   dec_route_harness plan ...    how plan_encode cuts common-factor rasters into chunks (print_plans, below)
#include "qb3_kernels.h"
#include "qb3_walk.h"
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace qb3dev;

// ------------------------------------------------------------------ the record of one case
namespace {
struct Rec { char line[1024], sig[48]; uint64_t ev; };          // ev != 0: an event record, named after the case
struct Recs {                                                   // (fixed storage: a run makes close to a million of these lists)
    Rec r[48]; int n = 0;
    void clear() { n = 0; }
    void add(const char *line, const char *sig, uint64_t ev) {
        if (n == 48) { fprintf(stderr, "more launches in a case than the record holds\n"); abort(); }
        if (strlen(line) >= sizeof(r[n].line) || strlen(sig) >= sizeof(r[n].sig)) abort();
        strcpy(r[n].line, line); strcpy(r[n].sig, sig); r[n++].ev = ev;
    }
} g_rec;
bool g_ret_exits = true, g_ret_wave_ok = true, g_ret_chain_lds = true;      // what the bool launchers answer in this case
int g_resolve = 0;                          // event pairs hipEventElapsedTime may still resolve in this prof_collect
uint64_t g_resolved_a = 0, g_resolved_b = 0;
std::map<const void *, std::string> &kernels() { static std::map<const void *, std::string> m; return m; }

// (a line is put together by hand: the grid has close to a million cases per run, and printf would take most of the time)
struct Line {
    char b[1280]; int n = 0;
    Line &s(const char *t) { while (*t) b[n++] = *t++; return *this; }
    Line &u(uint64_t v) { char d[24]; int k = 0; do d[k++] = (char)('0' + v % 10); while (v /= 10); while (k) b[n++] = d[--k]; return *this; }
    Line &f(const char *name, uint64_t v) { return s(name).u(v); }
    const char *str() { b[n] = 0; return b; }
};
void rec_args(const char *name, const DecArgs &a, const DecPlan *plan, size_t tab_bytes = 0, uint64_t max_bits = 0, bool walk = false) {
    Line l;
    l.s("  ").s(name).f(" bl_mode=", a.bl_mode).f(" totals_only=", a.totals_only).f(" chk_wgs=", a.chk_wgs).f(" from_ix=", a.from_ix).f(" in_cap_dw=", a.in_cap_dw)
     .f(" in_cap_full=", a.in_cap_full).f(" seg_cap_dw=", a.seg_cap_dw).f(" seg=[", a.seg0).f(",", a.seg_end).f(") wide_band=", a.wide_band).f(" px_aligned=", a.px_aligned)
     .f(" ix_K=", a.ix ? a.ix_K : 0).f(" ix_blocks=", a.ix_blocks).f(" ix_bl=", a.ix_bl).f(" ix_ver=", a.ix_ver).f(" ix_check_heads=", a.ix_check_heads);
    if (walk) l.f(" tab_bytes=", tab_bytes).f(" max_bits=", max_bits);
    if (plan) l.f(" | px_cap_dw=", plan->px_cap_dw).f(" lds_px=", plan->lds_px).f(" lds_pxw=", plan->lds_pxw);
    Line g;
    g.s(name).f(":", a.bl_mode != 0).u(a.totals_only != 0).u(a.from_ix != 0).u(a.chk_wgs != 0);
    g_rec.add(l.str(), g.str(), 0);
}
void rec_walk(const char *name, const DecArgs &a, size_t tab_bytes, uint64_t max_bits) { rec_args(name, a, nullptr, tab_bytes, max_bits, true); }
[[noreturn]] void never(const char *name) { fprintf(stderr, "%s: the decoder's launch code must not call this\n", name); abort(); }

// the encoder's launchers record in `enc` mode alone
bool g_enc = false;
uint8_t *const ENC_WS = (uint8_t *)0x20000000;
// what a plan says besides its kernel, which the launcher's name (and front) states
void enc_plan_fields(Line &l, const EncPlan &p) {
    l.f(" | plan threads=", p.threads).f(" slots=", p.slots).f(" nbp=", p.nbp).f(" nchunks=", p.nchunks).f(" lds_bytes=", p.lds_bytes).f(" ws_bytes=", p.ws_bytes)
     .f(" rgb=", p.rgb).f(" bg=", p.px16_bg).f(" ng=", p.px16_ng);
}
// front: of launch_enc_best, 0 unit per lane, 1 lane per block along the Hilbert curve, 2 along the Z curve
void rec_enc(const char *name, const EncArgs &a, const EncPlan &p, int front = -1, int strip = -1) {
    if (!g_enc) never(name);
    Line l;
    l.s("  ").s(name);
    if (front >= 0) l.f(" front=", front);
    if (strip >= 0) l.f(" strip=", strip);
    enc_plan_fields(l, p);
    l.f(" | px_ng=", a.px_ng).f(" px16_bg=", a.px16_bg).f(" px_aligned=", a.px_aligned).f(" ix_coder=", a.ix_coder).f(" ix_bl=", a.ix_bl).f(" have_idx=", a.have_idx)
     .f(" idx_no_ulen=", a.idx_no_ulen).f(" chunk0=", a.chunk0).f(" chunk_end=", a.chunk_end).f(" finish_what=", a.finish_what).f(" hdr_back=", a.hdr_back)
     .f(" slot_dw=", a.slot_dw).f(" ntiles=", a.ntiles).f(" tcols=", a.tcols).f(" zrun_probe=", a.zrun_probe);
    auto off = [](const void *q) { return (uint64_t)((const uint8_t *)q - ENC_WS); };
    l.f(" | ws chunk_bits=", off(a.chunk_bits)).f(" chunk_off=", off(a.chunk_off)).f(" group_sum=", off(a.group_sum)).f(" seams=", off(a.seams)).f(" scratch=", off(a.scratch))
     .f(" cw_has=", off(a.cw_has)).f(" cw_val=", off(a.cw_val)).f(" centry=", off(a.centry)).f(" centry_parts=", off(a.centry_parts)).f(" recode_n=", off(a.recode_n))
     .f(" cw_used=", off(a.cw_used)).f(" seg_from_entry=", off(a.seg_from_entry)).f(" recode_need=", off(a.recode_need)).f(" recode_list=", off(a.recode_list)).f(" res=", off(a.res));
    Line g;
    g.s(name).f(":", front < 0 ? 9 : front).f(",", a.finish_what).u(a.ix_coder != 0).u(a.have_idx != 0).u(a.idx_no_ulen != 0);
    g_rec.add(l.str(), g.str(), 0);
}
}  // namespace

// ------------------------------------------------------------------ the launchers of the kernel translation units
namespace qb3dev {
void launch_dec_generic(const DecArgs &a, const DecPlan &p, hipStream_t) { rec_args("launch_dec_generic", a, &p); }
void launch_dec_px(const DecArgs &a, const DecPlan &p, hipStream_t) { rec_args("launch_dec_px", a, &p); }
void launch_dec_px16(const DecArgs &a, const DecPlan &p, hipStream_t) { rec_args("launch_dec_px16", a, &p); }
void launch_dec_pxw(const DecArgs &a, const DecPlan &p, hipStream_t) { rec_args("launch_dec_pxw", a, &p); }
void launch_dec_pxw_best(const DecArgs &a, const DecPlan &p, hipStream_t) { rec_args("launch_dec_pxw_best", a, &p); }
void launch_dec_px_best(const DecArgs &a, const DecPlan &p, hipStream_t) { rec_args("launch_dec_px_best", a, &p); }
void launch_dec_pxu(const DecArgs &a, const DecPlan &p, hipStream_t) { rec_args("launch_dec_pxu", a, &p); }
void launch_dec_pxu_best(const DecArgs &a, const DecPlan &p, hipStream_t) { rec_args("launch_dec_pxu_best", a, &p); }
void launch_dec_index_serial(const DecArgs &a, hipStream_t) { rec_args("launch_dec_index_serial", a, nullptr); }
void launch_dec_index_walk_best(const DecArgs &a, hipStream_t) { rec_args("launch_dec_index_walk_best", a, nullptr); }
bool dec_index_walk_best_ok(const DecArgs &) { return g_ret_wave_ok; }
void launch_dec_walk(const DecArgs &a, hipStream_t) { rec_args("launch_dec_walk", a, nullptr); }
void launch_prev_scan(const DecArgs &a, hipStream_t) { rec_args("launch_prev_scan", a, nullptr); }
bool launch_dec_walk_best(const DecArgs &a, hipStream_t, void *, size_t n, uint64_t bits) {
    rec_walk(g_ret_exits ? "launch_dec_walk_best=true" : "launch_dec_walk_best=false", a, n, bits);
    return g_ret_exits;
}
void launch_dec_walk_table(const DecArgs &a, hipStream_t, void *, size_t n, uint64_t bits) { rec_walk("launch_dec_walk_table", a, n, bits); }
bool walk_chain_lds_ok() { return g_ret_chain_lds; }
bool walk_exit_lds_ok() { return true; }
void walk_chain_16bit(const DecArgs &a, hipStream_t, void *, size_t n, uint64_t bits) { rec_walk("walk_chain_16bit", a, n, bits); }
void walk_chain_8bit_any(const DecArgs &a, hipStream_t, void *, size_t n, uint64_t bits) { rec_walk("walk_chain_8bit_any", a, n, bits); }
void walk_chain_8bit(const DecArgs &, hipStream_t, void *, size_t, uint64_t) { never("walk_chain_8bit"); }
void walk_chain_wide(const DecArgs &, hipStream_t, void *, size_t, uint64_t) { never("walk_chain_wide"); }
// (a stand-in of the same shape as k_dec_walk.hip's: a state per tile, two windows per tile, a page)
size_t walk_table_min_bytes(uint32_t ntiles, uint32_t tsz) { return (((size_t)ntiles * 128 + 255) & ~(size_t)255) + (size_t)ntiles * 2 * (tsz >= 4 ? 30720 : 46080) + 4096; }
// the encoder's launchers: k_host.o names them, a decode never reaches them; the `enc` mode records them
void launch_enc_generic(const EncArgs &a, const EncPlan &p, hipStream_t) { rec_enc("launch_enc_generic", a, p); }
void launch_enc_best(const EncArgs &a, const EncPlan &p, hipStream_t, bool front) { rec_enc("launch_enc_best", a, p, !front ? 0 : a.g.order == ZCURVE ? 2 : 1); }
void launch_enc_px(const EncArgs &a, const EncPlan &p, hipStream_t) { rec_enc("launch_enc_px", a, p); }
void launch_enc_px_best(const EncArgs &a, const EncPlan &p, hipStream_t) { rec_enc("launch_enc_px_best", a, p); }
void launch_enc_px16(const EncArgs &a, const EncPlan &p, hipStream_t) { rec_enc("launch_enc_px16", a, p); }
void launch_enc_pxw(const EncArgs &a, const EncPlan &p, hipStream_t) { rec_enc("launch_enc_pxw", a, p); }
void launch_enc_post(const EncArgs &a, const EncPlan &p, hipStream_t) { rec_enc("launch_enc_post", a, p); }
void launch_enc_post_strip(const EncArgs &a, const EncPlan &p, hipStream_t, uint32_t strip) { rec_enc("launch_enc_post_strip", a, p, -1, (int)strip); }
void launch_enc_post_tail(const EncArgs &a, const EncPlan &p, hipStream_t) { rec_enc("launch_enc_post_tail", a, p); }
}  // namespace qb3dev

// ------------------------------------------------------------------ the HIP entry points the host half calls
extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, uint3 *, uint3 *, dim3 *, dim3 *, int *) { kernels()[host_fn] = device_name; }
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
}
static dim3 g_cfg_grid, g_cfg_block; static size_t g_cfg_lds; static hipStream_t g_cfg_st;
extern "C" hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t st) { g_cfg_grid = grid; g_cfg_block = block; g_cfg_lds = lds; g_cfg_st = st; return hipSuccess; }
extern "C" hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *lds, hipStream_t *st) { *grid = g_cfg_grid; *block = g_cfg_block; *lds = g_cfg_lds; *st = g_cfg_st; return hipSuccess; }
hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3, void **, size_t, hipStream_t) {
    const std::string &name = kernels()[fn];
    if (name.find("ix_check_kernel") == std::string::npos) { fprintf(stderr, "unexpected kernel launch: %s\n", name.c_str()); abort(); }
    char buf[96];
    snprintf(buf, sizeof(buf), "  ix_check_kernel grid=(%u,%u)", grid.x, grid.y);
    g_rec.add(buf, "ix_check_kernel", 0);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *, int, size_t n, hipStream_t) {
    char buf[64];
    snprintf(buf, sizeof(buf), "  hipMemsetAsync bytes=%zu", n);
    g_rec.add(buf, "memset", 0);
    return hipSuccess;
}
hipError_t hipMemset2DAsync(void *, size_t, int, size_t w, size_t h, hipStream_t) {
    char buf[64];
    snprintf(buf, sizeof(buf), "  hipMemset2DAsync bytes=%zux%zu", w, h);
    g_rec.add(buf, "memset2d", 0);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "hip error"; }
hipError_t hipEventCreate(hipEvent_t *e) { static uintptr_t n = 0; *e = (hipEvent_t)(++n); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { g_rec.add("", "", (uint64_t)(uintptr_t)e); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
    if (g_resolve <= 0) return hipErrorNotReady;
    g_resolve--; g_resolved_a = (uint64_t)(uintptr_t)a; g_resolved_b = (uint64_t)(uintptr_t)b; *ms = 1.0f;
    return hipSuccess;
}

// ------------------------------------------------------------------ the grid
namespace {
const char *const MODE_NAME[] = {"FTL", "BASE", "CF"};
constexpr uint64_t FOREIGN = 0x0123456789abcdefull;       // a curve that is neither Hilbert nor Z
struct Raster { uint32_t w, h; };
const Raster RASTERS[] = {{64, 64}, {1000, 37}, {3, 400}};
// order x band map: the launch code asks of the order only "Hilbert or Z, or another" and of the map only "identity, the default, core bands
// that are core, or not" -- independently of each other, so each map is crossed with one order and each order with the identity
// (and, to pin that independence, the default map once with the foreign curve)
struct Curve { const char *name; uint64_t order; int map; };
const Curve CURVES[] = {{"hilbert/identity", HILBERT, 0}, {"z/identity", ZCURVE, 0}, {"foreign/identity", FOREIGN, 0}, {"hilbert/rgb", HILBERT, 1}, {"z/noncore", ZCURVE, 2}, {"foreign/rgb", FOREIGN, 1}};
const char *const TABLE_NAME[] = {"none", "several", "per_seg", "block_fields", "wrong_K", "version2", "check_heads"};
const char *const ALIGN_NAME[] = {"aligned", "pointer+1", "odd_pitch"};
const char *const WALK_NAME[] = {"none", "min", "ample"};
const char *const STRIP_NAME[] = {"none", "first", "later"};

Geometry make_geometry(uint32_t w, uint32_t h, uint32_t bands, uint32_t tsz, uint32_t mode, uint64_t order, int map) {     // as qb3_api.cpp's
    Geometry g;
    memset(&g, 0, sizeof(g));
    g.w = w; g.h = h; g.bands = bands; g.tsz = tsz; g.stride = (uint64_t)w * bands; g.order = order;
    g.nbx = (w + 3) / 4; g.nby = (h + 3) / 4; g.nblocks = (uint64_t)g.nbx * g.nby;
    g.mode = mode;
    g.ulen_sz = ulen_size_for(tsz, mode, bands);
    for (uint32_t c = 0; c < bands; c++) g.cband[c] = (uint8_t)c;
    if (map == 1 && bands >= 3) g.cband[0] = g.cband[2] = 1;
    if (map == 2 && bands >= 2) { g.cband[0] = 1; g.cband[1] = bands >= 3 ? 2 : 0; }      // band 0's core band is not itself core
    g.seg_blocks = seg_blocks_for(g);
    g.nseg = (g.nblocks + g.seg_blocks - 1) / g.seg_blocks;
    return g;
}

IxTable make_table(const Geometry &g, int kind) {
    IxTable t;
    if (!kind) return t;
    t.base = (uint8_t *)0x40000000;
    t.block_lens = kind >= 3;
    t.blocks = kind == 1 ? 2 * g.seg_blocks : g.seg_blocks;
    t.entry_bytes = ix_entry_bytes(g, t.block_lens);
    t.K = (uint32_t)((g.nblocks + t.blocks - 1) / t.blocks) + (kind == 4 ? 1 : 0);
    t.per_chunk = (65535 - IX_HEAD) / t.entry_bytes;
    t.version = kind >= 5 ? 2 : 3;
    t.check_heads = kind == 6;
    return t;
}

struct Case {
    uint32_t tsz, bands, mode; int raster, curve, index, table, align, walk; uint32_t tiles; uint64_t bits; uint32_t wide_band; int full, strip;
    bool exits, wave_ok, chain_lds;
};

struct Out {
    std::string text, sig;        // of the case being written
    uint64_t fnv = 0xcbf29ce484222325ull, cases = 0;
    std::set<std::string> seen;
    void hash() { for (unsigned char c : text) { fnv ^= c; fnv *= 0x100000001b3ull; } }
};

// what every case of a raster, and of a raster with a table, shares: said once in the hashed output, and again under every case that is printed
struct Context { Geometry g; DecPlan plan; IxTable ix; std::string geometry_line, table_line; };

void set_geometry(Context &x, const Case &c, Out &out) {
    const Raster &r = RASTERS[c.raster];
    x.g = make_geometry(r.w, r.h, c.bands, c.tsz, c.mode, CURVES[c.curve].order, CURVES[c.curve].map);
    x.plan = plan_decode(x.g);
    const Geometry &g = x.g; const DecPlan &plan = x.plan;
    Line l;
    l.f("  geometry seg_blocks=", g.seg_blocks).f(" nseg=", g.nseg).f(" ulen_sz=", g.ulen_sz).f(" | plan threads=", plan.threads).f(" nwg=", plan.nwg).f(" lds_bytes=", plan.lds_bytes)
     .f(" ws_bytes=", plan.ws_bytes).f(" fast=", plan.fast).f(" threads2=", plan.threads2).f(" bpp=", plan.bpp).f(" passes=", plan.passes).f(" in_cap_dw=", plan.in_cap_dw)
     .f(" lds2_bytes=", plan.lds2_bytes).f(" px=", plan.px).f(" px_rgb=", plan.px_rgb).f(" lds_px=", plan.lds_px).f(" px_cap_dw=", plan.px_cap_dw).f(" px16=", plan.px16)
     .f("/", plan.px16_bg).f("/", plan.px16_ng).f(" px_best=", plan.px_best).f(" pxw=", plan.pxw).f(" pxw_best=", plan.pxw_best).f(" lds_pxw=", plan.lds_pxw)
     .f(" pxu=", plan.pxu).f(" pxu_best=", plan.pxu_best).f(" | walk_table_applies=", walk_table_applies(g, plan)).s("\n");
    x.geometry_line = l.str();
    out.text = x.geometry_line;
    out.hash();
}
void set_table(Context &x, const Case &c, Out &out) {
    x.ix = make_table(x.g, c.table);
    Line l;
    l.f("  table K=", x.ix.K).f(" blocks=", x.ix.blocks).f(" entry_bytes=", x.ix.entry_bytes).f(" per_chunk=", x.ix.per_chunk).f(" | decode_strips_ok=", decode_strips_ok(x.g, x.plan, x.ix))
     .f(" decode_window_ok=", decode_window_ok(x.g, x.plan, x.ix)).s("\n");
    x.table_line = l.str();
    out.text = x.table_line;
    out.hash();
}

// what the launch under test left in g_rec, behind the case line in out.text: the scopes named, the records written out, the return value; the case
// hashed and, when its launch sequence is new, printed with the two context lines under its case line
void finish_case(Out &out, int rc, size_t head, const std::string &context, const std::string &context2) {
    char buf[320];
    std::string &t = out.text;
    // the scopes' names: prof_collect resolves the pending event pairs in the order the scopes closed; let it resolve one at a time
    for (;;) {
        g_resolve = 1; g_resolved_a = 0;
        prof_collect();
        if (!g_resolved_a) break;
        char names[64] = "  { ";
        prof_names(names + 4, sizeof(names) - 4);
        prof_reset();
        for (int i = 0; i < g_rec.n; i++) {
            if (g_rec.r[i].ev == g_resolved_a) { snprintf(g_rec.r[i].line, sizeof(g_rec.r[i].line), "%s", names); g_rec.r[i].ev = 0; snprintf(g_rec.r[i].sig, sizeof(g_rec.r[i].sig), "%s", names + 2); }
            else if (g_rec.r[i].ev == g_resolved_b) { snprintf(g_rec.r[i].line, sizeof(g_rec.r[i].line), "  }"); g_rec.r[i].ev = 0; snprintf(g_rec.r[i].sig, sizeof(g_rec.r[i].sig), "}"); }
        }
    }
    std::string &sig = out.sig;
    sig.clear();
    for (int i = 0; i < g_rec.n; i++) {
        const Rec &x = g_rec.r[i];
        if (x.ev) { fprintf(stderr, "an event record that belongs to no scope\n"); abort(); }
        t += x.line; t += '\n';
        sig += x.sig; sig += ';';
    }
    if (rc) snprintf(buf, sizeof(buf), "  -> %d (%s)\n", rc, last_error()); else snprintf(buf, sizeof(buf), "  -> 0\n");
    t += buf;
    sig += rc ? last_error() : "0";
    out.hash();
    out.cases++;
    if (out.seen.insert(sig).second) { t.insert(head, context + context2); fputs(t.c_str(), stdout); fputc('\n', stdout); }
}

void run_case(const Context &x, const Case &c, Out &out) {
    const Raster &r = RASTERS[c.raster];
    const Geometry &g = x.g; const DecPlan &plan = x.plan; const IxTable &ix = x.ix;
    g_ret_exits = c.exits; g_ret_wave_ok = c.wave_ok; g_ret_chain_lds = c.chain_lds;
    std::string &t = out.text;
    t.clear();
    Line l;
    l.f("case tsz=", c.tsz).f(" bands=", c.bands).s(" mode=").s(MODE_NAME[c.mode]).f(" raster=", r.w).f("x", r.h).s(" curve=").s(CURVES[c.curve].name).f(" index=", c.index)
     .s(" table=").s(TABLE_NAME[c.table]).s(" align=").s(ALIGN_NAME[c.align]).s(" walk=").s(WALK_NAME[c.walk]).f(" tiles=", c.tiles).f(" bits=", c.bits)
     .f(" wide_band=", c.wide_band).f(" full_staging=", c.full).s(" strip=").s(STRIP_NAME[c.strip]).f(" answers=", c.exits).u(c.wave_ok).u(c.chain_lds).s("\n");
    t += l.str();
    const size_t head = t.size();

    const size_t img_bytes = ((size_t)r.w * r.h * c.bands * c.tsz + 255) & ~(size_t)255;
    TileBatch tb;
    if (c.tiles > 1) { tb.n = c.tiles; tb.src_pitch = 1 << 20; tb.dst_pitch = img_bytes + (c.align == 2 ? 1 : 0); tb.idx_pitch = index_bytes(g); tb.max_bits = c.bits; }
    void *img = (void *)(uintptr_t)(0x10000000 + (c.align == 1 ? 1 : 0));
    void *walk_tab = c.walk ? (void *)0x50000000 : nullptr;
    const size_t walk_bytes = c.walk == 1 ? walk_table_min_bytes(c.tiles, c.tsz) : c.walk == 2 ? (size_t)1 << 30 : 0;
    const uint64_t third = g.nseg / 3;
    const DecStrip strip = c.strip == 1 ? DecStrip{0, third + 1, true} : DecStrip{third, third + 1, false};
    uint32_t *status = nullptr;
    g_rec.clear();
    const int rc = launch_decode(g, plan, (const uint32_t *)0x30000000, 8, c.tiles > 1 ? 0 : c.bits, img, c.index ? (const void *)0x60000000 : nullptr, (void *)0x20000000, &status,
                                 nullptr, tb, c.tiles > 1 ? (const uint64_t *)0x70000000 : nullptr, ix, walk_tab, walk_bytes, c.full != 0, c.wide_band, c.strip ? &strip : nullptr);
    finish_case(out, rc, head, x.geometry_line, x.table_line);
}

void run_group(uint32_t tsz, uint32_t mode, Out &out) {
    static const uint32_t BANDS[] = {1, 2, 3, 4, 5, 7, 8};
    static const uint32_t TILES[] = {1, 5, 17};
    static const uint64_t BITS[] = {100000, 5000000};
    static const uint32_t WIDE[] = {16, 17, 18};
    Case c;
    Context x;
    c.tsz = tsz; c.mode = mode;
    for (uint32_t bands : BANDS) for (c.raster = 0; c.raster < 3; c.raster++) for (c.curve = 0; c.curve < 6; c.curve++) {
        c.bands = bands;
        if (CURVES[c.curve].map == 1 && bands < 3) continue;      // (the default map needs three bands, a core band that is not core two)
        if (CURVES[c.curve].map == 2 && bands < 2) continue;
        set_geometry(x, c, out);
        for (c.index = 0; c.index < 2; c.index++) for (c.table = 0; c.table < 7; c.table++) for (c.strip = 0; c.strip < 3; c.strip++) {
            if (c.strip && (!c.table || c.index)) continue;       // strips need a table, and come without an index
            // with an index handed in nothing runs in front of the decoder: of the tables, "none" and the one whose fields reach the arguments
            if (c.index && c.table != 0 && c.table != 3) continue;
            set_table(x, c, out);
            // a stream with no usable table is a plain one: only there walk memory, the band of rungs and the walks' answers are looked at
            const bool plain = !c.index && !c.strip && (c.table == 0 || c.table == 4);
            for (c.walk = 0; c.walk < (plain ? 3 : 1); c.walk++) for (uint32_t tiles : TILES) for (c.align = 0; c.align < 3; c.align++) {
                c.tiles = tiles;
                if (c.align == 2 && tiles == 1) continue;         // one image has no pitch
                if (tiles == 17 && (c.align == 1 || c.strip || c.index)) continue;    // (17 tiles against 5: more status words, more walk memory -- nothing an alignment or a strip meets)
                for (uint64_t bits : BITS) for (c.full = 0; c.full < 2; c.full++) for (uint32_t wb : WIDE) {
                    c.bits = bits; c.wide_band = wb;
                    if (wb != 16 && !(plain && tsz >= 4 && c.walk)) continue;
                    // full staging only switches off the sizing by the stream's length: with it on, one length says as much as two (what else
                    // a length moves, the lane-per-segment staging, is met with it off)
                    if (c.full && bits != BITS[1]) continue;         // the band of rungs is for plain 32/64-bit streams that walk
                    // what the bool launchers answer: every combination where a plain common-factor stream can ask them, once for one image
                    const bool ask = plain && mode == CM_BEST && tiles == 1 && c.align == 0 && !c.full;
                    for (int ans = 0; ans < (ask ? 8 : 1); ans++) {
                        c.exits = !(ans & 1); c.wave_ok = !(ans & 2); c.chain_lds = !(ans & 4);
                        run_case(x, c, out);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------ the encoder's grid (`enc` mode)
const Raster ENC_RASTERS[] = {{3, 8}, {4, 4}, {67, 41}, {16384, 4096}};   // no lane-per-block kernel; one block; partial last blocks and unaligned rows; strips (encode_strips_ok)
const uint32_t ENC_PTR[] = {0, 1, 2, 4};                // bytes the image pointer is off 16
const char *const ENC_TILES_NAME[] = {"one", "row5", "row5_odd_pitch", "grid2x3"};
const char *const ENC_TABLE_NAME[] = {"none", "level1", "level2", "level2_own_index"};
const char *const ENC_LAUNCHER_NAME[] = {"encode", "strip_first", "strip_middle", "strip_last", "tail"};
struct EncCase { uint32_t tsz, bands, mode; int raster, curve, ptr, tiles, index, table, launcher, zrun; };

// one launcher of the three, with the job named field by field
int enc_launch(const Geometry &g, const EncPlan &plan, const EncJob &job, int launcher) {
    const uint32_t nstrips = encode_strip_count(plan);
    switch (launcher) {
    case 0: return launch_encode(g, plan, job, nullptr);
    case 1: return launch_encode_strip(g, plan, job, nullptr, 0);
    case 2: return launch_encode_strip(g, plan, job, nullptr, nstrips / 2);
    case 3: return launch_encode_strip(g, plan, job, nullptr, nstrips - 1);
    default: return launch_encode_tail(g, plan, job, nullptr);
    }
}

// the memory of a case: the pointer, the tile batch as api_tiles.cpp lays one out, and whether all of it is value-aligned as the two callers
// of plan_encode ask (qb3_api.cpp: the pointer; api_tiles.cpp: the pointer and both pitches)
bool enc_memory(const Geometry &g, const EncCase &c, EncJob &job) {
    const size_t img_bytes = ((size_t)g.w * g.h * g.bands * g.tsz + 255) & ~(size_t)255;
    job.img = (const void *)(uintptr_t)(0x10000000 + ENC_PTR[c.ptr]);
    TileBatch &tb = job.tb;
    if (c.tiles) {
        tb.n = c.tiles == 3 ? 6 : 5; tb.src_pitch = img_bytes + (c.tiles == 2 ? 1 : 0); tb.dst_pitch = 1 << 20; tb.idx_pitch = (index_bytes(g) + 7) & ~(size_t)7;
        if (c.tiles == 3) { tb.cols = 2; tb.src_row = 4 * img_bytes; tb.dst_row = 2 * tb.dst_pitch; tb.idx_row = 2 * tb.idx_pitch; }
    }
    return value_aligned_memory(g.tsz, (uintptr_t)job.img | tb.src_pitch | tb.src_row);
}

void run_enc_case(const Geometry &g, const std::string &geometry_line, const EncCase &c, Out &out) {
    const Raster &r = ENC_RASTERS[c.raster];
    EncJob job;
    const bool aligned = enc_memory(g, c, job);
    const EncPlan plan = plan_encode(g, aligned);
    if (c.launcher && !encode_strips_ok(g, plan)) return;       // strips and their tail: where a pipelined call would cut the coding
    std::string &t = out.text;
    t.clear();
    Line l;
    l.f("case tsz=", c.tsz).f(" bands=", c.bands).s(" mode=").s(MODE_NAME[c.mode]).f(" raster=", r.w).f("x", r.h).s(" curve=").s(CURVES[c.curve].name).f(" pointer=+", ENC_PTR[c.ptr])
     .s(" tiles=").s(ENC_TILES_NAME[c.tiles]).f(" value_aligned=", aligned).f(" index=", c.index).s(" table=").s(ENC_TABLE_NAME[c.table]).s(" launcher=").s(ENC_LAUNCHER_NAME[c.launcher])
     .f(" zrun_probe=", c.zrun).s("\n");
    t += l.str();
    const size_t head = t.size();
    static const uint8_t hdr[16] = {0};
    job.out32 = (uint32_t *)0x30000000; job.out_bit0 = 8; memset(&job.st, 0, sizeof(job.st));
    job.ws = ENC_WS; job.tb.ws_pitch = (plan.ws_bytes + 255) & ~(size_t)255;
    job.index = c.index ? (void *)0x60000000 : nullptr;
    job.hdr = hdr; job.hdr_len = 11;
    if (c.table) { job.ix = ix_layout(g, c.table >= 2 ? 2 : 1); job.ix.base = (uint8_t *)0x40000000; job.ix.own_index = c.table == 3; }
    job.zrun_probe = c.zrun != 0;
    g_rec.clear();
    const int rc = enc_launch(g, plan, job, c.launcher);
    static const std::string none;
    finish_case(out, rc, head, geometry_line, none);
}

void run_enc_group(uint32_t tsz, uint32_t mode, Out &out) {
    static const uint32_t BANDS[] = {1, 2, 3, 4, 5, 6, 8, 16};
    EncCase c;
    c.tsz = tsz; c.mode = mode;
    // order x band map: crossed as the decoder's grid crosses them (CURVES) -- the rules ask of the order "Hilbert or Z, or another" and of the
    // map "identity, the default, or neither", one after the other; the Z curve moves the front end of launch_enc_best
    for (uint32_t bands : BANDS) for (c.raster = 0; c.raster < 4; c.raster++) for (c.curve = 0; c.curve < 6; c.curve++) {
        c.bands = bands;
        if (CURVES[c.curve].map == 1 && bands < 3) continue;      // (the default map needs three bands, the other one two)
        if (CURVES[c.curve].map == 2 && bands < 2) continue;
        const Raster &r = ENC_RASTERS[c.raster];
        const Geometry g = make_geometry(r.w, r.h, bands, tsz, mode, CURVES[c.curve].order, CURVES[c.curve].map);
        Line l;
        l.f("  geometry seg_blocks=", g.seg_blocks).f(" nseg=", g.nseg).f(" ulen_sz=", g.ulen_sz).f(" | encode_strip_count=", encode_strip_count(plan_encode(g))).s("\n");
        const std::string geometry_line = l.str();
        out.text = geometry_line;
        out.hash();
        for (c.ptr = 0; c.ptr < 4; c.ptr++) for (c.tiles = 0; c.tiles < 4; c.tiles++) for (c.index = 0; c.index < 2; c.index++) for (c.table = 0; c.table < 4; c.table++) {
            if (c.table == 3 && !c.index) continue;         // the library's own index is an index: own_index without one does not occur
            for (c.launcher = 0; c.launcher < 5; c.launcher++) for (c.zrun = 0; c.zrun < 2; c.zrun++) {
                if (c.launcher && (c.tiles || c.zrun)) continue;      // a pipelined call codes one image and does not probe
                run_enc_case(g, geometry_line, c, out);
            }
        }
    }
}

// plans made for value-aligned memory, launched with memory that is not: refused, nothing launched.  No earlier state of the code can
// produce these lines, so they stay out of the hashes; tests/test_encode_routes.py asserts them one by one
void run_enc_refusals() {
    struct { const char *name; EncKernel kernel; uint32_t tsz, bands, mode; } const R[] = {{"px16", EncKernel::px16, 2, 3, CM_FTL}, {"pxw", EncKernel::pxw, 4, 1, CM_BASE},
                                                                                         {"best_front", EncKernel::best_front, 2, 1, CM_BEST}};
    for (const auto &k : R) for (int how = 0; how < 2; how++) {
        const Geometry g = make_geometry(64, 64, k.bands, k.tsz, k.mode, HILBERT, 0);
        const EncPlan plan = plan_encode(g, true);
        EncJob job;
        memset(&job.st, 0, sizeof(job.st));
        job.img = (const void *)(uintptr_t)(0x10000000 + (how == 0 ? 1 : 0)); job.out32 = (uint32_t *)0x30000000; job.ws = ENC_WS;
        if (how == 1) { job.tb.n = 5; job.tb.src_pitch = (1 << 16) + 1; job.tb.dst_pitch = 1 << 20; job.tb.ws_pitch = (plan.ws_bytes + 255) & ~(size_t)255; }
        g_rec.clear();
        set_error("", 0);
        const int rc = launch_encode(g, plan, job, nullptr);
        printf("refusal kernel=%s planned=%d memory=%s rc=%d records=%d error=%s\n", k.name, plan.kernel == k.kernel, how == 0 ? "odd_pointer" : "odd_pitch", rc, g_rec.n, last_error());
    }
}
}  // namespace

// `plan W H BANDS TSZ MAP ...` (any number of such groups): how plan_encode cuts a common-factor raster into chunks -- blocks a chunk,
// chunks, which front end codes them and which chunks a sample looks at -- for tests/test_best_carry.py, which aims its rasters at the chunks' seams
static int print_plans(int argc, char **argv) {
    for (int i = 2; i + 4 < argc; i += 5) {
        const uint32_t w = (uint32_t)atoi(argv[i]), h = (uint32_t)atoi(argv[i + 1]), bands = (uint32_t)atoi(argv[i + 2]), tsz = (uint32_t)atoi(argv[i + 3]);
        const Geometry g = make_geometry(w, h, bands, tsz, CM_BEST, HILBERT, atoi(argv[i + 4]));
        const EncPlan p = plan_encode(g);
        printf("plan %u %u %u %u %s nbp=%u nchunks=%u front=%s sampled=", w, h, bands, tsz, argv[i + 4], p.nbp, p.nchunks, p.kernel == EncKernel::px_best ? "px_best" : p.kernel == EncKernel::best_front ? "pxw_front" : "enc_front");
        // the chunks a sample looks at, as the sampling kernels take them: best_sample_count of them, evenly spread from chunk 0
        const uint32_t count = best_sample_count(p.nchunks), step = (p.nchunks + count - 1) / count;
        for (uint32_t k = 0; k * step < p.nchunks && k < count; k++) printf("%s%u", k ? "," : "", k * step);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "plan")) return print_plans(argc, argv);
    g_enc = argc > 1 && !strcmp(argv[1], "enc");
    const char *label = argc > 1 + g_enc ? argv[1 + g_enc] : "none";
    prof_enable(1);
    static const uint32_t TSZ[] = {1, 2, 4, 8};
    std::vector<std::string> fnv;
    std::set<std::string> seen;
    for (uint32_t tsz : TSZ) for (uint32_t mode = 0; mode < 3; mode++) {
        Out out;
        out.seen.swap(seen);
        if (g_enc) run_enc_group(tsz, mode, out); else run_group(tsz, mode, out);
        seen.swap(out.seen);
        char buf[160];
        snprintf(buf, sizeof(buf), "fnv switch=%s tsz=%u mode=%s cases=%llu %016llx", label, tsz, MODE_NAME[mode], (unsigned long long)out.cases, (unsigned long long)out.fnv);
        fnv.push_back(buf);
    }
    for (const std::string &s : fnv) puts(s.c_str());
    if (g_enc) run_enc_refusals();
    return 0;
}
