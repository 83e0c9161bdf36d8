// qb3_amd/csrc/qb3_dev.h -- internal interface between the host API (qb3_api.cpp, api_*.cpp) and the HIP kernels
// (k_*.hip; their host side: k_host.hip, k_dec_launch.hip).  Nothing here is exported from the shared library.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace qb3dev {

constexpr int MAXBANDS = 16;
constexpr uint64_t ZCURVE = 0x0145236789cdabefull;   // reference QB3common.h:185
constexpr uint64_t HILBERT = 0x01548cd9aefb7623ull;  // reference QB3common.h:193

enum CodecMode { CM_FTL = 0, CM_BASE = 1, CM_BEST = 2 };   // no step / step / step + common factor + index

// Image geometry and coding parameters shared by encode and decode.
struct Geometry {
    uint32_t w, h, bands, tsz;      // tsz = bytes per value (1,2,4,8)
    uint64_t stride;                // line stride in values
    uint64_t order;                 // curve nibbles, never 0 here
    uint32_t nbx, nby;              // blocks per row / column (ceil)
    uint64_t nblocks;
    uint32_t mode;                  // CodecMode
    uint32_t seg_blocks;            // blocks per index segment
    uint64_t nseg;                  // number of index segments
    uint32_t ulen_sz;               // bytes per entry of the per-unit bit-length table (1, 2; 0 = none); 4: a dword per BLOCK instead
                                    // (8-bit common-factor streams of 1/3/4 bands: the block's bits | entering rungs << 16, four bits a band);
                                    // ULEN_UNIT: a dword per UNIT (every other common-factor stream of several bands: the unit's bits | the rung it is entered with << 16)
    uint8_t cband[MAXBANDS];
};

// Per-band coder state, the reference's band_state (QB3common.h:63-65)
struct BandState {
    uint64_t prev[MAXBANDS];
    uint64_t cf[MAXBANDS];
    uint8_t rung[MAXBANDS];
};

// Decode index, device resident.  Layout in one allocation of index_bytes(g):
//   u64 bitpos[nseg]; T prev[nseg*bands]; T cf[nseg*bands]; u8 rung[nseg*bands]; ulen[nblocks*bands]
// (each 8-byte aligned).  A segment entry is the coder state on entering a run of seg_blocks blocks.  For
// FTL/BASE streams segments are as large as a decoder workgroup and `ulen` holds the bit length of every unit
// (u8 for 8-bit data, u16 otherwise), which is what lets the decoder place every unit with a scan; for the
// common-factor modes segments are short, there is no ulen, and a lane walks each segment serially.
struct IndexView {
    uint64_t *bitpos;
    void *prev;
    void *cf;
    uint8_t *rung;
    void *ulen;
};
size_t index_bytes(const Geometry &g);
IndexView index_view(const Geometry &g, void *base);
uint32_t seg_blocks_for(const Geometry &g);      // needs w, h, bands, tsz, stride, order, mode, cband
uint32_t ulen_size_for(uint32_t tsz, uint32_t mode, uint32_t bands);
constexpr uint32_t ULEN_UNIT = 8;
constexpr uint32_t WIDE_PAD_DW = 40;      // zero words behind the staged words of a 32/64-bit segment (wide_values_lds, qb3_wide.h)
inline size_t ulen_table_bytes(const Geometry &g) { return g.ulen_sz == 4 ? (size_t)g.nblocks * 4 : g.ulen_sz == ULEN_UNIT ? (size_t)g.nblocks * g.bands * 4 : (size_t)g.nblocks * g.bands * g.ulen_sz; }
// common-factor streams whose index holds a dword per BLOCK (its bits | the rungs its units are entered with << 16) for a
// lane-per-block decoder: 8-bit rasters of 1/3/4 bands (four bits a band), 16/32/64-bit rasters of one band (the whole rung)
inline bool best_block_table(uint32_t tsz, uint32_t mode, uint32_t bands) {
    return mode == CM_BEST && ((tsz == 1 && (bands == 1 || bands == 3 || bands == 4)) || (tsz >= 2 && bands == 1));
}

// Rasters of the lane-per-UNIT kernels (k_dec_pxu.hip): every shape no lane-per-block kernel takes -- 8-bit rasters of 2 or more than 4
// bands, 16-bit rasters of an odd band count above 4, 32/64-bit rasters of several bands; of the common-factor streams every one without a
// block table.  A wave owns an index segment of 64 / bands blocks, a lane one unit.  A function of value size, band count and mode
// only: encoder and decoder derive the segment size from it.
inline bool lane_per_unit_shape(uint32_t tsz, uint32_t mode, uint32_t bands) {
    if (bands < 1 || bands > (uint32_t)MAXBANDS) return false;
    if (mode == CM_BEST) return !best_block_table(tsz, mode, bands);
    if (tsz == 1) return !(bands == 1 || bands == 3 || bands == 4);
    if (tsz == 2) return bands > 4 && (bands & 1);
    return bands >= 2;
}

// Waves of one window launch: 2^22 workgroups of four, well inside what a grid may hold (2^32 threads).  A batch beyond it is split in front
// of the window that would exceed it (window_batch_plan); one window alone stays below it with 64, 32 or 21 blocks a segment (at most 2^14
// block rows of 257 segments) ...
constexpr uint64_t WIN_LAUNCH_WAVES = 1ull << 24;
// ... and, for the segments of the lane-per-unit window kernels (k_dec_win_unit.hip: 64 / bands blocks, down to 4), where this says so:
// a window has at most nbx / seg_blocks + 2 waves for each of its block rows (window_desc, qb3_win.h).  Needs nbx, nby, nblocks, seg_blocks.
inline bool window_unit_geometry_ok(const Geometry &g) {
    return g.seg_blocks && (uint64_t)g.nby * (g.nbx / g.seg_blocks + 2) <= WIN_LAUNCH_WAVES && g.nblocks < (1ull << 31);
}

// Results the encoder hands back to the host (device resident, copied once per encode)
struct EncResult {
    uint64_t total_bits;
    uint64_t prev[MAXBANDS];
    uint64_t cf[MAXBANDS];
    uint32_t rung[MAXBANDS];
    // asked for with launch_encode's zrun_probe (the RLE0 modes), counted while the chunks are concatenated:
    uint64_t zero_run;          // byte positions at which four zero bytes in a row start -- at least as many as there are
    uint64_t ff_pairs;          // 0xff bytes followed by another 0xff -- at most as many as there are (rle0_may_win)
    uint64_t zero_dwords;       // aligned all-zero dwords that belong to one chunk of the stream alone -- at most as many as there are
};

// RLE0 (reference QB3encode.cpp:271-332) writes three bytes for every PAIR of 0xff bytes (a run of L of them holds L / 2
// pairs, at least (L - 1) / 2; the stream's last two bytes are copied) and three bytes for 4 + r zero bytes, which saves
// at most one byte per position at which four zero bytes start.  So its output is at least n + ff_pairs / 2 - 1 - zero_run
// bytes, and it can only be shorter than n when that is below n: for most streams the counts decide without the byte pass.
inline bool rle0_may_win(const EncResult &r) { return r.zero_run > 0 && 2 * r.zero_run + 2 > r.ff_pairs; }
// 4 KB of zero bytes hold at least 1022 aligned all-zero dwords, of which at most two per chunk of the stream are shared with a
// neighbour; a chunk is at least min_chunk_bytes long (the plan's blocks per chunk x bands x two bits), so 4 KB touch at most
// 4096 / min_chunk_bytes + 2 of them (the 8-bit lane-per-block plan: 63 bytes, 67 chunks, 888 dwords left); 4 KB of 0xff hold
// three pairs in each of those dwords.  Below both counts the table of one-valued 4 KB chunks the byte pass skips long runs
// by is all "no" and need not be made.  Plans with chunks too short for the count to say anything always make the table.
inline bool rle0_no_uniform_chunk(const EncResult &r, uint64_t min_chunk_bytes) {
    if (min_chunk_bytes < 16) return false;
    const uint64_t shared = 2 * (4096 / min_chunk_bytes + 2);
    return shared < 1000 && r.zero_dwords < 1022 - shared && r.ff_pairs < 1024;
}

// The kernel that codes the units of a raster.  pick_enc_kernel (k_host.hip) is the one place that says which: plan_encode asks it, the
// plan carries the answer, and everything behind the plan -- sizes, arguments, the launch -- reads plan.kernel.
//   generic     a unit per lane, FTL / BASE (k_enc_generic.hip)            best        ... common factor (k_enc_best.hip, FRONT 0)
//   px          8-bit, 1/3/4 bands: a lane per block (k_enc_px.hip)        px_best     ... common factor (k_enc_px_best.hip)
//   px16        16-bit: a lane per block and band group (k_enc_px16.hip)
//   pxw         32/64-bit, one band: a lane per block (k_enc_pxw.hip)      best_front  16/32/64-bit, one band, common factor: k_enc_best.hip
//                                                                                      behind its lane-per-block front end (FRONT 1 Hilbert, 2 Z curve)
// px16, pxw and best_front read values at their natural alignment: they need value-aligned memory.
enum class EncKernel { generic, px, px16, pxw, best, best_front, px_best };
// value-aligned memory: the image pointer and the pitches between tiles, OR-ed into `bits`, are multiples of the value size.  What the
// callers of plan_encode ask of the memory they will launch with, and what make_enc_args checks of the memory a launch is given
inline bool value_aligned_memory(uint32_t tsz, uint64_t bits) { return (bits & (tsz - 1)) == 0; }

// How a raster is coded: the kernel, its workgroups and its workspace
struct EncPlan {
    EncKernel kernel;
    bool rgb;               // px, px_best, px16: the default R-G,G,B-G map (else identity)
    uint32_t px16_bg, px16_ng;      // px16: bands per lane (1..4), lanes per block (else 0)
    uint32_t threads;       // workgroup size = units per chunk (incl. halo units)
    uint32_t slots;         // block slots per chunk, slot 0 is the halo block
    uint32_t nbp;           // payload blocks per chunk
    uint32_t nchunks;
    size_t lds_bytes;
    size_t ws_bytes;        // chunk counts/offsets, seam table, per-chunk scratch slots, EncResult (last)
};
// value_aligned: as above, of the memory the launches will get.  Where it is not, the 16-bit and one-band 16/32/64-bit lane-per-block
// kernels cannot read the raster and the plan is the unit-per-lane kernels' own -- their chunks, their LDS.  A plan made for aligned
// memory and launched with other memory is refused (make_enc_args, k_host.hip), not handed to another kernel
EncPlan plan_encode(const Geometry &g, bool value_aligned = true);
// payload blocks a chunk of the 8-bit FTL/BASE lane-per-block encoder (k_enc_px.hip) codes: a multiple of four, so that every
// four-block group of a level-2 restart table entry (five bytes) belongs to one workgroup, which writes it
constexpr uint32_t PX_NBP = 252;
constexpr uint32_t PXB_LDS_FIXED = 11664;      // LDS of the 8-bit common-factor lane-per-block encoder in front of its bit buffer

// Optional restart table carried INSIDE the container as ignorable chunks ("ix", include/qb3x.h): K entries, one per
// `blocks` blocks: [bit position, 6 bytes][rung, 1 byte per band][prev, tsz bytes per band][cf, the same,
// common-factor modes only].  A chunk holds at most 64 KB, so the table is a run of chunks of `per_chunk` entries
// (the last one may hold fewer), each [12-byte head][entries][4-byte "zz" pad chunk]; `base` points at the first
// chunk's first byte.  With it a stream that arrives without the out-of-band index is walked from K points at once.
constexpr uint32_t IX_HEAD = 12, IX_PAD = 4;
constexpr uint32_t IX_BL_BITS_WIDE = 12;  // ... of a unit length in a table of 32/64-bit data (a unit is at most 1048 bits; two fields are three whole bytes)
constexpr uint32_t IX_BL_BITS = 10;       // bits of a block length in a table entry (8-bit data, at most four bands: 4 x 149 < 1024)
struct IxTable {
    uint8_t *base = nullptr;        // device pointer (encode: where the chunks go, "DT" follows; decode: where they are)
    uint32_t K = 0, blocks = 0, entry_bytes = 0, per_chunk = 0;
    bool pads = true;               // false: a version 1 table (one chunk, no pad chunk behind it)
    uint32_t version = 3;           // decode: what the chunks say (3: every chunk carries a 16-bit check of its entries in the head's reserved bytes)
    bool check_heads = false;       // decode: the chunk heads behind the first were not read on the host: the check kernel looks at them
    bool block_lens = false;        // entries carry the bit length of every block of their segment (10 bits each): 8-bit lane-per-block rasters
    bool own_index = false;         // encode: the index is the library's own, only sampled for the table -- no unit lengths needed
};
uint32_t ix_entry_bytes(const Geometry &g, bool block_lens = false);
bool ix_block_lens_ok(const Geometry &g);         // can a table for this geometry carry block lengths
uint32_t ix_bl_fields(const Geometry &g);         // ... how many fields an entry then ends with
uint32_t px16_bands_per_lane(const Geometry &g);  // 16-bit lane-per-block kernels: bands a lane owns (0: the split does not apply)
inline uint32_t ix_bl_bits(uint32_t tsz) { return tsz >= 4 ? IX_BL_BITS_WIDE : IX_BL_BITS; }
constexpr uint32_t IX_BL_BEST_BYTES = 3;  // ... of a block's field in a table of 8-bit common-factor data: the block's bits (12) | the rungs its units are entered with (3 bits a band) << 12
// bytes of the fields behind the fixed part of an entry that covers `blocks` blocks (cf: the stream is a common-factor one)
// (rasters of the lane-per-unit kernels: a field per UNIT -- three bytes in a common-factor table (the unit's bits | the rung it is
// entered with << 12), twelve bits of length otherwise, whatever the value size)
inline uint32_t ix_bl_bytes(uint32_t tsz, uint32_t bands, uint32_t blocks, bool cf) {
    const bool per_unit = lane_per_unit_shape(tsz, cf ? CM_BEST : CM_FTL, bands);
    if (cf) return IX_BL_BEST_BYTES * blocks * (per_unit ? bands : 1u);
    if (per_unit) return (blocks * bands * IX_BL_BITS_WIDE + 7) / 8;
    const uint32_t fields = tsz == 1 ? blocks : tsz == 2 ? (bands == 1 ? 64u : 128u) : blocks * bands;
    return (fields * ix_bl_bits(tsz) + 7) / 8;
}
// the table this library writes for a geometry (needs seg_blocks, nseg, bands, tsz, mode); K == 0: none
IxTable ix_layout(const Geometry &g, int level = 1);       // level 2: with block lengths where the geometry allows
inline size_t ix_chunks(const IxTable &t) { return t.per_chunk ? (t.K + t.per_chunk - 1) / t.per_chunk : 0; }
inline size_t ix_total_bytes(const IxTable &t) { return ix_chunks(t) * (IX_HEAD + (t.pads ? IX_PAD : 0)) + (size_t)t.K * t.entry_bytes; }

// Batched tiles: n images/streams laid out at fixed byte pitches, processed by one set of launches (blockIdx.y).
// n == 0 means a single image.  ws_pitch = plan.ws_bytes of one tile; idx_pitch = index_bytes of one tile.
struct TileBatch { uint32_t n = 0; uint64_t src_pitch = 0, dst_pitch = 0, ws_pitch = 0, idx_pitch = 0; uint64_t max_bits = 0; /* decode: the longest stream */
    // A tile GRID (the tiles of a mosaic where they lie in the raster): cols > 0 makes launch tile t tile (t / cols, t % cols); images, containers
    // and the caller's index then go *_row bytes from row to row and *_pitch bytes from column to column (n is a multiple of cols).  The
    // workspace, the stream lengths and the status words stay indexed by t.  cols == 0: one row of n tiles, the *_row fields are not read.
    uint32_t cols = 0; uint64_t src_row = 0, dst_row = 0, idx_row = 0; };
// what the kernels divide by (EncArgs / DecArgs::tcols, tmagic, the three pitch pairs): one row of tiles takes no division at all (magic 0),
// a column of tiles is a row whose column pitch is the row pitch
struct TileGridRule { uint32_t cols, magic; uint64_t src, src_row, dst, dst_row, idx, idx_row; };
TileGridRule make_tile_grid(const TileBatch &tb);
inline uint64_t tile_pitch_bits(const TileGridRule &r, bool dst) { return dst ? (r.dst | r.dst_row) : (r.src | r.src_row); }     // low bits set: some tile is off that alignment
// Plain 8- and 16-bit streams (no index, no restart table) are walked through a table of unit lengths by position (k_dec_walk.hip).
// walk_table_bytes: memory that takes the whole call in one round; less means more rounds, down to walk_table_min_bytes.
size_t walk_table_bytes(uint32_t ntiles, uint64_t max_bits, uint32_t tsz);
size_t walk_table_min_bytes(uint32_t ntiles, uint32_t tsz);
size_t walk_memory_bytes(const Geometry &g, uint32_t ntiles, uint64_t max_bits);     // what the walk that will run for this raster wants (exits need far less than chains)
size_t walk_table_cap();                // what a decoder allocates at most (1 GiB; QB3_WALK_TAB_KB overrides)
struct DecPlan;
bool walk_table_applies(const Geometry &g, const DecPlan &plan);

// Encode the block stream of one image: what a launch codes, from where, to where.  All pointers are device pointers.
struct EncJob {
    const void *img = nullptr;      // image, g.tsz-byte values
    uint32_t *out32 = nullptr;      // 4-byte aligned address at or below the first stream byte
    uint32_t out_bit0 = 0;          // bit offset of the first stream bit relative to out32 (multiple of 8, < 32)
    BandState st;                   // initial band state (host copy, passed by value to the kernels)
    void *ws = nullptr;             // workspace of plan.ws_bytes; the EncResult is its LAST sizeof(EncResult) bytes
    void *index = nullptr;          // optional decode index (nullptr = none)
    TileBatch tb;
    const uint8_t *hdr = nullptr;   // container header stamped before each stream
    uint32_t hdr_len = 0;
    IxTable ix;                     // base == nullptr when no table is wanted
    bool zrun_probe = false;        // count runs of zero bytes and pairs of 0xff while concatenating (EncResult::zero_run, ff_pairs)
};
// Launches on `stream`, does not synchronise.  Returns hipError_t as int; -1, with nothing enqueued, for a value size that is none, or
// when the plan's kernel needs value-aligned memory and job.img or a tile pitch is not
int launch_encode(const Geometry &g, const EncPlan &plan, const EncJob &job, void *stream);

// Strips of a pipelined host call (k_host.hip): can this coding be cut into strips; how many; blocks of the raster a strip and
// its predecessors cover (what must be in device memory before it is coded); where the running stream length behind a strip is
bool encode_strips_ok(const Geometry &g, const EncPlan &plan);
uint32_t encode_strip_count(const EncPlan &plan);
uint64_t encode_strip_blocks(const EncPlan &plan, uint32_t strip);
const uint64_t *encode_strip_total(const Geometry &g, const EncPlan &plan, void *ws, uint32_t strip);
int launch_encode_strip(const Geometry &g, const EncPlan &plan, const EncJob &job, void *stream, uint32_t strip);
int launch_encode_tail(const Geometry &g, const EncPlan &plan, const EncJob &job, void *stream);

// What decodes a raster.  The bool flags say that a kernel APPLIES to the geometry (plan_decode); which one a launch uses, given the
// pointers it gets, is decided in one place: pick_dec_kernel (k_dec_launch.hip), and what runs in front of it next to that (DecFront).
struct DecPlan {
    uint32_t threads;       // lanes per workgroup, one index segment per lane
    uint32_t nwg;
    size_t lds_bytes;
    size_t ws_bytes;        // scratch for the foreign-stream path: rebuilt index + status word
    // unit-parallel kernel (FTL/BASE with ordinary band maps): one workgroup per index segment
    bool fast;
    uint32_t threads2, bpp, passes, in_cap_dw;
    size_t lds2_bytes;
    // 8-bit 1/3/4-band lane-per-block kernel
    bool px, px_rgb;
    size_t lds_px;
    uint32_t px_cap_dw;     // staging capacity (dwords) of the lane-per-block kernels, per wave
    bool px16;              // 16-bit lane-per-(block, band group) kernel applies
    uint32_t px16_bg, px16_ng;
    bool px_best;           // 8-bit common-factor streams: the lane-per-block decoder applies (k_dec_px_best.hip)
    bool pxw;               // 32/64-bit single-band FTL/BASE streams: the lane-per-block decoder applies (k_dec_pxw.hip)
    bool pxw_best;          // ... and its common-factor counterpart (dec_pxw_best_kernel)
    size_t lds_pxw;
    bool pxu, pxu_best;     // the lane-per-unit decoders apply (k_dec_pxu.hip: lane_per_unit_shape): FTL / BASE, common factor
};
DecPlan plan_decode(const Geometry &g);
// LDS of the decoders that stage a wave's segment, from px_cap_dw: 16-bit data (table, four waves' staging); 32/64-bit data (FTL / BASE: a 2 KB table in front)
inline size_t px16_lds_bytes(uint32_t cap_dw) { return 4096 + 4 * 4 * ((size_t)cap_dw + 16); }
inline size_t pxw_lds_bytes(uint32_t cap_dw, bool table) { return (table ? 2048 : 0) + 4 * 4 * ((size_t)cap_dw + WIDE_PAD_DW); }

// The kernel that decodes the units of a launch: the one of the plan's that applies and whose alignment needs the image pointer and the tile pitch (bytes)
// meet, else the generic one (the unit-parallel workgroup for FTL / BASE streams it takes, else a lane per segment).
enum class DecKernel { generic, px, px16, pxw, pxu, px_best, pxw_best, pxu_best };
DecKernel pick_dec_kernel(const Geometry &g, const DecPlan &plan, const void *img, uint64_t pitch);
inline DecKernel aligned_dec_kernel(const Geometry &g, const DecPlan &plan) { return pick_dec_kernel(g, plan, nullptr, 0); }   // ... with aligned memory

struct DecStrip { uint64_t seg0, nseg; bool first; };     // first: zero the status words, check the table; later strips skip both
// Decode a block stream.  in32/in_bit0 locate the first stream bit like out32/out_bit0 above; in_bits is
// the stream length in bits (bytes*8).  index == nullptr: the index is first rebuilt in ws by a serial
// boundary scan on the GPU.  status (device u32 inside ws, zeroed here) gets nonzero on decode failure.
// Returns hipError_t as int; does not synchronise.
int launch_decode(const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                  void *img, const void *index, void *ws, uint32_t **status_out, void *stream, const TileBatch &tb = TileBatch(),
                  const uint64_t *tile_bits = nullptr,     // tile_bits: device array, stream length of each tile in bits
                  const IxTable &ix = IxTable(),
                  void *walk_tab = nullptr, size_t walk_tab_bytes = 0,     // table memory for plain 8-bit streams (null: the one-wave walk)
                  bool full_staging = false,    // 16-bit data: worst-case LDS staging (after a call that ended with status bit 4)
                  uint32_t wide_band = 16,      // plain 32/64-bit streams: rungs the walk's table covers (16; 14: byte entries, 8: half rows -- QB3_WIDE_BAND, test hooks; the first
                                                // unit of a block row, entered from the far end of the row before, sits many rungs above its neighbours)
                  const DecStrip *strip = nullptr);     // a strip of a pipelined host call (decode_strips_ok): only these segments, from the container's table; value-aligned img and pitch, else refused

// can a container's table (with block fields, an entry per index segment) be decoded strip by strip: one launch of a
// lane-per-block decoder per range of segments, nothing else
bool decode_strips_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix);

// Window decode: a rectangle of the raster from the container's restart table, only the index segments that hold one of its blocks
// (mapping, clipping and trust: the head of k_dec_win.hip).  x0, y0, w, h in raster pixels; stride: values between the rows of the
// destination, which receives the window alone.
struct WinRect { uint32_t x0, y0, w, h; uint64_t stride; };
// the window's blocks, both ends included, by the geometry rule: pixel x is held by block min(x / 4, nbx - 1) -- the last block column /
// row is shifted, not padded.  The caller has checked that the window is not empty and lies inside the raster.
struct WinBlocks { uint32_t bx0, bx1, by0, by1; };
inline WinBlocks window_blocks(const Geometry &g, uint64_t x0, uint64_t y0, uint64_t w, uint64_t h) {
    return WinBlocks{ (uint32_t)std::min<uint64_t>(x0 / 4, g.nbx - 1), (uint32_t)std::min<uint64_t>((x0 + w - 1) / 4, g.nbx - 1),
                      (uint32_t)std::min<uint64_t>(y0 / 4, g.nby - 1), (uint32_t)std::min<uint64_t>((y0 + h - 1) / 4, g.nby - 1) };
}
// table chunks an entry of the window is read from: the chunk of its first segment's entry to the chunk of the entry behind its last
// segment, whose position ends it (K entries, per_chunk a chunk)
inline void window_chunk_range(const Geometry &g, const WinBlocks &b, uint32_t K, uint32_t per_chunk, uint32_t *c0, uint32_t *c1) {
    const uint64_t first = ((uint64_t)b.by0 * g.nbx + b.bx0) / g.seg_blocks, last = std::min<uint64_t>(((uint64_t)b.by1 * g.nbx + b.bx1) / g.seg_blocks + 1, K - 1);
    *c0 = (uint32_t)(first / per_chunk); *c1 = (uint32_t)(last / per_chunk);
}
// index segments of the raster that hold a block of the window (pure geometry: needs w, h, nbx, nby, seg_blocks; 0: the window is
// empty or not inside the raster)
uint64_t window_segments(const Geometry &g, const WinRect &r);
// behind a strip of launch_decode (which has checked the table): status bit 2 when the table's last entry lies beyond the stream's end
// -- a stream cut short, which only the whole decode may judge
int launch_window_tail_check(const Geometry &g, uint64_t in_bits, uint32_t *status, void *stream, const IxTable &ix);

// The window kernels come in FAMILIES, one per wave routine, each with a record (WinKernels) in the file that holds its kernels.  A
// family's predicate asks decode_strips_ok, a table with the fields its whole-raster decoder takes a segment from alone, and ONE answer
// of aligned_dec_kernel -- so at most one family takes a raster:
//   family   record in                 rasters (aligned_dec_kernel)                         table                 switch            dst     ranged
//   win_u8   k_dec_wins.hip            8-bit, 1/3/4 bands, FTL / BASE (px)                  level 2               always on         any     yes
//   win_u16  k_dec_win16.hip           16-bit, 1/2/3/4/6/8 bands, FTL / BASE (px16)         level 2, version 3    U16               2       yes
//   win_cf8  k_dec_win_best.hip        8-bit, 1/3/4 bands, common factor (px_best)          level 1 or 2          CF8               any     yes
//   win_unit k_dec_win_unit.hip        lane-per-unit and one-band 32/64-bit rasters,        level 2, version 3    UNIT              value   no
//                                      FTL / BASE (pxu, pxw), window_unit_geometry_ok
//   win_cfu  k_dec_win_best_unit.hip   the common-factor streams of such shapes and of      level 1 or 2, v. 3    CFU               value   no
//                                      one-band 16-bit rasters (pxu_best, pxw_best), window_unit_geometry_ok
// (switch: the bit of qb3x_set_decoder_window_kernels (include/qb3x.h) the handle must have set; dst: bytes every destination must be a multiple of.)
// Each family has up to three FORMS, one kernel shell each (qb3_win.h): a single window as kernel arguments, a batch of windows from a
// descriptor array, a batch decoded from fetched pieces of the container (ranged).  A dispatcher launches the shell's instantiation
// that the geometry and the plan select.
struct DecArgs; struct WinArgs; struct WinBatchArgs; struct WinRangedArgs; struct WinMosaicArgs;      // (qb3_kernels.h, qb3_win.h)
struct WinLaunch { uint32_t grid; size_t lds; void *stream; };
struct WinKernels {
    bool (*ok)(const Geometry &, const DecPlan &, const IxTable &);     // does the raster and its table qualify
    unsigned bit;                                                       // the switch that enables the family (0: always on)
    uint32_t (*align)(const Geometry &);                                // bytes every destination must be a multiple of (a power of two)
    void (*more_args)(DecArgs &, const DecPlan &);                      // what its wave routine takes besides window_dec_args (null: nothing)
    size_t (*lds)(const Geometry &, const DecPlan &);                   // dynamic LDS of a launch
    const char *noun, *prof, *prof_ranged;                              // in front of "window ..." in error texts; profile names
    void (*one)(const Geometry &, const DecPlan &, const WinArgs &, const WinLaunch &);
    void (*batch)(const Geometry &, const DecPlan &, const WinBatchArgs &, const WinLaunch &);
    void (*ranged)(const Geometry &, const DecPlan &, const WinRangedArgs &, const WinLaunch &);    // null: the family has no ranged form
    void (*batch_sel)(const Geometry &, const DecPlan &, const WinBatchArgs &, const WinLaunch &);  // the batch form that writes selected bands only (null: the family has none)
    void (*mosaic)(const Geometry &, const DecPlan &, const WinMosaicArgs &, const WinLaunch &);    // a batch over the tiles of a mosaic, a container a piece (null: the family has none)
    const char *prof_mosaic;                                                                        // ... its profile name
};
const WinKernels &win_u8(), &win_u16(), &win_cf8(), &win_unit(), &win_cfu();
bool decode_window_ok(const Geometry &g, const DecPlan &plan, const IxTable &ix);        // win_u8's predicate (k_dec_win.hip)
// The family that takes a raster and its table on a handle with these switches (mask), or null.  The order of the questions
// carries no meaning: every predicate requires another answer of aligned_dec_kernel (pick_dec_kernel, k_dec_launch.hip, returns one
// DecKernel for a geometry and plan: px; px16; px_best; pxu or pxw; pxu_best or pxw_best), so no two families qualify.  The caller
// applies the family's alignment to its destinations; one that misses it leaves no family at all, since no other can qualify.
const WinKernels *window_family(const Geometry &g, const DecPlan &plan, const IxTable &ix, unsigned mask);

// One window, one launch (its first workgroups check the table chunks the window's entries are read from); status: a device word of the
// caller's, zeroed here -- nonzero afterwards means "do not trust the window's bytes".  Does not synchronise.  Returns hipError_t as int.
int launch_decode_window(const WinKernels &k, const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                         void *dst, const WinRect &r, uint32_t *status, void *stream, const IxTable &ix);
// A batch of windows of one raster: one launch decodes all of them, a status word per window.  window_batch_plan fills n descriptors of
// WIN_DESC_BYTES each at `descs` (host memory the caller then copies to the device as it is), the sorted list of table chunks the
// launch has to check (window_chunk_list), and the sum of the windows' segment counts; it returns the list's length.
// launch_decode_windows takes the descriptors' host and device copies, the chunk list on the device and n + 1 zeroed status words
// (word 0: the table's checks, call wide; word 1 + i: window i).  Does not synchronise.  Returns hipError_t as int.
constexpr size_t WIN_DESC_BYTES = 64;
// (WIN_LAUNCH_WAVES, the waves of one launch: above, at window_unit_geometry_ok)
void window_chunk_list(const Geometry &g, uint32_t K, uint32_t per_chunk, const WinRect *rects, size_t n, std::vector<uint32_t> &chunks);     // ... and the table's last chunk: the tail check reads the last entry
size_t window_batch_plan(const Geometry &g, const IxTable &ix, const WinRect *rects, void *const *dsts, size_t n, void *descs,
                         std::vector<uint32_t> &chunks, uint64_t *segments);
int launch_decode_windows(const WinKernels &k, const Geometry &g, const DecPlan &plan, const uint32_t *in32, uint32_t in_bit0, uint64_t in_bits,
                          const void *h_descs, const void *d_descs, size_t n, const uint32_t *d_chunks, size_t nchunks,
                          uint32_t *d_status, void *stream, const IxTable &ix,
                          const uint8_t *sel = nullptr, uint32_t nsel = 0);
// (sel: the band-selected form of a family that has one (WinKernels::batch_sel; window_sel_fused says when it applies): a pixel of every
// window is the nsel values of bands sel[0 .. nsel), the descriptors' strides count those.)
// Band-selected windows (qb3x_decode_windows_bands_device).  The fused form writes the selection straight from the window kernel; every
// other case decodes full-band pixels into memory of the handle's and picks the bands with win_band_gather_kernel (k_win_bands.hip):
// a descriptor a window -- where its full-band pixels are (src: the first value of the window's first pixel; spitch: bytes between
// its rows; sbands: values a source pixel), where the selected ones go (dst at any address, dstride bytes between rows) -- and ONE
// launch for n of them.  quanta > 1: the values are multiplied back as launch_dequantize does it (dtype: the handle's qb3_dtype).
struct WinGather { const void *src; uint64_t spitch; void *dst; uint64_t dstride; uint32_t w, h, sbands, pad_; };
constexpr size_t WIN_GATHER_BYTES = 48;
inline bool window_sel_fused(const WinKernels *k, const Geometry &g, uint32_t nsel) { return k && k->batch_sel && g.seg_blocks * nsel <= 64; }
int launch_window_gather(const void *d_descs, size_t n, uint64_t max_rows, const uint8_t *sel, uint32_t nsel, int dtype, uint64_t quanta, void *stream);
// The same from PIECES of the container (api_ranged.cpp fetches them), for a family that has the form: d_pieces: npieces >= 1 pieces
// sorted by first segment, each a run of consecutive segments { seg0, nseg, ent0, word0, stream word of its first packed word (low,
// high), nwords, 0 }; d_entries: the compact array of table entries (ix.entry_bytes each), nseg + 1 per piece from index ent0; d_words:
// the pieces' stream words from index word0, counted as launch_decode's in32 counts them (word 0 holds the bit in_bit0 names).  The
// caller vouches that ent0 + nseg + 1 and word0 + nwords stay inside the two arrays: the kernel reads nothing outside them.  The
// descriptors are window_batch_plan's; status words as above, word 0 is not written (the table was checked on the host).  ix: the
// table's shape (its base only has to be non-null).  Destinations aligned as the family asks.
constexpr size_t WIN_PIECE_BYTES = 32;
int launch_decode_windows_ranged(const WinKernels &k, const Geometry &g, const DecPlan &plan, uint32_t in_bit0, uint64_t in_bits, const void *h_descs,
                                 const void *d_descs, size_t n, const void *d_pieces, size_t npieces, const void *d_entries, const uint32_t *d_words,
                                 uint32_t *d_status, void *stream, const IxTable &ix);

// Mosaic windows (k_dec_wins_mosaic.hip, api_mosaic_windows.cpp): the batch form over MANY containers of one shape -- the tiles of a mosaic.
// A descriptor is a PIECE, the part of a window that lies in one tile, in that tile's coordinates (window_desc; its destination already
// where the piece lies in its window), and names its tile in the descriptor's spare dword: an index into an array of WinTile in device
// memory, from which the wave takes the three things that differ between tiles -- where the stream starts, how long it is, where the
// table is.  Geometry, the table's shape and in_bit0 are those of tile 0 for every tile.  The launch's first nchecks workgroups check
// one table chunk of one tile each (WinTileCheck; the entry of a tile's LAST chunk has WIN_TILE_TAIL set: its workgroup also makes the
// tail check against that tile's stream length and compares the tile's mode byte, "ix" tag and "DT" mark with tile 0's: mode_byte at
// byte 10 of the container, the tag ix_off bytes in, the mark in front of byte hdr).  d_status: 1 + n + ntiles zeroed words -- word 0 is
// not written, word 1 + i is piece i's, word 1 + n + t is tile t's (a failed check).  The descriptors' wave0 prefixes start again where a
// launch would exceed WIN_LAUNCH_WAVES, as window_batch_plan's do.  Does not synchronise.  Returns hipError_t as int.
struct WinTile { const uint32_t *in32; uint64_t in_bits; const uint8_t *ix; uint64_t pad_; };
struct WinTileCheck { uint32_t tile, chunk; };
constexpr size_t WIN_TILE_BYTES = 32, WIN_TILE_CHECK_BYTES = 8;
constexpr uint32_t WIN_TILE_TAIL = 1u << 31;
// fills n piece descriptors of WIN_DESC_BYTES each at `descs` (host memory that goes up as it is): piece i is rects[i] of tile record
// tiles[i], written to dsts[i]; *segments: the sum of the pieces' segment counts
void window_mosaic_plan(const Geometry &g, const WinRect *rects, void *const *dsts, const uint32_t *tiles, size_t n, void *descs, uint64_t *segments);
int launch_decode_windows_mosaic(const WinKernels &k, const Geometry &g, const DecPlan &plan, uint32_t in_bit0, const void *h_descs, const void *d_descs,
                                 size_t n, const void *d_tiles, size_t ntiles, const void *d_checks, size_t nchecks, uint32_t *d_status, void *stream,
                                 const IxTable &ix, uint32_t ix_off, uint32_t hdr, uint32_t mode_byte);

// Mosaics (k_mosaic.hip): the tiles that cross a raster's right or bottom edge are coded from, and decoded into, memory of the handle's.
// One descriptor a tile and ONE launch for n of them copies the rows of a rectangle and, where the destination is larger, repeats the
// rectangle's last pixel to the right and its last row downwards: src to dst, spitch / dpitch bytes between rows, cw bytes of ch rows
// copied, ow >= cw bytes of oh >= ch rows written.  pad (raster -> tile): ow x oh is the tile; crop (tile -> raster): ow == cw, oh == ch.
// No byte outside the ow x oh destination is written, none outside the cw x ch source is read.
struct MosaicRect { const void *src; uint64_t spitch; void *dst; uint64_t dpitch; uint32_t cw, ch, ow, oh; };
constexpr size_t MOSAIC_RECT_BYTES = 48;
int launch_mosaic_rects(const void *d_descs, size_t n, uint32_t max_rows, uint32_t pixel_bytes, bool pad, void *stream);

// Reindex (k_reindex.hip): the table chunks this library's encoder writes for a raster, made from the index a plain walk of its stream
// has rebuilt (launch_decode with index == nullptr leaves it in ws behind the status words), and the new container around them.
// launch_reindex_fill writes the entries of the table laid out by ix (ix.base: where its first chunk goes) from the index at `index`.
// launch_reindex_finish, in one launch: hdr_len header bytes from HOST memory at hdr to d_dst (when there is no table they end with "DT");
// every chunk's head, pad and check and the "DT" behind the last (ix.K == 0: no table); the n coded bytes at d_src to d_pay, which
// may stand at any byte distance from each other.  Neither synchronises.  Both return hipError_t as int.
int launch_reindex_fill(const Geometry &g, void *index, const IxTable &ix, void *stream);
int launch_reindex_finish(const Geometry &g, const IxTable &ix, const uint8_t *hdr, size_t hdr_len, void *d_dst, const void *d_src, void *d_pay, uint64_t n, void *stream);
constexpr size_t DEC_WS_INDEX_OFF = 64;     // a single image's rebuilt index in the decoder's workspace: behind the status words

// The RLE0 byte pass of the *_RLE modes on device buffers (k_rle0.hip; reference QB3encode.cpp:271-332, QB3decode.cpp:267-307).
// ws: rle0_ws_bytes(n) bytes of device memory.  rle0_device_size returns the size of the coded (decode = false) or
// expanded (decode = true) form and synchronises the stream; rle0_device_write, called next with the same arguments,
// writes it (does not synchronise).
size_t rle0_ws_bytes(uint64_t n);
int rle0_device_size(const void *d_src, uint64_t n, void *ws, bool decode, uint64_t *total, void *stream, bool no_uniform_chunk = false);     // no_uniform_chunk: the caller knows that no 4 KB of the bytes hold one value only
int rle0_device_write(const void *d_src, uint64_t n, void *ws, bool decode, void *d_dst, void *stream);


// Elementwise helpers on device buffers (quantisation, reference QB3encode.cpp:137-186 / QB3decode.cpp:77-107)
int launch_quantize(void *dst, const void *src, const Geometry &g, int dtype, uint64_t q, bool away, void *stream);
int launch_dequantize(void *img, const Geometry &g, int dtype, uint64_t q, void *stream);

// Optional per-kernel timing with HIP events recorded on the launch stream (off by default).
void prof_enable(int level);        // 0 off, 1 every kernel, 2 the long kernels only (less event traffic)
void prof_reset();
void prof_collect();                                    // call after the stream was synchronised
bool prof_get(const char *name, double *total_ms, uint64_t *count);
int  prof_names(char *buf, size_t bufsize);             // comma separated kernel names seen so far

const char *last_error();
void set_error(const char *what, int hip_err);

}  // namespace qb3dev
