/*
 * include/qb3x.h -- extensions of the MI355X-native QB3 library that the reference does not have:
 * device-resident buffers, an out-of-band decode index, batched tiles.  The reference API (QB3.h)
 * only knows host pointers and one image per call (reference QB3lib/QB3.h:119-139).
 *
 * Why an index: a QB3 block stream has no restart points; a unit's bit position and rung depend on
 * every earlier unit (reference QB3decode.h:445-454), so a foreign stream can only be parsed
 * serially.  The encoder here can emit, next to the (bit-identical) stream, a small side table:
 * for every SEGMENT of `seg_blocks` consecutive 4x4 blocks the bit position of its first unit and the
 * per-band encoder state {previous value, rung, common factor} on entry -- i.e. the band_state the
 * reference keeps in its handle (reference QB3common.h:63-65), sampled along the stream.  With it,
 * decode is parallel over segments.  Without it the library first rebuilds the table on the GPU with
 * a serial boundary scan of the stream (slow, latency bound), then decodes in parallel.
 *
 * `stream` arguments are hipStream_t passed as void* (NULL = the default stream).  All `d_` pointers
 * are device pointers on the current HIP device.
 */
#ifndef QB3_AMD_QB3X_H
#define QB3_AMD_QB3X_H
#include "QB3.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Number of usable HIP devices; 0 means the library cannot encode or decode. */
int qb3x_device_count(void);

/* Device buffers of destroyed handles are kept (at most 24 buffers, 3 GiB) for the next handle of the process, so that a
 * caller who opens, decodes and closes a container per tile does not pay hipMalloc / hipFree every time; qb3x_trim returns
 * them to the HIP runtime.  (No counterpart in the reference, which owns no device memory.) */
void qb3x_trim(void);

/* Diagnostic: the status bits of the decoder handle's last decode call.  Bits 0, 1, 3, 4 are errors (the call returned 0),
 * bit 2 "the stream ended early" (the reference's reader clamps, QB3decode bitstream.h:36), bit 5 "the container's restart
 * table failed its check and was not used", bit 6 "a plain stream's walk by exits handed super-windows to its one hopping
 * lane" (slower, same pixels). */
unsigned qb3x_last_decode_status(const decsp p);

/* Bytes of device memory an index for this encoder's geometry needs (0 on error). */
size_t qb3x_index_size(const encsp p);
/* Same, from a decoder handle (valid after qb3_read_info). */
size_t qb3x_decoder_index_size(const decsp p);

/* Device-resident encode.  d_src: image laid out as qb3_encode expects; d_dst: at least
 * qb3_max_encoded_size(p) bytes, 4-byte aligned; d_index: qb3x_index_size(p) bytes or NULL.
 * Writes the complete QB3 container (headers + stream, STORED fallback included) to d_dst.
 * Returns its size in bytes, 0 on error (see qb3_get_encoder_state).  Synchronises `stream` once,
 * to learn the stream length.  Mode, band map, stride and handle statefulness as qb3_encode. */
size_t qb3x_encode_device(encsp p, const void *d_src, void *d_dst, void *d_index, void *stream);

/* Device-resident decode.  p: handle from qb3_read_start + qb3_read_info over a HOST copy of at least
 * the headers (source_size must be the true stream size); d_src: device copy of the whole container
 * (same bytes, 4-byte aligned); d_dst: qb3_decoded_size(p) bytes; d_index: index written by
 * qb3x_encode_device for this very stream, or NULL to rebuild it with the serial scan.
 * Returns decoded bytes, 0 on error. */
size_t qb3x_decode_device(decsp p, const void *d_src, void *d_dst, const void *d_index, void *stream);

/* Window decode: a rectangle of the raster without decoding all of it.  No counterpart in the reference, whose stream has no
 * restart points (QB3decode.h:445-454); here a container written with qb3x_set_encoder_index_chunk(p, 2) has one per index segment.
 * Decodes the w x h pixel window whose top-left pixel is (x0, y0) of the raster handle p describes.  d_src, d_index, stream: as
 * qb3x_decode_device.  d_dst receives h rows of w * bands values; dst_stride is the distance between rows IN VALUES (0: w * bands),
 * the convention of qb3_set_decoder_stride; the handle's own stride setting is not used by this call.  Returns the bytes of the
 * window (h * w * bands * value size), 0 on error.
 * The bytes are, for every container and handle setting (compat flags, quanta, band map, scan order), exactly the crop of what
 * qb3x_decode_device would write, and the call fails where that call fails, with the same error.  How it gets there
 * (qb3x_last_window_path):
 *   1  8-bit rasters of 1, 3 or 4 bands, FTL / BASE, level-2 table in the container, d_index NULL: one kernel decodes the index
 *      segments that hold a block of the window -- and no others -- straight into d_dst; of the table only the chunks the window's
 *      entries are read from are checked and read.  Time and memory follow the window, not the raster.
 *      On a handle with qb3x_set_decoder_window_kernels(p, QB3X_WINK_U16) path 1 also takes 16-bit rasters of 1, 2, 3, 4, 6 or 8
 *      bands (FTL / BASE, level-2 table of version 3, d_dst on an even address; else they go as below): the same, with the
 *      raster's blocks per segment (64, 32 for eight bands, 21 for six) -- time follows the window, and a handle that only ever
 *      takes path 1 allocates no scratch raster.  Path, segment count and status are reported with path 1's meaning.
 *      With QB3X_WINK_CF8 path 1 also takes 8-bit rasters of 1, 3 or 4 bands in the common-factor modes (QB3M_CF, QB3M_CF_H;
 *      QB3M_BEST / QB3M_CF_RLE where the RLE0 pass did not win: the header's mode byte says which) whose table, of level 1 or 2,
 *      carries a field per block (what this library's encoder writes for them; an entry has 6 + 3 * bands + 192 bytes): 64 blocks a
 *      segment, any destination address, the same reporting.  The factor in force inside a segment is found among the segment's own
 *      units, before the first of them it is the entry's.  What the kernel cross-checks under a table whose check was sealed again is
 *      what the whole decode from the table cross-checks: positions, block lengths, entering rungs -- not an entry's entering value
 *      or factor, which both take as they are and turn into the same pixels.
 *      With QB3X_WINK_UNIT path 1 also takes the FTL / BASE / BASE_Z rasters that decode a lane per unit or, 32/64-bit data of one
 *      band, a lane per block -- 8-bit rasters of 2 or of 5 to 16 bands, 16-bit rasters of an odd band count above 4, 32/64-bit
 *      rasters of any band count -- from a level-2 table of version 3 with its twelve-bit length per unit, d_index NULL, d_dst on a
 *      multiple of the value size: 64 / bands blocks a segment (64 for one band), as qb3x_window_segments reports; the same
 *      reporting, and no scratch raster on a handle that only ever takes path 1.  A raster so large that one window could need more
 *      waves than a launch holds -- more than 2^24 for blocks per column x (blocks per row / blocks per segment + 2), which takes 16 or
 *      fewer blocks a segment and a side beyond 2^15 pixels -- or of 2^31 blocks and more goes as below.  The common-factor modes of these
 *      shapes are not taken by this bit.
 *      With QB3X_WINK_CFU path 1 takes them: the common-factor streams (QB3M_CF, QB3M_CF_H; QB3M_BEST / QB3M_CF_RLE where the RLE0
 *      pass did not win) of 8-bit rasters of 2 or of 5 to 16 bands, of 16-bit rasters of 2 and more bands, of 32/64-bit rasters of any
 *      band count and of one-band 16-bit rasters, from a table of version 3, level 1 or 2, with its three-byte field per unit (an
 *      entry has 6 + bands * (1 + 2 * value size) + 3 * (64 / bands) * bands bytes), d_index NULL, d_dst on a multiple of the value
 *      size: 64 / bands blocks a segment (64 for one band), the same limits on the raster's size, the same reporting, no scratch
 *      raster on a handle that only ever takes path 1.  Trust is as under QB3X_WINK_CF8: under a table whose check was sealed again
 *      the kernel cross-checks what the whole decode from the table cross-checks -- positions, unit lengths, entering rungs -- not an
 *      entry's entering value or factor, which both take as they are and turn into the same pixels.
 *   2  every other raster with a level-2 table (16-bit, 32/64-bit, other band counts, the common-factor modes): the segments of the
 *      window's block ROWS are decoded into a scratch raster the handle owns, then cropped.  Time follows the window's rows; the
 *      scratch is raster sized (qb3_decoded_size bytes of device memory).
 *   3  everything else -- no table or a level-1 one, an out-of-band d_index, the RLE modes, narrow images, STORED containers: the
 *      whole decode into the scratch raster, then the crop.
 * Any nonzero status word from path 1 or 2 (a table that fails its check, a segment that does not decode, a stream that ends
 * early -- seen in the window's segments, or from the table's last entry lying beyond the stream's end) discards what they
 * wrote and takes path 3: a damaged table costs time, never pixels.  What paths 1 and 2 cannot see is a corrupt unit in a
 * segment they do not decode: the whole decode fails on such a stream, a window beside the damage does not.
 * Errors (QB3E_EINV, 0 returned, nothing written): a handle that is not past qb3_read_info, w == 0, h == 0, a window that is not
 * inside the raster, a nonzero dst_stride below w * bands, d_src not 4-byte aligned.  No byte of d_dst outside the h runs of
 * w * bands values is written: not the gaps of a wide stride, not behind the last row. */
size_t qb3x_decode_window_device(decsp p, const void *d_src, const void *d_index, size_t x0, size_t y0, size_t w, size_t h,
                                 void *d_dst, size_t dst_stride, void *stream);
/* The same for a container in HOST memory (handle from qb3_read_start + qb3_read_info over the whole container); dst is host
 * memory.  STORED containers are cropped on the host without a device; otherwise the whole container goes up the link and only
 * the window comes down. */
size_t qb3x_read_window(decsp p, size_t x0, size_t y0, size_t w, size_t h, void *dst, size_t dst_stride);
/* Pure geometry, needs no device: index segments of the raster that hold a block of the window (pixel x is held by block
 * min(x / 4, blocks per row - 1): the last block column / row is shifted, not padded); *blocks_per_segment (may be NULL) receives
 * the segment size the count is made with.  0: the window is not inside the raster (or is empty).  STORED containers and narrow
 * images (a side below 4) have no block grid: every valid window counts 1, *blocks_per_segment is 0. */
size_t qb3x_window_segments(const decsp p, size_t x0, size_t y0, size_t w, size_t h, size_t *blocks_per_segment);
/* Diagnostics of the handle's last window call: which way it went (0: none yet or it failed, 1: the window kernel, 2: a strip of
 * whole block rows + crop, 3: the whole raster + crop) and how many index segments it decoded (path 1: qb3x_window_segments of the
 * window; 2: those of its block rows; 3: all of the raster's, 0 where there is no block grid). */
int    qb3x_last_window_path(const decsp p);
size_t qb3x_last_window_segments(const decsp p);
/* Rasters beyond path 1's own that take a window kernel, per decoder handle; default 0: every window call goes as described above.
 * Honoured by qb3x_decode_window_device, qb3x_decode_windows_device, qb3x_read_window and qb3x_read_windows, and on a handle of
 * qb3x_open_ranged by qb3x_read_windows_ranged, qb3x_decode_windows_ranged and qb3x_ranged_table_ranges: with QB3X_WINK_U16 these
 * read a 16-bit raster the kernels take in pieces (below), without it whole, and with QB3X_WINK_CF8 an 8-bit common-factor raster
 * the kernels take.  QB3X_WINK_UNIT adds NO ranged shortcut: on a handle of qb3x_open_ranged a raster only that bit's kernels take is
 * still read whole, once, after which its windows go the way of qb3x_decode_windows_device -- with the bit, path 1 from the uploaded
 * container (decoding these rasters from fetched pieces is not built).  QB3X_WINK_CFU adds none either, exactly as QB3X_WINK_UNIT:
 * the container is read whole, once, and its windows then take path 1 from the uploaded copy.  Unknown bits are ignored; a NULL handle: no-op.  The bytes written are the same with and without a bit: the bit
 * only chooses the way.  Harmless on a handle whose raster the kernels of the bits set do not take (other value sizes, other band
 * counts, other modes, a container whose RLE0 pass won, STORED containers, narrow images, a table without block fields, an
 * out-of-band d_index): such a raster goes, and on a ranged handle is read, as it does with the mask at 0.
 * On a handle of qb3x_open_ranged the pieces of a common-factor raster are decoded with nothing but the HOST's check of the table
 * chunks in front of them: as on path 1, an entry's entering value or factor that was changed under a check sealed again is outside
 * "damage costs time, never pixels" -- no kernel and no whole decode from the table can tell it, and all give the same wrong pixels. */
#define QB3X_WINK_U16 1u   /* 16-bit rasters of 1, 2, 3, 4, 6, 8 bands, FTL / BASE, level-2 table: window kernel (path 1) instead of strips (path 2); ranged handles: pieces instead of the whole container */
#define QB3X_WINK_CF8 2u   /* 8-bit rasters of 1, 3, 4 bands in the common-factor modes (QB3M_CF, QB3M_CF_H; QB3M_BEST / QB3M_CF_RLE where the RLE0 pass did not win), table of version 3 with block fields (level 1 or 2): window kernel (path 1) instead of strips (path 2); ranged handles: pieces instead of the whole container */
#define QB3X_WINK_UNIT 4u  /* every other FTL / BASE raster with a level-2 table of version 3 -- 8-bit rasters of 2 or 5 to 16 bands, 16-bit rasters of 5, 7, 9, ... bands, 32/64-bit rasters of 1 to 16 bands: window kernel (path 1) instead of strips (path 2); ranged handles: no shortcut of its own (the container is read whole, once; its windows then take path 1) */
#define QB3X_WINK_CFU 8u   /* the common-factor streams (QB3M_CF, QB3M_CF_H; QB3M_BEST / QB3M_CF_RLE where the RLE0 pass did not win) of those shapes and of one-band 16-bit rasters -- 8-bit rasters of 2 or 5 to 16 bands, 16-bit rasters of 2 and more bands, 16/32/64-bit rasters of one band, 32/64-bit rasters of several -- with a table of version 3 (level 1 or 2) that carries a field per unit: window kernel (path 1) instead of strips (path 2); ranged handles: no shortcut of its own, as QB3X_WINK_UNIT */
void qb3x_set_decoder_window_kernels(decsp p, unsigned mask);

/* A batch of windows: n rectangles of ONE raster in one call -- what a tile server, a viewer or a cropping loader asks of a raster
 * it keeps in device memory.  wins is a HOST array; dst is a device pointer for qb3x_decode_windows_device and a host pointer for
 * qb3x_read_windows; dst_stride is in values, 0 meaning w * bands.  Both return the number of windows written.
 * Bytes: for every i, what qb3x_decode_window_device(p, d_src, d_index, x0, y0, w, h, dst, dst_stride, stream) writes -- the crop
 * of the whole decode, for every container and handle setting -- and no byte outside the window's h runs of w * bands values.
 * Destinations may lie in one buffer (a mosaic, an atlas); they must not overlap, which is the caller's duty and is not checked.
 * Errors are decided before anything is launched or written (QB3E_EINV, 0 returned): a handle that is not past qb3_read_info,
 * wins == NULL, n == 0, n > 2^20, d_src not 4-byte aligned, and ANY window the single call would refuse (empty, not inside the
 * raster, a nonzero stride below w * bands, dst == NULL): one bad window refuses the whole batch.
 * What the batch saves over n single calls:
 *   path 1  ONE kernel launch decodes every window: a descriptor per window goes up in one copy, a wave finds its window by a
 *           search over the windows' wave counts, a status word per window comes back in one copy.  A table chunk is checked once
 *           a call, however many windows read entries from it.
 *   path 2  the windows' ranges of block rows are merged; every merged range is one launch into the scratch raster, a segment is
 *           decoded at most once a call; then one status word, and a crop per window.
 *   path 3  ONE whole decode a call, at most: all windows that end on path 3 share it and are cropped from the scratch raster.
 * A damaged table costs time, never pixels, window by window: on path 1 a window whose segments raise a nonzero status gets the
 * crop of the whole decode, the other windows keep what the kernel wrote.  A table chunk that fails its check, or a table whose
 * last entry lies beyond the stream's end, sends every window to the whole decode; so does a nonzero status on path 2.
 * Afterwards qb3x_window_ok / qb3x_window_path tell how window i went, qb3x_last_window_path is the path of the batch's last
 * window, and qb3x_last_window_segments counts the segments the call's kernels decoded in total: on path 1 a segment two windows
 * share counts twice; where a whole decode ran the raster's count is added once.  With quanta above 1 every window is
 * dequantised as a raster of its own, as in the single call.  The call synchronises `stream` once on the good path, to read the
 * status words. */
typedef struct { size_t x0, y0, w, h; void *dst; size_t dst_stride; } qb3x_window;
size_t qb3x_decode_windows_device(decsp p, const void *d_src, const void *d_index, const qb3x_window *wins, size_t n, void *stream);
/* The same for a container in HOST memory and host destinations: the container goes up ONCE, the windows are decoded into one device
 * buffer and come down one by one.  STORED containers are cropped on the host without a device.  A handle over the container's head
 * only is refused (QB3E_EINV), as by qb3x_read_window. */
size_t qb3x_read_windows(decsp p, const qb3x_window *wins, size_t n);
int    qb3x_window_ok(const decsp p, size_t i);     /* 1: window i of the last batch call was written */
int    qb3x_window_path(const decsp p, size_t i);   /* 0 failed, 1 / 2 / 3 as qb3x_last_window_path */

/* Band-selected windows: the batch calls above with CHOSEN BANDS of every pixel in place of all of them -- three of eight for a false-
 * colour composite, the bands a model was trained on, one band for an index map.  sel is a HOST array of nsel band numbers,
 * 1 <= nsel <= 16, each below the raster's band count; any order, and a band may appear more than once.
 * Bytes: window i receives h rows of w * nsel values; value k of pixel (x, y) is band sel[k] of that pixel as
 * qb3x_decode_windows_device writes it -- the crop of the whole decode with the bands picked, for every container and handle setting
 * (compat flags, quanta, band map, scan order; dequantisation is elementwise, so it commutes with the selection).  dst_stride is in
 * values, 0 meaning w * nsel; no byte outside the h runs of w * nsel values is written.  Returns the number of windows written.
 * qb3x_window_ok, qb3x_window_path, qb3x_last_window_path, qb3x_last_window_segments and qb3x_last_decode_status mean what they mean
 * after qb3x_decode_windows_device; the three paths and "a damaged table costs time, never pixels, window by window" hold unchanged.
 * Errors are decided before anything is launched or written (QB3E_EINV, 0 returned): everything the batch call refuses, with
 * w * nsel in the stride rule, and sel == NULL, nsel == 0, nsel > 16, a band number at or above the raster's band count.
 * The identity selection (nsel == bands, sel[k] == k) IS qb3x_decode_windows_device / qb3x_read_windows: same code, same launches.
 * Two routes give the bytes:
 *   fused   rasters of QB3X_WINK_UNIT / QB3X_WINK_CFU on a handle that set the bit, d_index == NULL, the table the family needs,
 *           every destination on a multiple of the value size and (blocks of a segment) * nsel <= 64 (always so for nsel <= bands):
 *           the family's window kernel writes the selected bands itself -- nothing else runs, and nsel / bands of the bytes are
 *           written (profile names dec_window_unit, dec_window_best_unit);
 *   gather  every other case: the full-band pixels are produced as for qb3x_decode_windows_device, into memory the handle owns (path
 *           1: tight windows written by the family's kernel, sized by the windows; paths 2 and 3: the scratch raster), and ONE launch
 *           per path picks the bands into the destinations, which may lie at any address (profile name win_band_gather).  At most
 *           two such launches a call: one for the windows a shortcut gave, one for those the whole decode gave.  The call then waits
 *           for `stream`.
 * qb3x_last_window_gathers: gather launches of the handle's last band-selected call -- 0 when every window's pixels came straight
 * from a window kernel, and 0 for the identity selection. */
size_t qb3x_decode_windows_bands_device(decsp p, const void *d_src, const void *d_index, const qb3x_window *wins, size_t n,
                                        const uint8_t *sel, size_t nsel, void *stream);
/* The same for a container in HOST memory and host destinations: STORED containers are cropped and selected on the host without a
 * device; else the container goes up ONCE and only the selected bands of the windows come down.  A handle over the container's head
 * only (qb3x_read_start, qb3x_open_ranged) is refused (QB3E_EINV), as by qb3x_read_windows. */
size_t qb3x_read_windows_bands(decsp p, const qb3x_window *wins, size_t n, const uint8_t *sel, size_t nsel);
size_t qb3x_last_window_gathers(const decsp p);

/* Ranged window reads: windows of a container the caller does NOT hold in memory -- a file, an object in a store -- fetching only the
 * bytes that hold the rectangles.  The caller gives a reader: rd(ctx, offset, dst, size) copies `size` container bytes from `offset`
 * to dst (host memory) and returns 0, or nonzero on failure; it is called from the calling thread only, one call at a time, and never
 * for bytes outside [0, container_size).  No counterpart in the reference, whose containers are in host memory (QB3.h:133-141).
 * qb3x_open_ranged: what qb3x_read_start_device does, with rd in place of the device-to-host copies: a handle past qb3_read_info that
 * owns its copy of the container's head and remembers rd / ctx (both must outlive it).  It reads the first bytes chunk head by chunk
 * head, steps over a regular run of "ix" / "zz" chunks arithmetically and reads the "DT" mark behind it: never an entry of the table,
 * never the stream (a table that is not regular is read whole, as qb3x_read_start_device reads it).  NULL: rd failed, or not a container.
 * qb3x_read_windows_ranged (host destinations) and qb3x_decode_windows_ranged (device destinations): bytes, errors, dequantisation,
 * per-window results (qb3x_window_ok, qb3x_window_path, qb3x_last_window_path, qb3x_last_window_segments) are those of
 * qb3x_read_windows / qb3x_decode_windows_device over the whole container: the crop of the whole decode, no byte outside a window's
 * rows, one bad rectangle refuses the batch (QB3E_EINV) before rd is called.  A handle that is not qb3x_open_ranged's: QB3E_EINV.
 * The shortcut is taken where path 1 is -- 8-bit, 1 / 3 / 4 bands, FTL / BASE, a level-2 table of version 3; and, on a handle with
 * qb3x_set_decoder_window_kernels(p, QB3X_WINK_U16), 16-bit data (signed or unsigned) of 1, 2, 3, 4, 6 or 8 bands, FTL / BASE /
 * BASE_Z, a level-2 table of version 3, every device destination on an even address; and, on a handle with QB3X_WINK_CF8, 8-bit
 * data of 1 / 3 / 4 bands in the common-factor modes (QB3M_CF, QB3M_CF_H; QB3M_BEST / QB3M_CF_RLE where the RLE0 pass did not win:
 * the header's mode byte says which), a table of version 3 and level 1 or 2 with a field per block (E = 6 + 3 * bands + 192; its
 * chunk heads say flags 3), any destination address -- and what it reads is fixed by these rules, with B blocks a segment, B as
 * qb3x_window_segments reports (64; 32 for eight 16-bit bands, 21 for six), so that qb3x_ranged_bytes is a number the caller can
 * compute beforehand:
 *   table chunks   With S0 / S1 the first / last index segment that holds a block of window i (qb3x_window_segments' rule), K the
 *                  table's entries and N its entries per chunk: the chunks S0 / N .. min(S1 + 1, K - 1) / N of every window, and
 *                  always the table's last chunk (K - 1) / N; each once.  Chunk c is the container's bytes from T + c * (16 + N * E),
 *                  T the offset of the first "ix" chunk and E the entry size: 12 + n * E + 4 of them (head, its n entries, the pad),
 *                  and 2 more for the last chunk (the "DT" mark).  A chunk is read whole, in one call of rd, unless the handle's
 *                  cache holds it (qb3x_set_ranged_cache: verified chunks, 64 MB by default, the oldest leave first; 0: none).
 *                  Head, pad, mark and the 16-bit check of every chunk read are verified on the host (the formula above), and the
 *                  table's last entry must not lie beyond the stream's end.
 *   pieces         Every block row of every window needs a run of consecutive segments s0 .. s1; with P(s) the 6-byte position of
 *                  entry s (P(K): the stream's length in bits) and D the offset of the first stream byte, the run's bytes are
 *                  [D + P(s0) / 8, D + (P(s1 + 1) + 7) / 8), widened to container offsets that are multiples of 4 and clipped to
 *                  the container's size.  The ranges of all runs of all windows are sorted and merged where they overlap, touch, or
 *                  lie at most `gap` bytes apart (qb3x_set_ranged_gap; 0 by default); every merged range is one call of rd.
 * qb3x_ranged_bytes / qb3x_ranged_reads: the bytes and the calls the handle's last ranged call asked of rd.
 * The pieces go up packed back to back, with the entries their segments use and a sorted piece list, and ONE launch decodes every
 * window from them (profile name dec_window_ranged; dec_window16_ranged for 16-bit rasters, dec_window_best_ranged for 8-bit
 * common-factor ones); the kernel reads no word outside a
 * segment's piece and no byte outside the entries that went up, whatever the entries say.
 * Falling back costs time and bytes, never pixels: a chunk or the table's end failing its check, pieces whose window ends with a
 * nonzero status, a raster the shortcut does not take, a container without a usable table -- the call reads the WHOLE container
 * through rd, once, and goes the way of qb3x_read_windows / qb3x_decode_windows_device for the windows that have no pixels yet.
 * STORED containers need no device and no table: the windows' rows, and only them, are read from their offsets (a call of rd per row
 * of a window; one for a window as wide as the raster).  An rd that returns nonzero fails the call (QB3E_ERR, 0 returned).
 * qb3x_ranged_table_ranges: pure planning, no device and no rd: the chunk ranges above for a batch, sorted, cached or not; returns
 * their count and writes the first `cap` to out (which may be NULL); 0 where the shortcut does not apply or a rectangle is bad. */
typedef int (*qb3x_read_fn)(void *ctx, uint64_t offset, void *dst, size_t size);
typedef struct { uint64_t offset, size; } qb3x_range;
decsp  qb3x_open_ranged(qb3x_read_fn rd, void *ctx, uint64_t container_size, size_t *image_size);
size_t qb3x_read_windows_ranged(decsp p, const qb3x_window *wins, size_t n);
size_t qb3x_decode_windows_ranged(decsp p, const qb3x_window *wins, size_t n, void *stream);
uint64_t qb3x_ranged_bytes(const decsp p);
uint64_t qb3x_ranged_reads(const decsp p);
void   qb3x_set_ranged_gap(decsp p, size_t bytes);
void   qb3x_set_ranged_cache(decsp p, size_t bytes);
size_t qb3x_ranged_table_ranges(const decsp p, const qb3x_window *wins, size_t n, qb3x_range *out, size_t cap);

/* Batched tiles: n images of the encoder's geometry, image i at d_src + i*src_pitch, container i
 * written at d_dst + i*dst_pitch (dst_pitch >= qb3_max_encoded_size, multiple of 4), index i at
 * d_index + i*qb3x_index_size (or NULL).  sizes[i] receives the container size (0 = failed).
 * The band state is reset before every tile (tiles are independent streams).  Returns the number of
 * tiles encoded.  One host synchronisation for the whole batch.  With qb3x_set_encoder_index_chunk on, every tile's
 * container carries its own restart table (at the same offset in all of them). */
size_t qb3x_encode_tiles(encsp p, const void *d_src, size_t n, size_t src_pitch,
                         void *d_dst, size_t dst_pitch, void *d_index, size_t *sizes, void *stream);

/* Batched decode of n containers of the image size and type of handle p (parsed from tile 0);
 * sizes[i] = container size of tile i.  Tiles whose header matches tile 0's go through one set of launches; a tile
 * of another kind -- a raw-stored tile in a batch of coded ones, as qb3x_encode_tiles writes for incompressible
 * data, or the reverse -- is parsed and decoded on its own.  d_index = NULL: the restart tables inside the containers
 * are used when every tile of the batch has one where tile 0 has it, else the streams are walked.  Returns the number
 * of tiles decoded;
 * qb3x_decode_tile_ok(p, i) then tells which (1 = tile i of the last call was decoded). */
size_t qb3x_decode_tiles(decsp p, const void *d_src, size_t n, size_t src_pitch, const size_t *sizes,
                         void *d_dst, size_t dst_pitch, const void *d_index, void *stream);
int qb3x_decode_tile_ok(const decsp p, size_t i);

/* Mosaics: a W x H raster in device memory kept as a grid of independently coded tiles (the calling pattern of GDAL's MRF
 * driver), coded from and decoded to the raster where it lies -- no copy into tile order.  The tile shape is the handle's
 * (xsize x ysize = tw x th; tiles need not be square).  raster_stride is in values, 0 means W * bands; the handle's own
 * qb3_set_*_stride setting is not used by these calls.
 *
 * qb3x_mosaic_tiles is pure geometry (no device): the tiles of the raster, tx = ceil(W / tw) a row, ty = ceil(H / th) rows;
 * *tx, *ty (may be NULL) receive the grid; 0 when W, H, tw or th is 0.
 *
 * qb3x_encode_mosaic: tile k = j * tx + i is the tile at (i * tw, j * th).  Its container goes to d_dst + k * dst_pitch, its
 * index to d_index + k * qb3x_index_size(p) (or d_index is NULL), its size to sizes[k]; returns the number of tiles encoded.
 * Pixel (x, y) of tile k is raster pixel (min(i * tw + x, W - 1), min(j * th + y, H - 1)): tiles that cross the right or
 * bottom edge repeat the raster's last column and row.  The bytes of container k are, for every mode and handle setting,
 * what qb3x_encode_tiles writes for that tile given as a contiguous image -- the raw-stored fallback of an incompressible
 * tile, the restart tables under qb3x_set_encoder_index_chunk and the band state left in the handle (the last tile's)
 * included.  Tiles inside the raster are read in place; the edge tiles (at most tx + ty - 1) are built in memory of the
 * handle's by one launch.  Refused with QB3E_EINV (qb3_get_encoder_state), 0 returned, nothing launched or written:
 * whatever qb3x_encode_tiles refuses, W == 0 or H == 0, a nonzero stride below W * bands, d_raster == NULL.
 *
 * qb3x_decode_mosaic: containers as for qb3x_decode_tiles, tile k at d_src + k * src_pitch, p parsed from tile 0.  Tile k's
 * pixels go to the raster at (i * tw, j * th), clipped to W x H: no byte outside the H runs of W * bands values is written
 * -- not the gaps of a wide stride, nothing behind the last row.  qb3x_decode_tile_ok(p, k) as after qb3x_decode_tiles; a
 * tile that fails leaves its own rectangle unspecified and nothing else.  Tiles of another kind than tile 0, quanta, compat
 * flags, d_index and tables inside the containers: as qb3x_decode_tiles.  Returns the number of tiles decoded; 0 for what
 * qb3x_decode_tiles refuses and for the raster arguments qb3x_encode_mosaic refuses. */
size_t qb3x_mosaic_tiles(size_t W, size_t H, size_t tw, size_t th, size_t *tx, size_t *ty);
size_t qb3x_encode_mosaic(encsp p, const void *d_raster, size_t W, size_t H, size_t raster_stride,
                          void *d_dst, size_t dst_pitch, void *d_index, size_t *sizes, void *stream);
size_t qb3x_decode_mosaic(decsp p, const void *d_src, size_t src_pitch, const size_t *sizes,
                          size_t W, size_t H, void *d_raster, size_t raster_stride,
                          const void *d_index, void *stream);

/* Mosaic windows: rectangles of a mosaic's RASTER -- a viewport, a training crop, a reprojection's footprint -- from the tiles that
 * hold them, in one call, whatever their relation to the tile grid.
 *
 * qb3x_mosaic_window_tiles is pure geometry (no device): the number of tiles of the qb3x_mosaic_tiles grid that hold a pixel of the
 * rectangle [x0, x0 + w) x [y0, y0 + h); *i0 .. *i1 and *j0 .. *j1 (each may be NULL) receive the tile columns and rows, both ends
 * included.  0 when the rectangle is empty or not inside W x H, or when W, H, tw or th is 0.
 *
 * qb3x_decode_mosaic_windows: p, d_src, src_pitch and sizes exactly as qb3x_decode_mosaic takes them (p parsed from tile 0, tile
 * k = j * tx + i at d_src + k * src_pitch).  wins is a HOST array of n rectangles in raster pixels with DEVICE destinations;
 * dst_stride is in values, 0 meaning w * bands.  Returns the number of windows written.
 * Bytes: window i receives the crop [x0, x0 + w) x [y0, y0 + h) of what qb3x_decode_mosaic with the same p, d_src, src_pitch,
 * sizes, W, H (and d_index NULL) writes into a W x H raster -- for every container, tile shape, handle setting (compat flags,
 * quanta, band map, scan order, qb3x_set_decoder_window_kernels) and mix of tile kinds -- and no byte outside the window's h runs
 * of w * bands values.  A window that holds a pixel of a tile that fails to decode is not ok and its content is unspecified; the
 * other windows are unaffected.  Destinations must not overlap (not checked).
 * Errors are decided before anything is launched or written, 0 returned: everything qb3x_decode_mosaic refuses for p, d_src,
 * src_pitch, sizes, W, H; wins == NULL, n == 0, n > 2^20; ANY window that is empty, not inside W x H, has dst == NULL or a nonzero
 * stride below w * bands (one bad window refuses the batch); more than 2^20 pieces in total, a PIECE being the part of one
 * window that lies in one tile (the sum of qb3x_mosaic_window_tiles over the windows).
 * Every piece takes one of two routes:
 *   kernel  tile 0's handle is one path 1 takes without a switch (8-bit, 1 / 3 / 4 bands, FTL / BASE, a level-2 table, quanta 1)
 *           and the piece's tile has tile 0's mode byte, and its "ix" tag and "DT" mark where tile 0 has them: the pieces of ALL
 *           windows go up as one descriptor array and ONE launch decodes them from their containers, straight into the windows
 *           (profile name dec_window_mosaic); one status copy and one synchronisation of `stream`.  The launch itself asks
 *           whether a tile is of tile 0's kind and checks, tile by tile, the table chunks the pieces read entries from, the
 *           table's last chunk and its end against that tile's size: a tile that fails sends all its pieces the other way, a
 *           piece whose own segments raise a status sends that piece alone.  A damaged table costs time, never pixels.
 *   whole   every other piece -- other value sizes, band counts and modes, RLE and raw-stored tiles, narrow tiles, handles
 *           with quanta, tiles unlike tile 0, what failed above: the touched tiles that need it, and no others, are decoded
 *           whole into memory of the handle's as qb3x_decode_tiles decodes them (consecutive tiles in one set of launches), each
 *           at most once a call however many windows touch it, and ONE launch (mosaic_crop) copies the pieces out.
 * Copies to the host and host loops follow the touched tiles, not the mosaic's tile count.
 * Afterwards qb3x_window_ok(p, i) keeps its meaning; qb3x_window_path(p, i) is 1 when every piece of window i came from the
 * window kernel, 3 when at least one came from a whole-tile decode, 0 when it failed; qb3x_last_window_path is the path of the
 * last window; qb3x_last_window_segments counts the index segments the window kernel decoded (the sum of qb3x_window_segments
 * over the pieces that went up, each in its tile); qb3x_last_mosaic_whole_tiles counts the tiles the call decoded whole.
 * qb3x_decode_tile_ok keeps what the last tile or mosaic call left. */
size_t qb3x_mosaic_window_tiles(size_t W, size_t H, size_t tw, size_t th, size_t x0, size_t y0, size_t w, size_t h,
                                size_t *i0, size_t *j0, size_t *i1, size_t *j1);
size_t qb3x_decode_mosaic_windows(decsp p, const void *d_src, size_t src_pitch, const size_t *sizes,
                                  size_t W, size_t H, const qb3x_window *wins, size_t n, void *stream);
size_t qb3x_last_mosaic_whole_tiles(const decsp p);

/* qb3_read_start for the device flavour: `header` is a host copy of the FIRST header_size bytes of a container of
 * stream_size bytes (the parser never reads beyond the copy; qb3_read_info fails when the copy ends before the
 * container's "DT" mark).  qb3x_header_size_bound(first bytes, how many) says how many bytes always suffice,
 * from the container's first 11 bytes (0: not a QB3 container). */
decsp qb3x_read_start(void *header, size_t header_size, size_t stream_size, size_t *image_size);
/* ... and for a container that is in DEVICE memory: qb3_read_start + qb3_read_info in one call; the handle keeps its own
 * copy of the few header bytes it needs (two small device-to-host copies, whatever the size of a restart table: the
 * table's chunk heads and checks are verified on the device before it is used).  Returns a handle ready for
 * qb3x_decode_device / qb3x_decode_tiles, or NULL.  No counterpart in the reference (its containers are in host memory,
 * QB3.h:133-141). */
decsp qb3x_read_start_device(const void *d_container, size_t nbytes, size_t *image_size, void *stream);
size_t qb3x_header_size_bound(const void *container, size_t avail);
/* After qb3_read_info: entries of the restart table found in the container's header chunks that the decoder will use
 * (0: none, or chunks that do not form one table -- the stream is then walked).  No counterpart in the reference. */
size_t qb3x_decoder_table_entries(const decsp p);

/* Self-indexing containers (off by default: the container then differs from the reference's by a few chunks).
 * When on, qb3_encode / qb3x_encode_device put a restart table -- the bit position and band state at the start of every
 * index segment of an FTL/BASE stream (64 blocks of 8-bit grey/RGB/RGBA: 12 bytes, 0.7 % of a typical stream), at about
 * every 64th unit of a common-factor stream (every 32nd for 32/64-bit data; 1.5-6 %) -- into the container in front of "DT", as ignorable (lower-case)
 * chunks: "ix" chunks of at most 64 KB, each followed by a 4-byte pad chunk "zz".
 * An "ix" chunk: 'i' 'x', u16 length of the whole chunk, u8 version (3), u8 flags (bit 0: entries carry common factors),
 * u16 check of the chunk's entries (version 3; reserved and zero in versions 1 and 2, which are still read), u32 blocks per
 * entry, then the entries (flag bit 1: they end with block lengths, see below).  The check: the sum over the n entry bytes
 * b[i] of (b[i] + 1) * (i * 0x9e3779b1 + 1) modulo 2^32, folded to 16 bits (low half XOR high half).  The table sits in a
 * chunk the format does not protect, and the decoder takes positions, rungs, entering values and lengths from it: before
 * using it the decoder verifies every chunk's head and check ON THE DEVICE, and on a mismatch -- or when the decode that
 * relied on the table fails -- decodes the stream WITHOUT the table (the plain walk: what the reference, which skips the
 * chunk, does).  A damaged table costs time, never pixels.  An entry: 6-byte little-endian bit position of its first unit
 * (from the first stream bit), a rung byte per band, the value entering each band (the type's width, little-endian),
 * and with flag bit 0 the common factor entering each band likewise.  The rung byte is the rung the band's first unit is entered
 * with (the one the unit before left; 0 in entry 0), also where the entry's fields say it again.  The entering value is the
 * band-differenced one (the band map's, modulo the type's width) of the pixel the curve visits last in the block before, 0 in
 * entry 0.  The factor is the band-state value the reference keeps (QB3common.h:63-65): the factor of the band's last
 * common-factor unit MINUS 2, 0 before the first such unit -- not the factor itself.  Entry k starts at block k * (blocks per entry);
 * every chunk but the last holds the same number of entries, (65535 - 12) / (bytes an entry) of them, rounded down.  The head's
 * blocks-per-entry word is the raster's blocks per index segment in every table this library writes, also where the decoder
 * derives it from the raster: 64 for 8-bit rasters of 1 / 3 / 4 bands and for one band of any width, in every mode; FTL / BASE
 * streams of 16-bit rasters: 64 for 2, 3 and 4 bands, 21 for six, 32 for eight, 12 for ten, 21 for twelve, 9 for fourteen, 16 for
 * sixteen (64 / lanes a block, a lane owning four bands where the count is a multiple of four, else two); 64 / bands, rounded down,
 * for every other raster -- the common-factor streams of several 16-bit bands among them.  Every field of a block or unit behind the raster's last is
 * zero, and so are the bits of an entry's last byte behind its last field (an odd number of twelve-bit fields): a table is a function
 * of the stream and the raster's shape alone -- not of the level where two levels have the same layout, of the call that wrote it
 * (host, device, tile batch, reindex), of the out-of-band index being asked for, or of what the destination held.
 * tests/qb3_table_spec.py states all of this in numpy and is what the encoder's bytes are compared with.
 * The reference's decoder steps over them
 * (QB3decode.cpp:251-255) and decodes the same pixels: it skips an unknown chunk by its length field counted from the
 * chunk START, so the field holds the whole chunk size, and the pad makes the container parse the same for a reader
 * that adds the 4 head bytes to it.  This library's decoder uses the table when no out-of-band index is given:
 * qb3_read_data / qb3x_decode_device(d_index = NULL) then walk (FTL/BASE) or decode (common-factor modes) the stream
 * from every entry at once, one lane each, instead of serially.  qb3_max_encoded_size() grows by the table's size while the switch is on.  Not written for
 * narrow images and STORED output; a container whose RLE0 pass wins keeps its table in front of "DT" (the entries describe the
 * block stream, which the decoder has again once it has expanded the bytes).  A decoder handle for a container in device memory: qb3x_read_start_device
 * (two small copies whatever the table's size); or, from a host copy of the container up to its "DT" mark,
 * qb3x_read_start (qb3x_header_size_bound() bytes always suffice).  qb3_max_encoded_size() does not depend on the mode:
 * it is the room of the largest table any mode writes for the raster (callers size their buffer before setting the mode).
 * Callers that only know the reference API (LD_PRELOAD, relinked tools) can set QB3X_INDEX_CHUNK=1 (or 2) in the
 * environment: it is read when an encoder handle is created.
 * on = 2 -- entries with BLOCK LENGTHS: for the rasters the 8-bit lane-per-block decoder takes (uint8, 1/3/4 bands, FTL/BASE,
 * Hilbert or Z order) the "ix" chunks' flag bit 1 is set and every entry (one per 64-block segment) ends with the bit
 * lengths of its segment's blocks, ten bits each, little endian: 80 more bytes, 5.5 % of a typical RGB stream instead of
 * 0.7 %.  The decoder then needs neither a walk nor an index -- one kernel, twice the decode rate from the container alone
 * (16384 x 16384 x 3: 0.37 ms instead of 0.65).  16-bit rasters of 2, 3, 4, 6 or 8 bands (FTL/BASE): an entry (one per 64 lanes of
 * the decoder's wave; a lane owns up to four bands of a block) ends with two fields per lane -- four bands: the bit lengths of the
 * band PAIRS (0,1) and (2,3); three: of (0,1) and of band 2; two: of each band; six: three lanes a block of two bands each, a field a band, 21 blocks an entry, both fields of lane 63 zero; eight: two lanes a block of four bands each, their pairs; lanes block-major, a block's lanes in band order -- ten bits each, 160 bytes -- about 5 % of a typical stream (8192 x 8192 x 8: 0.65 ms instead of 0.94); 16-bit rasters of ONE band:
 * a field per block (its unit's length), 80 bytes an entry; 16-bit rasters of an even band count ABOVE eight (10, 12, 14, 16): no
 * length fields, flag bit 1 clear -- their level-2 table is their level-1 table.  32/64-bit rasters
 * (FTL/BASE, where the unit-parallel decoder applies): an entry ends with a twelve-bit length per UNIT of its segment
 * (band-minor, little endian) -- about 10 % of a stream of small units (4096 x 4096 int32: 0.06 ms instead of 0.40).
 * Every OTHER FTL/BASE raster (8-bit data of 2 or more than 4 bands, 16-bit data of an odd band count above 4, 32/64-bit data of
 * several bands: the lane-per-unit decoder, a wave per segment of 64 / bands blocks): the same twelve-bit length per unit.
 * Common-factor streams of one band of 16/32/64-bit data: a three-byte field per block (= unit) at either level: its bits (12)
 * | the rung it is entered with << 12.  8-bit common-factor streams of 1, 3 or 4 bands (round 3): at EITHER level an entry
 * per 64-block segment -- position, rungs, entering values, factors in force -- that ends with a three-byte field per
 * block: the block's bits (12) | the rungs its units are entered with (3 bits a band) << 12, little endian; 6 + 3 * bands +
 * 192 bytes an entry, about 12 % of a typical stream.  It is what the lane-per-block decoder of those streams works from
 * (a common-factor unit leaves its band at the rung of the MULTIPLIED values, so rungs cannot be scanned from the switch
 * codes; the factor in force is found by a ballot of the units that bring their own): 16384 x 16384 x 3 in QB3M_BEST
 * decodes from the container alone in 0.47 ms (round 2: 2.4 ms).  Every other common-factor stream (several bands; round 4):
 * at either level an entry per segment of 64 / bands blocks that ends with a three-byte field per UNIT (band-minor): the
 * unit's bits (12) | the rung it is entered with << 12 -- what the lane-per-unit decoder works from (8192 x 8192 x 8 uint16
 * in QB3M_CF_H from the container alone: 1.0 ms; 2.3 before).  So every common-factor table this library writes carries fields
 * (flags 3) and is the same at level 1 and level 2; entries without fields in a common-factor table (one per about 64 units) are
 * what earlier versions wrote: still read, no longer written.  In the one-band fields the rung takes six bits (bits 12..17), in the
 * per-unit fields likewise; the bits above are zero. */
void qb3x_set_encoder_index_chunk(encsp p, int on);

/* Reindex: a restart table for a container that exists -- a file the reference or GDAL wrote, one of this library's with a table of
 * another version or segment size -- without decoding to pixels and encoding again: no stream bit changes, nothing has to be restated
 * (mode, band map, quanta and scan order stay in the header as they are), and the plain walk is paid once.  No counterpart in the
 * reference, whose stream has no restart points (QB3decode.h:445-454).
 * level 0: no table (the reference's bytes), 1: positions and states, 2: with block / unit lengths where the raster has them
 * (qb3x_set_encoder_index_chunk's values).
 * The output is the source with every "ix" / "zz" chunk removed and, for levels 1 and 2, directly in front of "DT" the table chunks
 * this library's ENCODER writes for the raster at that level: the same segment size, entry layout (version 3, checks sealed) and pads.
 * Every other header byte (CB, QV, SC, the mode, foreign ignorable chunks) stays, in order; every byte behind "DT" is unchanged.  So for
 * the containers C0, C1, C2 the encoder writes for one raster with qb3x_set_encoder_index_chunk 0, 1, 2: reindex(Ca, level b) == Cb, byte
 * for byte.  Where the encoder writes no table -- STORED containers, narrow images (a side below 4) -- the output is the source without
 * its "ix" / "zz" chunks at every level.  A table the source carries is dropped and never trusted, whatever its version, segment size
 * or state.  A container whose RLE0 pass won keeps its coded bytes and gets the table of the expanded block stream, as from the encoder.
 * How: the whole decode of the stream WITHOUT a table into a scratch raster the handle owns (qb3_decoded_size bytes of device memory;
 * the pixels prove the stream sound) leaves a complete index in the handle's workspace; the encoder's own fill code makes the entries
 * of it (profile name reindex_fill), one more launch writes the kept header, the chunks' heads, pads and checks, "DT", and moves the
 * coded bytes (reindex_finish).  The call synchronises `stream` once more than the decode does.
 * qb3x_reindex_size: the size of the new container (what dst_cap must at least be), 0 on error; needs no device.
 * qb3x_reindex_device: p is a handle past qb3_read_info over a HOST copy of the whole container (the header is rebuilt from it);
 * d_src the whole container, 4-byte aligned; d_dst 4-byte aligned, not overlapping d_src.  Returns the new container's size, 0 on error.
 * qb3x_reindex: host buffers; makes and destroys its own handle.  Level 0, STORED and narrow sources need no device; otherwise the
 * container goes up once and the new one comes down.
 * Errors (0 returned, no byte written at or behind d_dst + dst_cap):
 *   QB3E_EINV  a handle that is not past qb3_read_info or holds only a copy of the container's head, a level outside 0..2, dst_cap
 *              below qb3x_reindex_size, pointers that are NULL or not 4-byte aligned;
 *   QB3E_ERR   a stream whose walk ends with an error, or with "the stream ended early" (status bit 2, which a decode forgives as the
 *              reference's reader does): an archive tool must not index a truncated stream -- the table's last entry would lie
 *              beyond its end.  The destination's contents are then unspecified.  (Bit 6, which lane walked the stream, is no error.)
 * qb3x_last_decode_status reports the walk's status word as after a decode. */
size_t qb3x_reindex_size(const decsp p, int level);
size_t qb3x_reindex_device(decsp p, const void *d_src, void *d_dst, size_t dst_cap, int level, void *stream);
size_t qb3x_reindex(const void *src, size_t src_size, void *dst, size_t dst_cap, int level);

/* Compatibility switches. */
#define QB3X_REF_CBAND0 1u      /* decoder: reproduce reference defect (no CB chunk => every band adds band 0,
                                   reference QB3decode.cpp:138 + QB3decode.h:560-567) instead of identity */
void qb3x_set_decoder_compat(decsp p, unsigned flags);

/* Aliases for the names BASELINE.json uses; the reference has no such symbols. */
decsp  qb3_create_decoder(void *source, size_t source_size, size_t *image_size);  /* read_start + read_info */
size_t qb3_decode(decsp p, void *destination);                                     /* read_data */

/* Per-kernel timing for benchmarks: when enabled, every kernel the library launches is bracketed by HIP
 * events on the launch stream; totals are resolved at the library's own synchronisation points.
 * Kernel names: enc_units, enc_scan, enc_concat, enc_seams, enc_best_units, enc_best_scan, enc_best_recode,
 * dec_index_table, dec_index_serial, dec_index_prev, dec_index_scan, dec_units, dec_segments, dec_window (the window kernel of
 * qb3x_decode_window_device, path 1), dec_window16 (the 16-bit window kernels: path 1 under QB3X_WINK_U16), dec_window_best (the window kernels of the 8-bit common-factor modes: path 1 under QB3X_WINK_CF8), dec_window_unit (the window kernels of the lane-per-unit and one-band 32/64-bit rasters: path 1 under QB3X_WINK_UNIT), dec_window_best_unit (those of the common-factor streams of such shapes: path 1 under QB3X_WINK_CFU), dec_window_ranged (the same from fetched pieces: the ranged calls), dec_window16_ranged (... of 16-bit rasters under QB3X_WINK_U16), dec_window_best_ranged (... of 8-bit common-factor rasters under QB3X_WINK_CF8), win_band_gather (the band pick of the band-selected window calls where no window kernel writes the selection itself), reindex_fill, reindex_finish (qb3x_reindex_device: the table's entries; everything else of the
 * new container).
 * level: 0 off, 1 every kernel, 2 all but the microsecond kernels (enc_scan, enc_seams, enc_best_scan), whose two
 * events cost more than they take. */
void qb3x_profile_enable(int level);
void qb3x_profile_reset(void);
int  qb3x_profile_get(const char *kernel, double *total_ms, uint64_t *count);   /* 1 if the kernel was seen */
int  qb3x_profile_names(char *buf, size_t bufsize);                             /* comma separated, returns count */

/* FNV-1a (64 bit) of n host bytes -- the checksum this project's reference anchors are published with (SURVEY.md
 * Appendix C), for callers that verify containers.  seed = 0 starts a hash, a previous result continues it. */
uint64_t qb3x_fnv1a64(const void *data, size_t n, uint64_t seed);

/* The RLE0 byte pass of the *_RLE modes (reference QB3encode.cpp:271-332, QB3decode.cpp:267-307) on DEVICE buffers: the
 * coded (decode = 0) or expanded (decode != 0) form of the n bytes at d_src, bit for bit what the reference's serial
 * loops produce.  d_dst == NULL asks for the size only.  Returns the size; 0 on failure or when it exceeds dst_cap.
 * The library uses it for QB3M_RLE / QB3M_CF_RLE (and the legacy _H modes) so that such streams stay on the device. */
size_t qb3x_rle0_device(const void *d_src, size_t n, void *d_dst, size_t dst_cap, int decode, void *stream);

/* Last HIP error string seen by this thread inside the library ("" if none). */
const char *qb3x_last_error(void);

#if defined(__cplusplus)
}
#endif
#endif
