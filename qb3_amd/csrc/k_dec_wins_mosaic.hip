// qb3_amd/csrc/k_dec_wins_mosaic.hip -- windows of a MOSAIC in one launch: rectangles of a raster that is kept as a grid of independently
// coded tiles (api_mosaic_windows.cpp), decoded from the tiles that hold them.  The batch kernel's work (k_dec_wins.hip) with one thing
// added: the launch reads many containers.
//   * PIECES  A window is cut along the tile grid on the host; every piece is a window of ONE tile, described in that tile's coordinates
//     with its destination already where the piece lies in its window -- to the wave routine it is a window like any other.  The pieces
//     of all windows are one descriptor array and one launch; a wave finds its piece by the batch's search.
//   * TILES   What differs between the containers of equally shaped tiles written by one encoder is where the stream starts, how long it
//     is and where the table stands: three fields of DecArgs.  They sit in an array in device memory, a record a touched tile; the piece
//     names its record in the spare dword of its descriptor, and the shell (win_mosaic_kernel, qb3_win.h) puts them into a local copy of
//     the launch's arguments.  Geometry, table shape and the bit the stream starts on are tile 0's.
//   * TRUST   Tile by tile what the batch gives its one container: the launch's first workgroups check, for every touched tile, the table
//     chunks its pieces read entries from and its last chunk; the workgroup of the last chunk makes the tail check against that tile's
//     stream length and compares mode byte, "ix" tag and "DT" mark with tile 0's -- a raw-stored tile among coded ones fails there.
//     A failure raises a bit in the TILE's status word, and the host sends all pieces of that tile to the whole-tile decode; a wave's own
//     failures go to its PIECE's word.  What a wave reads is bounded as in the batch: entries inside the table's bytes, stream words
//     below the tile's end, staging inside the wave's LDS -- whatever the table says.
// Only the 8-bit family is instantiated here; another family is its dispatcher and a member of its record.
#include "qb3_win.h"

namespace qb3dev {

static_assert(sizeof(WinTile) == WIN_TILE_BYTES && sizeof(WinTileCheck) == WIN_TILE_CHECK_BYTES, "tile records go up as the host wrote them");

void win_u8_mosaic(const Geometry &g, const DecPlan &plan, const WinMosaicArgs &ma, const WinLaunch &l) {
    win_u8_pick(g, plan, [&](auto f) { win_launch(f, ma, l); });
}

void window_mosaic_plan(const Geometry &g, const WinRect *rects, void *const *dsts, const uint32_t *tiles, size_t n, void *descs, uint64_t *segments) {
    WinDesc *d = (WinDesc *)descs;
    uint64_t waves = 0, segs = 0;
    for (size_t i = 0; i < n; i++) {
        window_desc(g, rects[i], dsts[i], &d[i]);
        d[i].pad_ = tiles[i];
        // a launch ends in front of the piece that would take it beyond WIN_LAUNCH_WAVES; the prefix starts again there (window_batch_plan)
        if (waves && waves + d[i].nwaves > WIN_LAUNCH_WAVES) waves = 0;
        d[i].wave0 = (uint32_t)waves;
        waves += d[i].nwaves;
        segs += window_segments(g, rects[i]);
    }
    if (segments) *segments = segs;
}

int launch_decode_windows_mosaic(const WinKernels &k, const Geometry &g, const DecPlan &plan, uint32_t in_bit0, const void *h_descs, const void *d_descs,
                                 size_t n, const void *d_tiles, size_t ntiles, const void *d_checks, size_t nchecks, uint32_t *d_status, void *stream,
                                 const IxTable &ix, uint32_t ix_off, uint32_t hdr, uint32_t mode_byte) {
    hipStream_t st = (hipStream_t)stream;
    if (!k.mosaic || !k.ok(g, plan, ix) || !n || !ntiles || nchecks > 0xffffffffull || hdr < 2 || ix_off + 2 > hdr) {
        set_error("mosaic window batch: not for this raster", 0);
        return -1;
    }
    WinMosaicArgs ma = {};
    IxTable shape = ix;
    shape.check_heads = true;       // (only tile 0's chunk heads were read on the host)
    window_dec_args(ma.d, g, plan, nullptr, in_bit0, 0, nullptr, shape);
    ma.d.ix = nullptr;
    if (k.more_args) k.more_args(ma.d, plan);
    ma.tiles = (const WinTile *)d_tiles; ma.tstatus = d_status + 1 + n;
    ma.checks = (const WinTileCheck *)d_checks;
    ma.ix_off = ix_off; ma.mode_byte = mode_byte;
    // in front of the first launch's waves: a workgroup for every (tile, chunk) pair of the list
    window_launches(ma, h_descs, d_descs, n, d_status, (uint32_t)nchecks, [&](uint32_t grid, bool head) {
        ma.chk_n = head ? (uint32_t)nchecks : 0;
        ProfScope ps(k.prof_mosaic, st);
        k.mosaic(g, plan, ma, WinLaunch{ grid, k.lds(g, plan), stream });
    });
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace qb3dev
