"""tools/mosaic_bench.py [CASE] -- a raster on the device as a grid of 512 x 512 tiles: qb3x_encode_mosaic / qb3x_decode_mosaic (the
tiles coded where they lie) against the way open without them: a device-side rearrangement into tile order (torch reshape / permute /
contiguous, edge tiles padded by repeating the last column and row) in front of qb3x_encode_tiles, and qb3x_decode_tiles followed by
the inverse.  Two rasters of uint8 x 3, FTL: "whole" 16384 x 16384 (no edge tile) and "edges" 16000 x 15000 (a right column and a
bottom row); every tile's container carries its level-2 restart table, so both ways decode from the containers alone.  One JSON line a case with
  mosaic_ms / tiles_ms   wall time of encode and decode, each way: events on the caller's stream around the whole call (the
                         rearrangement included on the tiles side), the ways alternating over the rounds of one process; min and median;
  rearrange_ms           the rearrangement alone, each direction;
  ratio                  mosaic over tiles, of the minima;
  kernel_ms              per kernel, from the library's profile (ms a call), in a pass of its own for each way.
Both ways are checked to write the same containers and to return the raster.  Without CASE every raster runs in a child process of its
own under a time limit, and the first failure ends the run.
--windows N --win WxH[,WxH...] times reads by rectangle instead (run_windows): N seeded random rectangles of each shape through
qb3x_decode_mosaic_windows against the whole decode followed by slices and against a loop of per-tile window calls."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"whole": (16384, 16384), "edges": (16000, 15000)}
T, B = 512, 3


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def run(case, rounds=7):
    import torch
    from qb3_amd import synth, device as qdev
    W, H = CASES[case]
    raster = synth.generate(W, H, B, 0, "NOISY3", 3).reshape(H, W, B)
    mc = qdev.MosaicCoder(W, H, B, 0, tile=(T, T), index_chunk=2)      # self-indexed containers, as bench.py's headline: decode needs nothing else
    tx, ty, n = mc.tx, mc.ty, mc.n
    tb = qdev.TileBatchCoder(T, T, B, 0, n, want_index=False, index_chunk=2)
    edges = (tx * T, ty * T) != (W, H)
    ys = torch.clamp(torch.arange(ty * T, device="cuda"), max=H - 1)
    xs = torch.clamp(torch.arange(tx * T, device="cuda"), max=W - 1)
    tiles = torch.empty((ty, tx, T, T, B), dtype=torch.uint8, device="cuda")
    padded = torch.empty((ty * T, tx * T, B), dtype=torch.uint8, device="cuda") if edges else None
    out_m = torch.empty_like(raster)
    out_t = torch.empty_like(raster)

    def to_tiles():
        src = raster.index_select(0, ys).index_select(1, xs) if edges else raster
        tiles.copy_(src.view(ty, T, tx, T, B).permute(0, 2, 1, 3, 4))

    def from_tiles():
        rows = tiles.permute(0, 2, 1, 3, 4)             # (ty, T, tx, T, B): the padded raster's rows
        if edges:
            padded.view(ty, T, tx, T, B).copy_(rows)
            out_t.copy_(padded[:H, :W])
        else:
            out_t.view(ty, T, tx, T, B).copy_(rows)

    def enc_tiles():
        to_tiles()
        tb.encode(tiles)

    def dec_tiles():
        tb.decode(tiles, use_index=False)
        from_tiles()

    ways = {"mosaic_encode": lambda: mc.encode(raster), "tiles_encode": enc_tiles,
            "mosaic_decode": lambda: mc.decode(out_m), "tiles_decode": dec_tiles,
            "rearrange_to_tiles": to_tiles, "rearrange_from_tiles": from_tiles}
    for k in ("mosaic_encode", "tiles_encode", "mosaic_decode", "tiles_decode"):      # warm-up, and the check that both ways agree
        ways[k]()
    torch.cuda.synchronize()
    assert list(mc.sizes) == list(tb.sizes), "the two ways wrote containers of different sizes"
    for k in (0, tx - 1, n - 1):
        assert torch.equal(mc.container(k), tb.dst[k * tb.pitch:k * tb.pitch + tb.sizes[k]]), "container %d" % k
    assert torch.equal(out_m, raster) and torch.equal(out_t, raster), "a way did not return the raster"
    t = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            t[k].append(timed(fn))
    kern = {}
    for way in ("mosaic", "tiles"):
        qdev.profile_reset()
        qdev.profile_enable(1)
        for _ in range(2):
            ways[way + "_encode"]()
            ways[way + "_decode"]()
        torch.cuda.synchronize()
        qdev.profile_enable(0)
        kern[way] = {k: round(v[0] / 2, 4) for k, v in sorted(qdev.profile_report().items())}      # ms a call of the API (all launches of the name)
    stat = lambda v: {"min": round(min(v), 3), "median": round(statistics.median(v), 3)}
    res = {"case": case, "raster": [W, H, B], "tile": T, "tiles": n, "edge_tiles": (tx + ty - 1) if edges else 0, "rounds": rounds,
           "container_bytes": int(sum(mc.sizes))}
    for what in ("encode", "decode"):
        res["mosaic_%s_ms" % what] = stat(t["mosaic_" + what])
        res["tiles_%s_ms" % what] = stat(t["tiles_" + what])
        res["ratio_%s" % what] = round(min(t["mosaic_" + what]) / min(t["tiles_" + what]), 4)
    res["rearrange_ms"] = {"to_tiles": stat(t["rearrange_to_tiles"]), "from_tiles": stat(t["rearrange_from_tiles"])}
    res["kernel_ms"] = kern
    print(json.dumps(res), flush=True)


def run_windows(case, nwin, shapes, rounds=7):
    """--windows: nwin seeded random rectangles of each shape, read three ways from the containers of `case`:
      mosaic_windows   qb3x_decode_mosaic_windows, one call;
      decode_all       qb3x_decode_mosaic of everything, then the slices copied into the windows;
      per_tile_loop    one qb3x_decode_windows_device call per touched tile, over that tile's pieces; the per-tile handles and the
                       window arrays are made outside the timed region.
    Events around each way, the ways alternating over the rounds of one process; one JSON line a shape."""
    import ctypes as C
    import numpy as np
    import torch
    import qb3_amd
    from qb3_amd import synth, device as qdev
    L = qb3_amd.lib
    W, H = CASES[case]
    raster = synth.generate(W, H, B, 0, "NOISY3", 3).reshape(H, W, B)
    mc = qdev.MosaicCoder(W, H, B, 0, tile=(T, T), index_chunk=2)
    mc.encode(raster)
    out_m = torch.empty_like(raster)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    handles = {}
    for (ww, wh) in shapes:
        rng = np.random.default_rng(nwin * 1000003 + ww * 1009 + wh)
        rects = [(int(rng.integers(0, W - ww + 1)), int(rng.integers(0, H - wh + 1)), ww, wh) for _ in range(nwin)]
        outs = [torch.empty(ww * wh * B, dtype=torch.uint8, device="cuda") for _ in rects]
        per_tile = {}                                       # tile -> [(x, y, w, h in the tile, destination, stride)]
        for (x0, y0, w, h), o in zip(rects, outs):
            for j in range(y0 // T, (y0 + h - 1) // T + 1):
                for i in range(x0 // T, (x0 + w - 1) // T + 1):
                    ax, bx, ay, by = max(x0, i * T), min(x0 + w, (i + 1) * T), max(y0, j * T), min(y0 + h, (j + 1) * T)
                    per_tile.setdefault(j * mc.tx + i, []).append((ax - i * T, ay - j * T, bx - ax, by - ay,
                                                                   o.data_ptr() + ((ay - y0) * w + (ax - x0)) * B, w * B))
        calls = []
        for k, ps in sorted(per_tile.items()):
            if k not in handles:
                dims = (C.c_size_t * 3)()
                handles[k] = L.qb3x_read_start_device(C.c_void_p(mc.dst.data_ptr() + k * mc.pitch), int(mc.sizes[k]), dims, stream)
                assert handles[k], "tile %d does not parse" % k
            arr = qb3_amd.window_array([p[:4] for p in ps], [p[4] for p in ps], [p[5] for p in ps])
            calls.append((handles[k], C.c_void_p(mc.dst.data_ptr() + k * mc.pitch), arr, len(ps)))

        mc.decode_windows(rects[:1], out=outs[:1])         # (parses tile 0: the handle is made outside the timed region, as the loop's are)
        wins = qb3_amd.window_array(rects, [o.data_ptr() for o in outs])
        src0 = C.c_void_p(mc.dst.data_ptr())

        def mosaic_windows():                               # the window array prebuilt too, as the loop's
            if L.qb3x_decode_mosaic_windows(mc.d, src0, mc.pitch, mc.sizes, W, H, wins, nwin, stream) != nwin:
                raise RuntimeError("qb3x_decode_mosaic_windows: " + qb3_amd.last_error())

        def decode_all():
            mc.decode(out_m)
            for (x0, y0, w, h), o in zip(rects, outs):
                o.view(h, w, B).copy_(out_m[y0:y0 + h, x0:x0 + w])

        def per_tile_loop():
            for (p, src, arr, n) in calls:
                if L.qb3x_decode_windows_device(p, src, None, arr, n, stream) != n:
                    raise RuntimeError("qb3x_decode_windows_device: " + qb3_amd.last_error())

        ways = {"mosaic_windows": mosaic_windows, "decode_all": decode_all, "per_tile_loop": per_tile_loop}
        for name, fn in ways.items():                       # warm-up, and the check that every way returns the raster's crops
            for o in outs:
                o.fill_(0xA5)
            fn()
            torch.cuda.synchronize()
            for (x0, y0, w, h), o in zip(rects, outs):
                assert torch.equal(o.view(h, w, B), raster[y0:y0 + h, x0:x0 + w]), "%s: window (%d, %d)" % (name, x0, y0)
        mosaic_windows()
        paths = [L.qb3x_window_path(mc.d, i) for i in range(nwin)]
        whole = L.qb3x_last_mosaic_whole_tiles(mc.d)
        t = {k: [] for k in ways}
        for _ in range(rounds):
            for k, fn in ways.items():
                t[k].append(timed(fn))
        kern = {}
        for name in ("mosaic_windows", "per_tile_loop"):
            qdev.profile_reset()
            qdev.profile_enable(1)
            for _ in range(2):
                ways[name]()
            torch.cuda.synchronize()
            qdev.profile_enable(0)
            kern[name] = {k: [round(v[0] / 2, 4), v[1] // 2] for k, v in sorted(qdev.profile_report().items())}     # [ms, launches] a call of the way
        stat = lambda v: {"min": round(min(v), 3), "median": round(statistics.median(v), 3)}
        res = {"mode": "windows", "case": case, "raster": [W, H, B], "tile": T, "tiles": mc.n, "windows": nwin, "win": [ww, wh],
               "pieces": sum(len(v) for v in per_tile.values()), "touched_tiles": len(per_tile), "rounds": rounds,
               "paths": sorted(set(paths)), "whole_tiles": whole}
        for k in ways:
            res[k + "_ms"] = stat(t[k])
        res["ratio_to_decode_all"] = round(min(t["mosaic_windows"]) / min(t["decode_all"]), 4)
        res["ratio_to_per_tile_loop"] = round(min(t["mosaic_windows"]) / min(t["per_tile_loop"]), 4)
        res["kernel_ms"] = kern
        print(json.dumps(res), flush=True)
    for p in handles.values():
        L.qb3_destroy_decoder(p)
    mc.close()


def window_args(args):
    """--windows N --win WxH[,WxH...] taken out of args: (N, [(W, H)], the rest)"""
    nwin, shapes, rest = 0, [], []
    it = iter(args)
    for a in it:
        if a == "--windows":
            nwin = int(next(it))
        elif a == "--win":
            shapes = [tuple(int(v) for v in s.split("x")) for s in next(it).split(",")]
        else:
            rest.append(a)
    if bool(nwin) != bool(shapes):
        sys.exit("mosaic_bench: --windows N and --win WxH go together")
    return nwin, shapes, rest


if __name__ == "__main__":
    nwin, shapes, args = window_args(sys.argv[1:])
    if args:
        run_windows(args[0], nwin, shapes) if nwin else run(args[0])
    else:
        extra = ["--windows", str(nwin), "--win", ",".join("%dx%d" % s for s in shapes)] if nwin else []
        for case in CASES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), case] + extra, timeout=280)
            if r.returncode:
                sys.exit("mosaic_bench: %s ended with status %d; nothing more is run" % (case, r.returncode))
