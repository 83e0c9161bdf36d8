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
own under a time limit, and the first failure ends the run."""
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


if __name__ == "__main__":
    args = sys.argv[1:]
    if args:
        run(args[0])
    else:
        for case in CASES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), case], timeout=280)
            if r.returncode:
                sys.exit("mosaic_bench: %s ended with status %d; nothing more is run" % (case, r.returncode))
