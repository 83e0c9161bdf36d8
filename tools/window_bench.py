"""tools/window_bench.py [CASE] -- time of a window decode (qb3x_decode_window_device) against what a caller had to do without it:
the whole qb3x_decode_device into a buffer of its own, then a strided device copy of the window.  Two rasters: the headline one
(16384 x 16384 x 3 uint8, FTL, level-2 table: the window kernel, path 1) and config 3's (8192 x 8192 x 8 uint16, FTL: a strip of
block rows + crop, path 2); windows of 256^2, 1024^2, 4096^2 and the whole raster at an origin that is not a multiple of 256.
Events on the caller's stream around N calls, both ways alternating in the same run; the window kernel's own time from the
library's profile (dec_window) in a pass of its own.  One JSON line per window.
--kernels16 sets QB3X_WINK_U16 on the handle (qb3x_set_decoder_window_kernels): 16-bit rasters then take the window kernel too
(path 1, profile name dec_window16); CASE may also be u16x1 (8192 x 8192 x 1 uint16, FTL).
--kernels-cf sets QB3X_WINK_CF8: CASE best (the 16384 x 16384 x 3 QB3M_BEST raster of bench.py's second configuration) then takes the
window kernel of the common-factor modes (path 1, profile name dec_window_best).  The same call with and without the bit alternate
in one run (window_ms against window_off_ms: the strips of path 2), and the profile pass also times the whole decode's kernel
(dec_units) for the whole-raster window to be compared with.
--kernels-unit CASE (u8x5, u16x7, i32x1, i64x2: 8192 x 8192 rasters of uint8 x 5, uint16 x 7, int32 x 1, int64 x 2, FTL, level-2 table; without
CASE each in a child process of its own) times the window kernels of QB3X_WINK_UNIT: the call with the bit (path 1, profile name
dec_window_unit) and the same call with the mask at 0 (path 2: the strips of the window's block rows, then the crop) on the same
handle, alternating in one run, for windows of 256^2, 1024^2 and 4096^2; the kernels' own times from the profile in a pass of its own.
Without CASE every raster runs in a child process of its own under a time limit, and the first failure ends the run; --kernels-cf
then adds CASE best and is passed to it alone (the bit changes nothing for the other two).
best --kernels-cfu [SHAPE] is the best workload for the other common-factor rasters (SHAPE u16x8, u8x5, i32x1, i64x2: 8192 x 8192 rasters
of uint16 x 8 in QB3M_CF_H, uint8 x 5 and int32 x 1 in QB3M_BEST, int64 x 2 in QB3M_CF -- generated rasters quantised to multiples of
a factor; without SHAPE each in a child process of its own): QB3X_WINK_CFU (path 1, profile name dec_window_best_unit) against the
mask at 0 on the same handle, as --kernels-unit measures, for windows of 256^2, 512^2 and 2048^2 and one of 8192 x 512 (whole block rows), and for each
square side a batch of 64 windows at seeded random origins (qb3x_decode_windows_device: batch_ms against batch_off_ms).

tools/window_bench.py --batch [CASE] -- the batch call (qb3x_decode_windows_device) against the same windows through single calls on
the same handle: 64 windows of 256^2 and 64 of 1024^2 of the headline raster at seeded random origins that are not multiples of 256
(path 1: one launch against 64), and 16 windows of 256^2 of a plain 4096 x 4096 x 3 container (path 3: one whole decode against
16).  Same timing: events on the caller's stream, alternating over three rounds in one process, dec_window's time in a pass of its
own.  One JSON line per case.  With --kernels-cf the cases are best256 and best1024 (the QB3M_BEST raster): the batch with the bit
(path 1, one launch) against the batch without it (path 2, merged strips) and against single calls with it, alternating.

tools/window_bench.py --ranged FILE [x0,y0,w,h] -- a window of a file on disk read in pieces (qb3x_open_ranged over os.pread,
qb3x_read_windows_ranged) against qb3x_read_window of the same file read whole: wall-clock milliseconds (the reads are part of the
work) of a cold window (a fresh handle a call), a warm one (the table chunks cached in the handle) and the whole-file way, the best of
a few, with the bytes read beside each.  The window defaults to 512 x 512 in the raster's middle.  One JSON line.
--kernels16 sets QB3X_WINK_U16 on the ranged handles: a 16-bit file is then read in pieces too (without it: whole, every call), and
the line also carries the kernel's own time (dec_window16_ranged, from the library's profile in a pass of its own).
--kernels-cf sets QB3X_WINK_CF8 on them: an 8-bit common-factor file (--write best) is then read in pieces too.  The same calls on
handles without the bit -- the file read whole, every call -- alternate with them in the same process, round by round (cold_off_ms,
warm_off_ms and their bytes and reads beside cold_ms, warm_ms), and the kernel's own time is dec_window_best_ranged's.

tools/window_bench.py [--kernels-unit | --kernels16] CASE --bands LIST -- band-selected windows (qb3x_decode_windows_bands_device, LIST: comma
separated band numbers) against what a caller does without them, for batches of 64 windows of 256^2 and of 1024^2 at seeded origins, in
one process, alternating over three rounds, events on the caller's stream: bands_ms, the band-selected call; full_ms, the full-band
qb3x_decode_windows_device of the same windows on the same handle -- twice a round, so the line carries its own spread (full_spread_ms:
the largest difference between the two of a round); full_pick_ms, that call followed by out[..., LIST].contiguous() in torch.  With
--kernels-unit CASE is u8x5 / u16x7 / i32x1 / i64x2 and the lane-per-unit kernels write the selection themselves (gathers 0); with
--kernels16 config3, or headline, full-band windows go to the handle's memory and one gather launch picks the bands (gathers 1).  The
kernels' own times (the window kernel's and win_band_gather's) come from the library's profile in a pass of its own.

tools/window_bench.py --write CASE FILE -- writes CASE's container (level-2 table) to FILE, for --ranged to read; CASE best is the
container of bench.py's second configuration (16384 x 16384 x 3, QB3M_BEST)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"headline": (16384, 16384, 3, 0, "NOISY3", 8), "config3": (8192, 8192, 8, 2, "LANDSAT16", 8), "u16x1": (8192, 8192, 1, 2, "LANDSAT16", 8),
         "best": (16384, 16384, 3, 0, "NOISY3", 7)}
SEEDS = {"best": 2}         # (bench.py's raster; the others: 3)


def timed(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def run(case, kernels16=False, kernels_cf=False):
    import torch
    from qb3_amd import synth, device as qdev, TYPESIZE, QB3X_WINK_U16, QB3X_WINK_CF8
    w, h, b, dt, gen, mode = CASES[case]
    tsz = TYPESIZE[dt]
    img = synth.generate(w, h, b, dt, gen, SEEDS.get(case, 3))
    raw = img.reshape(-1).view(torch.uint8)
    enc = qdev.DeviceEncoder(w, h, b, dt, mode=mode, want_index=False, index_chunk=2)
    dst, n, _ = enc.encode(raw)
    dec = qdev.DeviceDecoder(dst, n)
    mask = (QB3X_WINK_U16 if kernels16 else 0) | (QB3X_WINK_CF8 if kernels_cf else 0)
    dec.set_window_kernels(mask)
    full = torch.empty(raw.numel(), dtype=torch.uint8, device="cuda")
    rows = full.view(h, w * b * tsz)
    x0, y0 = 1001, 517
    for side in (256, 1024, 4096, 0):
        ww, hh = (side, side) if side else (w, h)
        wx, wy = (x0, y0) if side else (0, 0)
        out = torch.empty(hh * ww * b * tsz, dtype=torch.uint8, device="cuda")
        crop = out.view(hh, ww * b * tsz)

        def window():
            dec.decode_window(dst, wx, wy, ww, hh, out=out)

        def decode_and_crop():
            dec.decode(dst, out=full)
            crop.copy_(rows[wy:wy + hh, wx * b * tsz:(wx + ww) * b * tsz])

        window()
        path, segs = dec.last_window
        assert torch.equal(crop, raw.view(h, -1)[wy:wy + hh, wx * b * tsz:(wx + ww) * b * tsz]), "window bytes"
        reps = 200 if side and side <= 1024 else 30
        t_win, t_off, t_old = [], [], []
        off = {}
        for _ in range(3):                              # alternating, three rounds each
            t_win.append(timed(window, reps))
            if kernels_cf:                              # the same call without the bit
                dec.set_window_kernels(mask & ~QB3X_WINK_CF8)
                t_off.append(timed(window, reps))
                off = {"path_off": dec.last_window[0], "segments_off": dec.last_window[1], "window_off_ms": [round(t, 4) for t in t_off]}
                assert torch.equal(crop, raw.view(h, -1)[wy:wy + hh, wx * b * tsz:(wx + ww) * b * tsz]), "window bytes without the bit"
                dec.set_window_kernels(mask)
            t_old.append(timed(decode_and_crop, reps))
        qdev.profile_reset()
        qdev.profile_enable(1)
        for _ in range(20):
            window()
        for _ in range(5 if kernels_cf else 0):         # dec_units: the whole decode's kernel on the same container in the same run
            dec.decode(dst, out=full)
        torch.cuda.synchronize()
        qdev.profile_enable(0)
        prof = qdev.profile_report()
        kern = {k: round(v[0] / v[1], 4) for k, v in prof.items() if k in ("dec_window", "dec_window16", "dec_window_best", "dec_units")}
        line = {"case": case, "kernels16": kernels16, "kernels_cf": kernels_cf, "window": [wx, wy, ww, hh], "path": path, "segments": segs,
                "window_ms": [round(t, 4) for t in t_win]}
        line.update(off)
        line.update({"decode_and_crop_ms": [round(t, 4) for t in t_old], "kernel_ms": kern})
        print(json.dumps(line), flush=True)


# SHAPE: width, height, bands, type, generator, mode (QB3M_CF_H 5, QB3M_BEST 7, QB3M_CF 1), the factor the values are multiples of
CFU_CASES = {"u16x8": (8192, 8192, 8, 2, "LANDSAT16", 5, 10), "u8x5": (8192, 8192, 5, 0, "NOISY3", 7, 6), "i32x1": (8192, 8192, 1, 5, "DEM", 7, 1000),
             "i64x2": (8192, 8192, 2, 7, "DEM", 1, 2 ** 20 + 1)}
UNIT_CASES = {"u8x5": (8192, 8192, 5, 0, "NOISY3"), "u16x7": (8192, 8192, 7, 2, "LANDSAT16"), "i32x1": (8192, 8192, 1, 5, "DEM"), "i64x2": (8192, 8192, 2, 7, "DEM")}


def run_unit(case, cfu=False):
    """path 1 under QB3X_WINK_UNIT (cfu: QB3X_WINK_CFU, and a batch of 64 windows too) against path 2 with the mask at 0: the same
    handle, the same windows, alternating"""
    import numpy as np
    import torch
    from qb3_amd import synth, device as qdev, TYPESIZE, QB3X_WINK_UNIT, QB3X_WINK_CFU
    w, h, b, dt, gen, mode, factor = CFU_CASES[case] if cfu else UNIT_CASES[case] + (8, 1)
    bit, kname = (QB3X_WINK_CFU, "dec_window_best_unit") if cfu else (QB3X_WINK_UNIT, "dec_window_unit")
    tsz = TYPESIZE[dt]
    img = synth.generate(w, h, b, dt, gen, 3)
    if factor > 1:                                      # multiples of the factor: a common factor in practically every unit
        img = (img.to(torch.int64) % min(2 ** (8 * tsz - 1) // factor, 4096) * factor).to(img.dtype)      # (4096 steps at most: no RLE0 win)
    raw = img.reshape(-1).view(torch.uint8)
    enc = qdev.DeviceEncoder(w, h, b, dt, mode=mode, want_index=False, index_chunk=2)
    dst, n, _ = enc.encode(raw)
    dec = qdev.DeviceDecoder(dst, n)
    # (cfu: the last window is 2048^2 pixels as whole block rows, where the strips of path 2 decode nothing the window does not hold)
    for x0, y0, side, wh in ((1001, 517, 256, 256), (1001, 517, 512, 512), (1001, 517, 2048, 2048), (0, 512, w, 512)) if cfu else \
                            ((1001, 517, 256, 256), (1001, 517, 1024, 1024), (1001, 517, 4096, 4096)):
        out = torch.empty(wh * side * b * tsz, dtype=torch.uint8, device="cuda")
        crop = out.view(wh, side * b * tsz)
        want = raw.view(h, -1)[y0:y0 + wh, x0 * b * tsz:(x0 + side) * b * tsz]

        def window():
            dec.decode_window(dst, x0, y0, side, wh, out=out)

        reps = 200 if side * wh <= 1024 * 1024 else 30
        t, last = {1: [], 0: []}, {}
        for _ in range(3):                              # alternating, three rounds each
            for on in (1, 0):
                dec.set_window_kernels(bit if on else 0)
                out.zero_()
                window()
                assert torch.equal(crop, want), "window bytes"
                last[on] = dec.last_window
                t[on].append(round(timed(window, reps), 4))
        kern = {}
        for on in (1, 0):
            dec.set_window_kernels(bit if on else 0)
            qdev.profile_reset()
            qdev.profile_enable(1)
            for _ in range(20):
                window()
            torch.cuda.synchronize()
            qdev.profile_enable(0)
            kern.update({k: round(v[0] / v[1], 4) for k, v in qdev.profile_report().items() if k in (kname, "dec_units")})
        batch = {}
        if cfu and wh == side:                          # 64 windows of this side at seeded random origins, one call
            rng = np.random.default_rng(side)
            rects = [(int(rng.integers(1, w - side)), int(rng.integers(1, h - side)), side, side) for _ in range(64)]
            outs = [torch.empty(side * side * b * tsz, dtype=torch.uint8, device="cuda") for _ in rects]
            tb = {1: [], 0: []}
            for _ in range(3):
                for on in (1, 0):
                    dec.set_window_kernels(bit if on else 0)
                    dec.decode_windows(dst, rects, out=outs)
                    for (bx, by, _, _), o in zip(rects[:2] + rects[-1:], outs[:2] + outs[-1:]):
                        assert torch.equal(o.view(side, -1), raw.view(h, -1)[by:by + side, bx * b * tsz:(bx + side) * b * tsz]), "batch bytes"
                    tb[on].append(round(timed(lambda: dec.decode_windows(dst, rects, out=outs), 10 if side <= 512 else 3), 4))
            batch = {"batch": 64, "batch_ms": tb[1], "batch_off_ms": tb[0]}
        print(json.dumps({"case": case, "mode": lib_mode(dec), **batch, "raster": [w, h, b], "bytes_per_value": tsz, "container_bytes": n, "window": [x0, y0, side, wh],
                          "path": last[1][0], "segments": last[1][1], "window_ms": t[1],
                          "path_off": last[0][0], "segments_off": last[0][1], "window_off_ms": t[0], "kernel_ms": kern}), flush=True)


def run_bands(case, sel, kunit=False, kernels16=False):
    """the band-selected batch against the full-band batch and against the full-band batch + a torch gather: see the head of the file"""
    import numpy as np
    import torch
    from qb3_amd import synth, device as qdev, TYPESIZE, QB3X_WINK_U16, QB3X_WINK_UNIT
    w, h, b, dt, gen = UNIT_CASES[case] if kunit else CASES[case][:5]
    tsz, nsel = TYPESIZE[dt], len(sel)
    img = synth.generate(w, h, b, dt, gen, 3)
    raw = img.reshape(-1).view(torch.uint8)
    enc = qdev.DeviceEncoder(w, h, b, dt, mode=8, want_index=False, index_chunk=2)
    dst, n, _ = enc.encode(raw)
    dec = qdev.DeviceDecoder(dst, n)
    dec.set_window_kernels((QB3X_WINK_UNIT if kunit else 0) | (QB3X_WINK_U16 if kernels16 else 0))
    kname = "dec_window_unit" if kunit else "dec_window16" if kernels16 else "dec_window"
    tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[tsz]      # (the value's width: torch indexes every signed type)
    px = raw.view(tdt).view(h, w, b)
    for side in (256, 1024):
        rng = np.random.default_rng(64 + side)
        rects = [(int(rng.integers(1, w - side)), int(rng.integers(1, h - side)), side, side) for _ in range(64)]
        nb_full, nb_sel = side * side * b * tsz, side * side * nsel * tsz
        full = torch.empty(64 * nb_full, dtype=torch.uint8, device="cuda")
        part = torch.empty(64 * nb_sel, dtype=torch.uint8, device="cuda")
        outs_full = [full[i * nb_full:(i + 1) * nb_full] for i in range(64)]
        outs_sel = [part[i * nb_sel:(i + 1) * nb_sel] for i in range(64)]
        full_px = full.view(tdt).view(64, side, side, b)
        picked = []

        def bands():
            dec.decode_windows(dst, rects, out=outs_sel, bands=sel)

        def whole():
            dec.decode_windows(dst, rects, out=outs_full)

        def whole_pick():
            dec.decode_windows(dst, rects, out=outs_full)
            picked[:] = [full_px[..., sel].contiguous()]

        bands()
        paths, gathers, segs = sorted(set(dec.last_windows)), dec.last_window_gathers(), dec.last_window[1]
        whole_pick()
        for i in (0, 1, 63):                            # the three ways give the source's pixels
            x0, y0 = rects[i][:2]
            want = px[y0:y0 + side, x0:x0 + side][:, :, sel]
            assert torch.equal(part.view(tdt).view(64, side, side, nsel)[i], want), "band-selected bytes"
            assert torch.equal(picked[0][i], want), "full-band bytes"
        reps = 10 if side <= 256 else 3
        t = {"bands": [], "full": [], "pick": []}
        spread = 0.0
        for _ in range(3):                              # alternating, three rounds; the full-band call twice a round
            a = timed(whole, reps)
            t["bands"].append(round(timed(bands, reps), 4))
            t["pick"].append(round(timed(whole_pick, reps), 4))
            c = timed(whole, reps)
            t["full"] += [round(a, 4), round(c, 4)]
            spread = max(spread, abs(a - c))
        kern = {}
        for fn in (bands, whole):
            qdev.profile_reset()
            qdev.profile_enable(1)
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            qdev.profile_enable(0)
            kern[fn.__name__] = {k: round(v[0] / v[1], 4) for k, v in qdev.profile_report().items() if k in (kname, "win_band_gather")}
        print(json.dumps({"case": case, "bands": sel, "raster": [w, h, b], "bytes_per_value": tsz, "windows": 64, "side": side, "paths": paths, "gathers": gathers,
                          "segments": segs, "bands_ms": t["bands"], "full_ms": t["full"], "full_spread_ms": round(spread, 4), "full_pick_ms": t["pick"],
                          "kernel_ms": kern}), flush=True)


def lib_mode(dec):
    """the container's mode byte (QB3M_BEST: 5 unless its RLE0 pass won)"""
    from qb3_amd import lib
    return lib.qb3_get_mode(dec.p)


BATCH_CASES = {"batch256": (16384, 16384, 3, 2, 64, 256), "batch1024": (16384, 16384, 3, 2, 64, 1024), "batch_path3": (4096, 4096, 3, 0, 16, 256)}
BATCH_CASES_CF = {"best256": (16384, 16384, 3, 2, 64, 256), "best1024": (16384, 16384, 3, 2, 64, 1024)}      # --kernels-cf: QB3M_BEST, bench.py's raster


def run_batch(case, kernels_cf=False):
    import numpy as np
    import torch
    from qb3_amd import synth, device as qdev, QB3X_WINK_CF8
    w, h, b, level, count, side = (BATCH_CASES_CF if kernels_cf else BATCH_CASES)[case]
    img = synth.generate(w, h, b, 0, "NOISY3", 2 if kernels_cf else 3)
    raw = img.reshape(-1).view(torch.uint8)
    enc = qdev.DeviceEncoder(w, h, b, 0, mode=7 if kernels_cf else 8, want_index=False, index_chunk=level)
    dst, n, _ = enc.encode(raw)
    dec = qdev.DeviceDecoder(dst, n)
    dec.set_window_kernels(QB3X_WINK_CF8 if kernels_cf else 0)
    rng = np.random.default_rng(64 + side)
    rects = []
    while len(rects) < count:
        x0, y0 = int(rng.integers(0, w - side + 1)), int(rng.integers(0, h - side + 1))
        if x0 % 256 and y0 % 256:
            rects.append((x0, y0, side, side))
    nb = side * side * b
    buf = torch.empty(count * nb, dtype=torch.uint8, device="cuda")
    outs = [buf[i * nb:(i + 1) * nb] for i in range(count)]

    def batch():
        dec.decode_windows(dst, rects, out=outs)

    def singles():
        for (x0, y0, ww, hh), o in zip(rects, outs):
            dec.decode_window(dst, x0, y0, ww, hh, out=o)

    rows = raw.view(h, -1)
    for fn in (singles, batch):                         # both ways give the crop
        buf.zero_()
        fn()
        for (x0, y0, ww, hh), o in zip(rects, outs):
            assert torch.equal(o.view(hh, ww * b), rows[y0:y0 + hh, x0 * b:(x0 + ww) * b]), "window bytes"
    paths = dec.last_windows
    segs = dec.last_window[1]
    reps = 50 if level else 10
    t_batch, t_off, t_single = [], [], []
    off = {}
    for _ in range(3):                                  # alternating, three rounds each
        t_batch.append(timed(batch, reps))
        if kernels_cf:                                  # the same batch without the bit
            dec.set_window_kernels(0)
            t_off.append(timed(batch, reps))
            off = {"paths_off": sorted(set(dec.last_windows)), "segments_off": dec.last_window[1], "batch_off_ms": [round(t, 4) for t in t_off]}
            dec.set_window_kernels(QB3X_WINK_CF8)
        t_single.append(timed(singles, reps))
    qdev.profile_reset()
    qdev.profile_enable(1)
    for _ in range(20):
        batch()
    torch.cuda.synchronize()
    qdev.profile_enable(0)
    prof = qdev.profile_report()
    kern = {k: round(v[0] / v[1], 4) for k, v in prof.items() if k in ("dec_window", "dec_window_best", "dec_units")}
    launches = {k: v[1] / 20 for k, v in prof.items() if k in ("dec_window", "dec_window_best")}
    line = {"case": case, "windows": count, "side": side, "paths": sorted(set(paths)), "segments": segs, "batch_ms": [round(t, 4) for t in t_batch]}
    line.update(off)
    line.update({"single_calls_ms": [round(t, 4) for t in t_single], "ratio": round(min(t_batch) / min(t_single), 4), "kernel_ms": kern,
                 "launches_per_call": launches})
    print(json.dumps(line), flush=True)


def write_case(case, path):
    import torch
    from qb3_amd import synth, device as qdev
    w, h, b, dt, gen, mode = CASES[case]
    img = synth.generate(w, h, b, dt, gen, SEEDS.get(case, 3))
    enc = qdev.DeviceEncoder(w, h, b, dt, mode=mode, want_index=False, index_chunk=2)
    dst, n, _ = enc.encode(img.reshape(-1).view(torch.uint8))
    dst[:n].cpu().numpy().tofile(path)
    print(json.dumps({"case": case, "file": os.path.basename(path), "file_bytes": n}), flush=True)


def run_ranged(path, rect=None, kernels16=False, kernels_cf=False):
    import time
    import numpy as np
    import qb3_amd
    mask = (qb3_amd.QB3X_WINK_U16 if kernels16 else 0) | (qb3_amd.QB3X_WINK_CF8 if kernels_cf else 0)
    size = os.path.getsize(path)
    with qb3_amd.open_ranged(path) as rd:
        W, H = rd.width, rd.height
    if rect is None:
        w, h = min(512, W), min(512, H)
        rect = ((W - w) // 2, (H - h) // 2, w, h)

    def wall(fn, n=5, other=None):
        """the best of n calls of fn and its last result; other: a second function called after each, timed the same way"""
        best, out, best2, out2 = None, None, None, None
        for _ in range(n):
            t0 = time.perf_counter()
            out = fn()
            t = (time.perf_counter() - t0) * 1e3
            best = t if best is None or t < best else best
            if other:
                t0 = time.perf_counter()
                out2 = other()
                t = (time.perf_counter() - t0) * 1e3
                best2 = t if best2 is None or t < best2 else best2
        return (best, out, best2, out2) if other else (best, out)

    def cold(m=mask):
        with qb3_amd.open_ranged(path, window_kernels=m) as rd:
            return rd.read_windows([rect])[0], rd.last_bytes, rd.last_reads, rd.last_windows[0]

    def whole():
        return qb3_amd.decode_window(np.fromfile(path, np.uint8), *rect)

    whole()                                             # (the device and the library's buffers are up before anything is timed)
    t_whole, want = wall(whole)
    off = {}
    if kernels_cf:                                      # with the bit and without it, round by round
        t_cold, (got, cold_bytes, cold_reads, path1), t_off, (got_off, off_bytes, off_reads, path_off) = wall(cold, other=lambda: cold(mask & ~qb3_amd.QB3X_WINK_CF8))
        assert np.array_equal(got_off, want), "the window without the bit is not the window of the whole file"
        off = {"path_off": path_off, "cold_off_ms": round(t_off, 3), "cold_off_bytes": off_bytes, "cold_off_reads": off_reads}
    else:
        t_cold, (got, cold_bytes, cold_reads, path1) = wall(cold)
    assert np.array_equal(got, want), "the ranged window is not the window of the whole file"
    kern = {}
    with qb3_amd.open_ranged(path, window_kernels=mask) as rd:
        rd.read_windows([rect])
        if kernels_cf:
            with qb3_amd.open_ranged(path, window_kernels=mask & ~qb3_amd.QB3X_WINK_CF8) as rd_off:
                rd_off.read_windows([rect])
                t_warm, got, t_off, got_off = wall(lambda: rd.read_windows([rect])[0], other=lambda: rd_off.read_windows([rect])[0])
                assert np.array_equal(got_off, want)
                off.update({"warm_off_ms": round(t_off, 3), "warm_off_bytes": rd_off.last_bytes, "warm_off_reads": rd_off.last_reads})
        else:
            t_warm, got = wall(lambda: rd.read_windows([rect])[0])
        warm_bytes, warm_reads = rd.last_bytes, rd.last_reads
        if kernels16 or kernels_cf:                     # the kernel's own time, in a pass of its own
            from qb3_amd import device as qdev
            qdev.profile_reset()
            qdev.profile_enable(1)
            for _ in range(20):
                rd.read_windows([rect])
            qdev.profile_enable(0)
            kern = {k: round(v[0] / v[1], 4) for k, v in qdev.profile_report().items() if k in ("dec_window16_ranged", "dec_window_ranged", "dec_window_best_ranged")}
    assert np.array_equal(got, want)
    line = {"file": os.path.basename(path), "file_bytes": size, "raster": [W, H], "window": list(rect), "kernels16": kernels16, "kernels_cf": kernels_cf,
            "path": path1, "cold_ms": round(t_cold, 3), "cold_bytes": cold_bytes, "cold_reads": cold_reads,
            "warm_ms": round(t_warm, 3), "warm_bytes": warm_bytes, "warm_reads": warm_reads}
    line.update(off)
    line.update({"whole_file_ms": round(t_whole, 3), "whole_file_bytes": size, "kernel_ms": kern})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    k16, kcf, kunit, kcfu = "--kernels16" in args, "--kernels-cf" in args, "--kernels-unit" in args, "--kernels-cfu" in args
    args = [a for a in args if a not in ("--kernels16", "--kernels-cf", "--kernels-unit", "--kernels-cfu")]
    sel = None
    if "--bands" in args:
        at = args.index("--bands")
        if at + 1 >= len(args):
            sys.exit("window_bench: --bands takes a comma separated list of band numbers")
        sel = [int(v) for v in args[at + 1].split(",")]
        del args[at:at + 2]
    if sel is not None:
        if len(args) != 1 or args[0] not in (UNIT_CASES if kunit else CASES):
            sys.exit("window_bench: --bands goes with one CASE (%s; with --kernels-unit: %s)" % (", ".join(CASES), ", ".join(UNIT_CASES)))
        run_bands(args[0], sel, kunit, k16)
    elif kcfu:
        if args[:1] != ["best"] or (len(args) > 1 and args[1] not in CFU_CASES):
            sys.exit("window_bench: --kernels-cfu goes with CASE best and, optionally, one of %s" % ", ".join(CFU_CASES))
        if len(args) > 1:
            run_unit(args[1], cfu=True)
        else:
            for shape in CFU_CASES:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "best", "--kernels-cfu", shape], timeout=300)
                if r.returncode:
                    sys.exit("window_bench: %s ended with status %d; nothing more is run" % (shape, r.returncode))
    elif kunit:
        if args and args[0] not in UNIT_CASES:
            sys.exit("window_bench: --kernels-unit takes one of %s" % ", ".join(UNIT_CASES))
        if args:
            run_unit(args[0])
        else:
            for case in UNIT_CASES:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-unit", case], timeout=300)
                if r.returncode:
                    sys.exit("window_bench: %s ended with status %d; nothing more is run" % (case, r.returncode))
    elif args and args[0] == "--ranged":
        if len(args) < 2:
            sys.exit("window_bench: --ranged takes a file (and, optionally, x0,y0,w,h)")
        run_ranged(args[1], tuple(int(v) for v in args[2].split(",")) if len(args) > 2 else None, k16, kcf)
    elif args and args[0] == "--write":
        if len(args) != 3 or args[1] not in CASES:
            sys.exit("window_bench: --write takes a case (%s) and a file" % ", ".join(CASES))
        write_case(args[1], args[2])
    elif args and args[0] == "--batch":
        if len(args) > 1:
            run_batch(args[1], kcf)
        else:
            for case in (BATCH_CASES_CF if kcf else BATCH_CASES):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--batch", case] + (["--kernels-cf"] if kcf else []), timeout=300)
                if r.returncode:
                    sys.exit("window_bench: %s ended with status %d; nothing more is run" % (case, r.returncode))
    elif args:
        run(args[0], k16, kcf)
    else:
        for case in ("headline", "config3") + (("best",) if kcf else ()):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), case] + (["--kernels16"] if k16 else []) + (["--kernels-cf"] if kcf and case == "best" else []),
                               timeout=420)
            if r.returncode:
                sys.exit("window_bench: %s ended with status %d; nothing more is run" % (case, r.returncode))
