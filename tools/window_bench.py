"""tools/window_bench.py [CASE] -- time of a window decode (qb3x_decode_window_device) against what a caller had to do without it:
the whole qb3x_decode_device into a buffer of its own, then a strided device copy of the window.  Two rasters: the headline one
(16384 x 16384 x 3 uint8, FTL, level-2 table: the window kernel, path 1) and config 3's (8192 x 8192 x 8 uint16, FTL: a strip of
block rows + crop, path 2); windows of 256^2, 1024^2, 4096^2 and the whole raster at an origin that is not a multiple of 256.
Events on the caller's stream around N calls, both ways alternating in the same run; the window kernel's own time from the
library's profile (dec_window) in a pass of its own.  One JSON line per window.
Without CASE every raster runs in a child process of its own under a time limit, and the first failure ends the run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"headline": (16384, 16384, 3, 0, "NOISY3", 8), "config3": (8192, 8192, 8, 2, "LANDSAT16", 8)}


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


def run(case):
    import torch
    from qb3_amd import synth, device as qdev, TYPESIZE
    w, h, b, dt, gen, mode = CASES[case]
    tsz = TYPESIZE[dt]
    img = synth.generate(w, h, b, dt, gen, 3)
    raw = img.reshape(-1).view(torch.uint8)
    enc = qdev.DeviceEncoder(w, h, b, dt, mode=mode, want_index=False, index_chunk=2)
    dst, n, _ = enc.encode(raw)
    dec = qdev.DeviceDecoder(dst, n)
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
        t_win, t_old = [], []
        for _ in range(3):                              # alternating, three rounds each
            t_win.append(timed(window, reps))
            t_old.append(timed(decode_and_crop, reps))
        qdev.profile_reset()
        qdev.profile_enable(1)
        for _ in range(20):
            window()
        torch.cuda.synchronize()
        qdev.profile_enable(0)
        prof = qdev.profile_report()
        kern = {k: round(v[0] / v[1], 4) for k, v in prof.items() if k in ("dec_window", "dec_units")}
        print(json.dumps({"case": case, "window": [wx, wy, ww, hh], "path": path, "segments": segs, "window_ms": [round(t, 4) for t in t_win],
                          "decode_and_crop_ms": [round(t, 4) for t in t_old], "kernel_ms": kern}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run(sys.argv[1])
    else:
        for case in CASES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), case], timeout=420)
            if r.returncode:
                sys.exit("window_bench: %s ended with status %d; nothing more is run" % (case, r.returncode))
