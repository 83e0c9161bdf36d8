"""tools/reindex_bench.py [CASE] -- what it costs to give a plain container a restart table without coding it again
(qb3x_reindex_device), against what the table then saves.  Two rasters, as tools/window_bench.py's: the headline one (16384 x 16384
x 3 uint8, FTL) and config 3's (8192 x 8192 x 8 uint16, FTL).  For the plain container the encoder writes (no table: what the
reference's encoder writes too) one JSON line with
  reindex_ms             qb3x_reindex_device at levels 0, 1 and 2 (level 0 moves bytes only; 1 and 2 walk the stream first);
  plain_decode_ms        qb3x_decode_device(d_index = NULL) of the same plain container: the walk reindex has to make as well;
  reindexed_decode_ms    qb3x_decode_device(d_index = NULL) of the containers reindex wrote at levels 1 and 2;
  ratio_level2           reindex at level 2 over the plain decode (the best of the runs of each);
  kernel_ms              reindex_fill and reindex_finish from the library's profile, in a pass of their own;
  finish                 reindex_finish alone against its algorithmic bytes (container in + container out) and the rate a plain
                         device-to-device copy reaches here (bench.py's roofline.device_copy_GBps, measured the same way).
Events on the caller's stream around every call, the calls alternating over the rounds of one process.
Without CASE every raster runs in a child process of its own under a time limit, and the first failure ends the run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"headline": (16384, 16384, 3, 0, "NOISY3", 8), "config3": (8192, 8192, 8, 2, "LANDSAT16", 8)}


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def copy_rate(torch):
    """device-to-device copy of 1 GiB, read + write bytes counted (bench.py, copy_peak)"""
    n = 1 << 30
    a = torch.empty(n, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return round(2 * n * 10 / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)


def run(case, rounds=3):
    import torch
    from qb3_amd import synth, device as qdev, lib
    w, h, b, dt, gen, mode = CASES[case]
    img = synth.generate(w, h, b, dt, gen, 3)
    raw = img.reshape(-1).view(torch.uint8)
    dst, n, _ = qdev.DeviceEncoder(w, h, b, dt, mode=mode, want_index=False, index_chunk=0).encode(raw)
    src = dst[:(n + 3) // 4 * 4].clone()
    host = src[:n].cpu().numpy()
    del dst, img
    dec = qdev.DeviceDecoder(host, n)                   # over the whole container in host memory: what reindex asks for
    pixels = torch.empty(raw.numel(), dtype=torch.uint8, device="cuda")
    outs, sizes = {}, {}
    for level in (0, 1, 2):
        cap = lib.qb3x_reindex_size(dec.p, level)
        outs[level] = torch.empty((cap + 3) // 4 * 4, dtype=torch.uint8, device="cuda")
        _, sizes[level] = dec.reindex(src, level, out=outs[level])
    assert sizes[0] == n and torch.equal(outs[0][:n], src[:n]), "level 0 of a plain container is the container"
    decs = {level: qdev.DeviceDecoder(outs[level], sizes[level]) for level in (1, 2)}
    entries = {level: lib.qb3x_decoder_table_entries(decs[level].p) for level in (1, 2)}
    for level in (1, 2):                                # what reindex wrote decodes to the raster
        decs[level].decode(outs[level], out=pixels)
        assert torch.equal(pixels, raw), "decode of the level %d container" % level
        assert lib.qb3x_last_decode_status(decs[level].p) == 0
    t_re = {0: [], 1: [], 2: []}
    t_plain, t_dec = [], {1: [], 2: []}
    for _ in range(rounds):
        t_plain.append(timed(lambda: dec.decode(src, out=pixels)))
        for level in (0, 1, 2):
            t_re[level].append(timed(lambda: dec.reindex(src, level, out=outs[level])))
        for level in (1, 2):
            t_dec[level].append(timed(lambda: decs[level].decode(outs[level], out=pixels)))
    qdev.profile_reset()
    qdev.profile_enable(1)
    dec.reindex(src, 2, out=outs[2])
    dec.reindex(src, 2, out=outs[2])
    torch.cuda.synchronize()
    qdev.profile_enable(0)
    prof = qdev.profile_report()
    kern = {k: round(v[0] / v[1], 4) for k, v in prof.items() if k in ("reindex_fill", "reindex_finish")}
    rate = copy_rate(torch)
    fin = kern.get("reindex_finish")
    finish = None
    if fin:
        gbps = (n + sizes[2]) / (fin * 1e-3) / 1e9
        finish = {"ms": fin, "bytes": n + sizes[2], "GBps": round(gbps, 1), "device_copy_GBps": rate, "frac_of_device_copy": round(gbps / rate, 3)}
    r3 = lambda v: [round(t, 3) for t in v]
    print(json.dumps({"case": case, "raster": [w, h, b, dt], "container_bytes": n, "reindexed_bytes": {str(k): v for k, v in sizes.items()},
                      "table_entries": {str(k): v for k, v in entries.items()},
                      "reindex_ms": {str(k): r3(v) for k, v in t_re.items()}, "plain_decode_ms": r3(t_plain),
                      "reindexed_decode_ms": {str(k): r3(v) for k, v in t_dec.items()},
                      "ratio_level2": round(min(t_re[2]) / min(t_plain), 4), "kernel_ms": kern, "finish": finish}), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args:
        run(args[0])
    else:
        for case in CASES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), case], timeout=540)
            if r.returncode:
                sys.exit("reindex_bench: %s ended with status %d; nothing more is run" % (case, r.returncode))
