#!/usr/bin/env python3
"""bench.py -- QB3M_FTL encode+decode throughput of the MI355X-native QB3 library.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
    (N > 1: the command above starts its N ranks itself; python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...
     bench.py --gpus N ..., what the driver runs, works as well)

A plain run sets up, warms up, times the K steps (no profiler events inside them) and prints the headline line.  Everything
else described below -- the checks against the reference's anchors and of both decode flavours, the per-kernel table and
roofline, the other table level, the sustained leg, plain containers, the host API, the other configurations and the CPU
baselines -- runs only with --full.  --dump-outputs DIR writes what the last timed step computed (a fixed, seeded sample of the
container and of the decoded raster, float32 .npy files, about 36 MB) so that two builds can be compared output for output.

N = 1 -- BASELINE.json configs[1]: ONE 16384x16384 3-band uint8 raster (NOISY3, seed 2), resident in HBM before the
clock starts.  A step = qb3x_encode_device (the container, self-indexed: the restart table travels INSIDE it as
ignorable chunks -- level 2 by default: an entry per 64-block segment that ends with the bit lengths of its blocks, 5.5 % on top of
the stream, so that the decoder needs no walk; --table-level 1: 0.7 %, with a walk; d_index = NULL, nothing is written beside it) followed by qb3x_decode_device of that container ALONE
(index = NULL): what `value` counts is
decode from the stream, as the reference's contract has it (QB3decode.cpp:455-464).  The same decode with this
library's out-of-band index, and of a plain (reference-made) container with nothing to help, are reported beside it
in `decode`.  The container minus its table chunks is checked against the reference's published size AND FNV-1a64
(SURVEY.md Appendix C).  The line also carries, under `workloads`, short measurements of the other BASELINE
configurations -- 3 (8192^2 x 8 uint16, QB3M_BASE), 4 (4096^2 int32 and int64, FTL and QB3M_BEST), 5 (one rank's 32
tiles of 4096^2 x 3 through qb3x_encode_tiles / qb3x_decode_tiles) -- each with its own roofline entry.

N > 1 -- BASELINE.json configs[4]: every rank codes 32 independent 4096x4096x3 tiles per step (N = 8: the 256 tiles
of the configuration; weak scaling), in batches through qb3x_encode_tiles; the containers of batch k travel to rank 0
(RCCL send/recv over xGMI, one message per peer and batch: the sender packs its containers back to back) while batch k+1 is coded; then every rank decodes its own tiles.
The gather is INSIDE the timed step: `value` = pixels of all ranks / max over ranks of the time until every
container is on rank 0 and every tile is decoded.  `coding_only` is the same loop without the gather.

`roofline` prices the dominant kernel against the HBM rate with the algorithmic bytes of SURVEY.md section 8(d):
bands*sizeof(T)*(1+rho) bytes per pixel (raw once + stream once; the in-container table is overhead, listed under
`extra_bytes`), timed live with HIP events the library records on the launch stream.
`cpu_baseline` times oracle/ (the CPU restatement, a "port") on one host core over a bounded sample.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md (6.29 TB/s measured copy)
ANCHORS = {                 # reference containers, SURVEY.md Appendix C: (size, FNV-1a64)
    "c2": (434747055, "777cb7eb671956c2"),
    "c3": (462603297, "5481f2264a7cae14"),
    "c4_i32_ftl": (16417361, "4f3674340266a2f6"), "c4_i64_ftl": (16429835, "6917fa654ba9f9f9"),
    "c4_i32_best": (16413700, "cd51ae557cfbb14f"), "c4_i64_best": (16426177, "62e44ea20713d272"),
    "c5_tile1000": (27171401, "8e91222e70136a30"), "c5_tile1001": (27171735, "4e40f05b13367ea8"),
}
ENC_KERNELS = ("enc_units", "enc_best_units", "enc_best_scan", "enc_best_recode", "enc_scan", "enc_concat", "enc_seams", "rle0_size", "rle0_write")
DEC_KERNELS = ("dec_index_table", "dec_index_serial", "dec_index_prev", "dec_index_scan", "dec_segments", "dec_units", "rle0_expand_size", "rle0_expand")


def container_check(qb3_amd, np, host, tag):
    """(ok, fnv) of a container against ANCHORS[tag]; the restart-table chunks ("ix" + "zz" pairs in front of "DT"),
    if any, are left out of both."""
    size, want = ANCHORS[tag]
    pos, cut0, cut1 = 11, None, None
    while pos + 4 <= len(host):
        sig, ln = bytes(host[pos:pos + 2]), int(host[pos + 2]) | int(host[pos + 3]) << 8
        if sig == b"DT":
            break
        if sig in (b"ix", b"zz"):
            cut0 = pos if cut0 is None else cut0
            pos += ln
            cut1 = pos
        elif sig in (b"CB", b"QV", b"SC"):
            pos += 4 + ln
        else:
            return False, None
    if cut0 is None:
        h = qb3_amd.fnv(host)
        return len(host) == size and h == want, h
    h = qb3_amd.fnv(host[:cut0], host[cut1:])
    return len(host) - (cut1 - cut0) == size and h == want, h


def table_bytes(host):
    """bytes of the restart-table chunks in a container"""
    pos, n = 11, 0
    while pos + 4 <= len(host):
        sig, ln = bytes(host[pos:pos + 2]), int(host[pos + 2]) | int(host[pos + 3]) << 8
        if sig in (b"ix", b"zz"):
            pos += ln
            n += ln
        elif sig in (b"CB", b"QV", b"SC"):
            pos += 4 + ln
        else:
            break
    return n


class Prof:
    """per-kernel HIP-event times of the library (qb3x_profile_*), as deltas between marks"""

    def __init__(self, qdev):
        self.q = qdev

    def start(self, level=1):
        self.q.profile_reset()
        self.q.profile_enable(level)

    def stop(self):
        self.q.profile_enable(False)
        return {k: (ms / max(c, 1), int(c)) for k, (ms, c) in self.q.profile_report().items()}


def kernel_table(avg, algo_bytes):
    return {k: {"avg_ms": round(ms, 4), "launches": c, "GBps_algorithmic": round(algo_bytes / ms / 1e6, 1) if ms > 0 else None}
            for k, (ms, c) in sorted(avg.items())}


def roofline_of(avg, algo_bytes, names, traffic=None, extra=None):
    cand = {k: v for k, v in avg.items() if k in names}
    if not cand:
        return None
    dom = max(cand, key=lambda k: cand[k][0])
    ms = cand[dom][0]
    ach = algo_bytes / (ms * 1e-3) / 1e9
    r = {"bound": "hbm", "kernel": dom, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
         "traffic": traffic, "algorithmic_bytes_per_launch": int(algo_bytes)}
    if extra:
        r["extra_bytes"] = extra
    return r


def pmc_traffic(kernel, workload=None, from_table=False):
    """HBM bytes per launch (PMC, corrected), the VALU summary and the CSV the bytes are a row of, for a kernel from the
    committed rocprofv3 passes (profiles/collect.sh -> profiles/pmc_traffic.json); the other workloads' records sit under
    their name in `workloads`.  from_table: the launch decoded from the container's own table (the decoders' BL variants are
    kept apart from the ones that take the out-of-band index: profiles/summarise.py, `dec_units_bl`)."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            rec = json.load(f)
        rec = rec.get(workload, {}) if workload else rec
        rec = (rec.get(kernel + "_bl") if from_table and kernel + "_bl" in rec else rec.get(kernel)) or {}
        return rec.get("hbm_bytes_per_launch"), rec.get("valu"), rec.get("source")
    except (OSError, ValueError):
        return None, None, None


def attach_traffic(roofline, algo_bytes, workload=None, from_table=False, scale=1.0):
    """roofline.traffic (+ .valu, .traffic_source) from the committed PMC passes.  A record that says the kernel moves more
    than four times its algorithmic bytes is not believed (a summary gone wrong, not a kernel): traffic stays null and the
    line says why."""
    if roofline is None:
        return
    t, valu, src = pmc_traffic(roofline["kernel"], workload, from_table)
    if t is not None:
        t = int(round(t * scale))
        if t > 4 * algo_bytes:
            roofline["traffic_rejected"] = f"{src}: {t} B per launch is more than 4x the algorithmic {int(algo_bytes)} B"
            t = None
    roofline["traffic"] = t
    roofline["traffic_source"] = src if t is not None else None
    if valu:
        roofline["valu"] = valu


def measure_image(torch, qb3_amd, synth, qdev, dev, tag, w, h, bands, dtype, gen, seed, mode, steps, label, traffic_tag=None):
    """One raster: self-indexed encode, decode from the container alone and with the out-of-band index."""
    import numpy as np
    img = synth.generate(w, h, bands, dtype, gen, seed, device=dev)
    raw = img.reshape(-1).view(torch.uint8)
    raw_bytes = raw.numel()
    enc = qdev.DeviceEncoder(w, h, bands, dtype, mode=mode, index_chunk=2)      # (level 2 where the raster takes it: 8-bit 1/3/4 bands, 16-bit 4/8 bands; else the level 1 table)
    dst, n, index = enc.encode(img)
    host = dst[:n].cpu().numpy()
    ok, fnv = container_check(qb3_amd, np, host, tag) if tag in ANCHORS else (None, None)
    hdr_mode = int(host[10])
    dec = qdev.DeviceDecoder(dst, n)
    out = torch.empty(raw_bytes, dtype=torch.uint8, device=dev)
    for ix in (None, index):
        out.zero_()
        dec.decode(dst, out=out, index=ix)
        if not torch.equal(out, raw):
            sys.exit(f"bench.py: {label}: decode(encode(x)) != x -- refusing to report a number")
    stream_bytes = ANCHORS[tag][0] if tag in ANCHORS else int(n) - table_bytes(host)
    algo = raw_bytes + stream_bytes
    prof = Prof(qdev)
    res = {"workload": label, "stream_bytes": stream_bytes, "ratio": round(stream_bytes / raw_bytes, 4), "container_bytes": int(n),
           "header_mode": hdr_mode, "bit_identical_to_reference": None if ok is None else bool(ok), "fnv1a64": fnv}
    prof.start()
    t0 = time.perf_counter()
    for _ in range(steps):
        enc.encode(img)
    torch.cuda.synchronize()
    enc_wall = (time.perf_counter() - t0) * 1e3 / steps         # (with the library's event records and its one host wait per call)
    e = prof.stop()
    prof.start()
    t0 = time.perf_counter()
    for _ in range(steps):
        dec.decode(dst, out=out, index=None)
    torch.cuda.synchronize()
    dec_wall = (time.perf_counter() - t0) * 1e3 / steps
    d_ix = prof.stop()
    prof.start()
    for _ in range(steps):
        dec.decode(dst, out=out, index=index)
    torch.cuda.synchronize()
    d_oob = prof.stop()
    enc_ms = sum(e[k][0] for k in ENC_KERNELS if k in e)
    ix_ms = sum(d_ix[k][0] for k in DEC_KERNELS if k in d_ix)
    oob_ms = sum(d_oob[k][0] for k in DEC_KERNELS if k in d_oob)
    px = w * h
    res.update({
        "encode_ms_kernels": round(enc_ms, 4), "encode_MPixel_s": round(px / enc_ms / 1e3, 1),
        "encode_ms_wall": round(enc_wall, 4), "decode_from_container_ms_wall": round(dec_wall, 4),
        "decode_from_container_ms_kernels": round(ix_ms, 4), "decode_from_container_MPixel_s": round(px / ix_ms / 1e3, 1),
        "decode_out_of_band_index_ms_kernels": round(oob_ms, 4), "decode_out_of_band_index_MPixel_s": round(px / oob_ms / 1e3, 1),
        "kernels": {"encode": kernel_table(e, algo), "decode_from_container": kernel_table(d_ix, algo), "decode_out_of_band_index": kernel_table(d_oob, algo)},
        "roofline": roofline_of({**e, **d_oob}, algo, ENC_KERNELS + DEC_KERNELS,
                                extra={"restart_table_in_container": int(n) - stream_bytes, "out_of_band_index": enc.index_bytes}),
    })
    attach_traffic(res["roofline"], algo, traffic_tag or tag)      # HBM bytes of the dominant kernel by the PMC passes of this workload (profiles/collect.sh)
    del enc, dec, img, out
    return res


def measure_tiles(torch, qb3_amd, synth, qdev, dev, ntiles, steps, seed0=1000):
    """configs[4], one rank's share: ntiles tiles of 4096^2 x 3 through the batched entry points."""
    w = h = 4096
    imgs = torch.stack([synth.generate(w, h, 3, qb3_amd.QB3_U8, "NOISY3", seed0 + t, device=dev) for t in range(ntiles)])
    tc = qdev.TileBatchCoder(w, h, 3, qb3_amd.QB3_U8, ntiles, device=dev)
    sizes = tc.encode(imgs)
    out = torch.empty_like(imgs)
    checks = {}
    for t, tag in ((0, "c5_tile1000"), (1, "c5_tile1001")):
        if seed0 == 1000 and t < ntiles:
            host = tc.dst[t * tc.pitch:t * tc.pitch + sizes[t]].cpu().numpy()
            checks[tag] = bool(sizes[t] == ANCHORS[tag][0] and qb3_amd.fnv(host) == ANCHORS[tag][1])
    for use_index in (True, False):
        out.zero_()
        tc.decode(out, use_index=use_index)
        if not torch.equal(out, imgs):
            sys.exit("bench.py: tiles: decode(encode(x)) != x -- refusing to report a number")
    raw = ntiles * tc.raw_bytes
    algo = raw + sum(sizes)
    prof = Prof(qdev)
    t_enc = t_dec = t_plain = 0.0
    prof.start()
    torch.cuda.synchronize()
    for _ in range(steps):
        t0 = time.perf_counter()
        tc.encode(imgs)
        t1 = time.perf_counter()
        tc.decode(out, use_index=True)
        t2 = time.perf_counter()
        t_enc += t1 - t0
        t_dec += t2 - t1
    avg = prof.stop()
    t0 = time.perf_counter()
    tc.decode(out, use_index=False)
    t_plain = time.perf_counter() - t0
    # the same tiles as self-indexed containers (every tile carries its restart table): encode, and decode from the containers alone
    tci = qdev.TileBatchCoder(w, h, 3, qb3_amd.QB3_U8, ntiles, device=dev, want_index=False, index_chunk=2)
    sizes_i = tci.encode(imgs)
    out.zero_()
    tci.decode(out, use_index=False)
    if not torch.equal(out, imgs):
        sys.exit("bench.py: self-indexed tiles: decode(encode(x)) != x -- refusing to report a number")
    torch.cuda.synchronize()
    t_enc_i = t_dec_i = 0.0
    for _ in range(steps):
        t0 = time.perf_counter()
        tci.encode(imgs)
        t1 = time.perf_counter()
        tci.decode(out, use_index=False)
        t2 = time.perf_counter()
        t_enc_i += t1 - t0
        t_dec_i += t2 - t1
    table_bytes_all = int(sum(sizes_i) - sum(sizes))
    tci.close()
    px = ntiles * w * h
    res = {"workload": f"{ntiles} tiles of {w}x{h}x3 uint8 NOISY3 (seeds {seed0}..{seed0 + ntiles - 1}) per call, QB3M_FTL, qb3x_encode_tiles + qb3x_decode_tiles",
           "stream_bytes": int(sum(sizes)), "ratio": round(sum(sizes) / raw, 4), "bit_identical_to_reference": checks,
           "encode_ms_wall": round(t_enc / steps * 1e3, 3), "decode_ms_wall": round(t_dec / steps * 1e3, 3),
           "encode_MPixel_s": round(px / (t_enc / steps) / 1e6, 1), "decode_out_of_band_index_MPixel_s": round(px / (t_dec / steps) / 1e6, 1),
           "decode_plain_containers_ms_wall": round(t_plain * 1e3, 2), "decode_plain_containers_MPixel_s": round(px / t_plain / 1e6, 1),
           "self_indexed": {"encode_ms_wall": round(t_enc_i / steps * 1e3, 3), "decode_from_containers_ms_wall": round(t_dec_i / steps * 1e3, 3),
                            "encode_MPixel_s": round(px / (t_enc_i / steps) / 1e6, 1), "decode_from_containers_MPixel_s": round(px / (t_dec_i / steps) / 1e6, 1),
                            "restart_table_bytes": table_bytes_all},
           "kernels": kernel_table(avg, algo), "roofline": roofline_of(avg, algo, ENC_KERNELS + DEC_KERNELS)}
    attach_traffic(res["roofline"], algo, "c5_one_rank")
    return res, tc, imgs, out


def copy_peak(torch, dev):
    """device-to-device copy of 1 GiB: the achievable HBM rate next to the 8 TB/s spec (read + write bytes counted)"""
    n = 1 << 30
    a = torch.empty(n, dtype=torch.uint8, device=dev)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=16384, help="raster edge in pixels at N = 1 (default: BASELINE configs[1])")
    ap.add_argument("--table-level", type=int, default=2, choices=[1, 2],
                    help="restart table inside the container: 1 = an entry per segment (0.7 %% of the stream, the decoder walks the "
                         "segments' unit lengths first), 2 = entries with the blocks' bit lengths (5.5 %%, no walk)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-workloads", action="store_true", help="N = 1: skip the short measurements of configs 3, 4, 5")
    ap.add_argument("--workload", default="c2", choices=["c2", "c2best", "c3", "c3cf", "c4", "c5", "plain", "shapes"],
                    help="N = 1: make this configuration the only one run (for profiling); c2 is the headline")
    ap.add_argument("--tiles-per-rank", type=int, default=32)
    ap.add_argument("--batch-tiles", type=int, default=8)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only to rehearse on one GPU)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: reference checks, kernel table and roofline, the other table level, sustained leg, plain "
                         "containers, host API, the other configurations and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write a seeded sample of what the last step computed as DIR/<name>.npy")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` by itself: start the N ranks as fresh child processes -- BEFORE anything here touches the
        # GPU (no torch import yet) -- through the same launcher the driver uses; rank 0 of the children prints the one JSON
        # line on this process's stdout, a failing child makes the launcher (and this process) exit non-zero.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        sys.exit(f"bench.py --gpus {args.gpus} inside a job of {world} ranks: start it as `python bench.py --gpus N` or under torch.distributed.run with N ranks")
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: the QB3 block codec has no CPU fallback")
    if args.backend != "nccl":
        local_rank %= torch.cuda.device_count()         # rehearsal: ranks may share a GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    import qb3_amd
    from qb3_amd import synth, device as qdev, tiles

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if world > 1:
        line = run_tiles_multi(args, torch, dist, qb3_amd, synth, qdev, tiles, dev, rank, world, fence)
        if rank == 0:
            print(json.dumps(line))
        dist.destroy_process_group()
        return

    if args.workload != "c2":           # profiling aid: one of the other configurations alone
        print(json.dumps(run_other(args.workload, args, torch, qb3_amd, synth, qdev, dev)))
        return

    import numpy as np
    W = H = args.size
    bands, dtype = 3, qb3_amd.QB3_U8
    img = synth.generate(W, H, bands, dtype, "NOISY3", 2, device=dev)
    raw = img.reshape(-1).view(torch.uint8)
    raw_bytes = raw.numel()
    # the step's encoder writes the self-indexed container and nothing beside it (d_index = NULL); with --full a second handle
    # writes the out-of-band index once, for the decode flavour that is reported next to the headline
    enc = qdev.DeviceEncoder(W, H, bands, dtype, mode=qb3_amd.QB3M_FTL, want_index=False, index_chunk=args.table_level)
    out = torch.empty(raw_bytes, dtype=torch.uint8, device=dev)
    dst, n, _ = enc.encode(img)
    if args.full:
        enc_oob = qdev.DeviceEncoder(W, H, bands, dtype, mode=qb3_amd.QB3M_FTL, want_index=True, index_chunk=args.table_level)
        dst_oob, n_oob, index = enc_oob.encode(img)
        if n_oob != n or not torch.equal(dst_oob[:n], dst[:n]):
            sys.exit("bench.py: the container depends on whether an out-of-band index is asked for")
        oob_index_bytes = enc_oob.index_bytes
        index = index.clone()
        del dst_oob, enc_oob
        torch.cuda.empty_cache()
    dec = qdev.DeviceDecoder(dst, n)
    last_n = [n]

    def step():
        last_n[0] = enc.encode(img)[1]                   # container (self-indexed) -> enc.dst
        dec.decode(dst, out=out, index=None)             # decode from the container alone

    if args.full:
        # ---- correctness first: bit identity with the reference (size AND hash), both decode flavours exact
        host = dst[:n].cpu().numpy()
        ident, fnv = (None, None)
        if args.size == 16384:
            ident, fnv = container_check(qb3_amd, np, host, "c2")
            if not ident:
                sys.exit(f"bench.py: container (minus its table chunks) hashes to {fnv}, the reference's to {ANCHORS['c2'][1]} -- not bit-identical")
        stream_bytes = ANCHORS["c2"][0] if args.size == 16384 else n
        for ix in (None, index):
            out.zero_()
            dec.decode(dst, out=out, index=ix)
            if not torch.equal(out, raw):
                sys.exit("bench.py: decode(encode(x)) != x -- refusing to report a number")
    for _ in range(max(1, args.warmup)):
        step()

    # ---- the timed region.  --full: HIP events around the two coding kernels only -- the dominant kernel is one of them (level 3: an
    # event pair costs the stream about 15 us, more than the microsecond kernels take and a tenth of the concatenation; those are timed
    # in two extra, untimed steps afterwards).  A plain run records no events.
    prof = Prof(qdev)
    if args.full:
        prof.start(3)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, torch, dst[:last_n[0]], out)
    if not args.full:
        print(json.dumps(headline(args, W, H, dt, {"table_level": args.table_level, "container_bytes": int(last_n[0])})))
        return
    timed = prof.stop()
    prof.start(1)
    for _ in range(2):
        step()
    fence()
    both = prof.stop()
    avg = dict(both)
    avg.update(timed)
    algo = raw_bytes + stream_bytes
    kernels = kernel_table(avg, algo)
    for k in kernels:
        kernels[k]["in_timed_region"] = k in timed
    enc_ms = sum(avg[k][0] for k in ENC_KERNELS if k in avg)
    dec_ms = sum(avg[k][0] for k in DEC_KERNELS if k in avg)

    # ---- the same decode with the out-of-band index, and a sustained leg of at least a second
    prof.start(1)
    for _ in range(5):
        dec.decode(dst, out=out, index=index)
    torch.cuda.synchronize()
    oob = prof.stop()
    oob_ms = sum(oob[k][0] for k in DEC_KERNELS if k in oob)
    # ---- ... and of the container with the OTHER table level (1: an entry per segment, 0.7 % of the stream, the decoder
    # walks the segments' unit lengths first; 2: entries with their blocks' bit lengths, 5.5 %, no walk)
    other_level = 3 - args.table_level
    enc_o = qdev.DeviceEncoder(W, H, bands, dtype, mode=qb3_amd.QB3M_FTL, want_index=False, index_chunk=other_level)
    dst_o, n_o, _ = enc_o.encode(img)
    dec_o = qdev.DeviceDecoder(dst_o, n_o)
    out.zero_()
    dec_o.decode(dst_o, out=out, index=None)
    if not torch.equal(out, raw):
        sys.exit("bench.py: decode(encode(x)) != x with the other table level -- refusing to report a number")
    prof.start(1)
    for _ in range(5):
        enc_o.encode(img)
        dec_o.decode(dst_o, out=out, index=None)
    torch.cuda.synchronize()
    oth = prof.stop()
    other = {"table_level": other_level, "container_bytes": int(n_o), "table_bytes": int(n_o) - (int(n) - table_bytes(host)),
             "encode_ms_kernels": round(sum(oth[k][0] for k in ENC_KERNELS if k in oth), 4),
             "decode_from_container_ms_kernels": round(sum(oth[k][0] for k in DEC_KERNELS if k in oth), 4)}
    del enc_o, dec_o, dst_o
    torch.cuda.empty_cache()
    fence()
    s0 = time.perf_counter()
    sustained_steps = 0
    while time.perf_counter() - s0 < 1.2:
        for _ in range(50):
            step()
        torch.cuda.synchronize()
        sustained_steps += 50
    sustained = time.perf_counter() - s0

    # what a container seen for the first time costs: a handle made from the bytes in device memory (qb3x_read_start_device: a
    # 64-byte fetch, the chunk heads), the decode from the container alone, the handle destroyed -- the timed step reuses one handle
    fresh = None
    if not args.no_workloads:
        f0 = time.perf_counter()
        for _ in range(10):
            fdec = qdev.DeviceDecoder(dst, n)
            fdec.decode(dst, out=out, index=None)
            fdec.close()
        torch.cuda.synchronize()
        fresh = {"ms_wall": round((time.perf_counter() - f0) * 100, 3), "what": "qb3x_read_start_device + qb3_read_info + qb3x_decode_device (index = NULL) + qb3_destroy_decoder per container"}

    # ---- plain containers (what the reference writes: no table inside, no index beside them): the stream is walked
    # serially (a table of unit lengths by bit position, built by the whole chip, then one look-up per unit on one lane)
    plain = None
    if not args.no_workloads:
        def plain_decode(pimg, pw, pb=3, pdt_=None, pmode=None):
            penc = qdev.DeviceEncoder(pw, pw, pb, dtype if pdt_ is None else pdt_, mode=qb3_amd.QB3M_FTL if pmode is None else pmode)
            pdst, pn, _ = penc.encode(pimg)
            pdec = qdev.DeviceDecoder(pdst, pn)
            pout = torch.empty(pimg.numel() * pimg.element_size(), dtype=torch.uint8, device=dev)
            pdec.decode(pdst, out=pout, index=None)          # (first call: allocates the table)
            torch.cuda.synchronize()
            p0 = time.perf_counter()
            pdec.decode(pdst, out=pout, index=None)
            torch.cuda.synchronize()
            pdt = time.perf_counter() - p0
            res = {"ms_wall": round(pdt * 1e3, 2), "MPixel_s": round(pw * pw / pdt / 1e6, 1), "exact": bool(torch.equal(pout, pimg.reshape(-1).view(torch.uint8)))}
            if pb == 1:         # ... and through the reference's own entry point on host buffers (qb3_read_data: upload and download included)
                import ctypes as C
                L = qb3_amd.lib
                hsrc = pdst[:int(pn)].cpu().numpy().copy()
                hout = np.zeros(pout.numel(), dtype=np.uint8)
                dims = (C.c_size_t * 3)()
                hp = L.qb3_read_start(hsrc.ctypes.data, hsrc.size, dims)
                if hp and L.qb3_read_info(hp):
                    L.qb3_read_data(hp, hout.ctypes.data)       # (first call: device buffers, the table)
                    h0 = time.perf_counter()
                    got = L.qb3_read_data(hp, hout.ctypes.data)
                    hdt = time.perf_counter() - h0
                    res["qb3_read_data_ms_wall"] = round(hdt * 1e3, 2)
                    res["qb3_read_data_MPixel_s"] = round(pw * pw / hdt / 1e6, 1)
                    res["qb3_read_data_exact"] = bool(got == hout.size and np.array_equal(hout, pimg.reshape(-1).view(torch.uint8).cpu().numpy()))
                if hp:
                    L.qb3_destroy_decoder(hp)
            return res
        pimg = synth.generate(4096, 4096, 3, dtype, "NOISY3", 1000, device=dev)
        plain = {"workload": "4096x4096x3 uint8 NOISY3 seed 1000, plain container, index = NULL"}
        plain.update(plain_decode(pimg, 4096))
        plain["uint8x3_best"] = {"workload": "the same raster in QB3M_BEST (common factor + index coding), plain container, index = NULL"}
        plain["uint8x3_best"].update(plain_decode(pimg, 4096, 3, None, qb3_amd.QB3M_BEST))
        del pimg
        if args.size == 16384:
            plain["config2"] = {"workload": "the 16384x16384x3 raster of the headline, plain container, index = NULL"}
            plain["config2"].update(plain_decode(img, 16384))
        # one band (elevation rasters; config 4's): the walk by exits of super-windows (k_dec_walk.hip), also for common-factor streams
        for ptag, pdt_, pgen, pmode, pname in (("int32_ftl", qb3_amd.QB3_I32, "DEM", qb3_amd.QB3M_FTL, "int32 DEM seed 4, QB3M_FTL"),
                                               ("int32_best", qb3_amd.QB3_I32, "DEM", qb3_amd.QB3M_BEST, "int32 DEM seed 4, QB3M_BEST"),
                                               ("int64_ftl", qb3_amd.QB3_I64, "DEM", qb3_amd.QB3M_FTL, "int64 DEM seed 4, QB3M_FTL"),
                                               ("int16_base", qb3_amd.QB3_I16, "DEM", qb3_amd.QB3M_BASE, "int16 DEM seed 4, QB3M_BASE"),
                                               ("int16_best", qb3_amd.QB3_I16, "DEM", qb3_amd.QB3M_BEST, "int16 DEM seed 4, QB3M_BEST"),
                                               ("uint8_grey", qb3_amd.QB3_U8, "NOISY3", qb3_amd.QB3M_FTL, "uint8 NOISY3 seed 4, QB3M_FTL")):
            pimg = synth.generate(4096, 4096, 1, pdt_, pgen, 4, device=dev)
            plain[ptag] = {"workload": f"4096x4096x1 {pname}, plain container, index = NULL"}
            plain[ptag].update(plain_decode(pimg, 4096, 1, pdt_, pmode))
            del pimg
        # several bands beyond 8-bit RGB: the chained table walks (k_dec_walk_chain.hip) -- common-factor streams of 8- and 16-bit data too, the
        # walking lane parsing their signal units (round 4); 32/64-bit common-factor streams of several bands: one wave walking unit lengths
        for ptag, pw, pb, pdt_, pgen, pmode, pname in (("uint8x4_ftl", 2048, 4, qb3_amd.QB3_U8, "NOISY3", qb3_amd.QB3M_FTL, "x4 uint8 NOISY3, QB3M_FTL"),
                                                       ("uint8x4_best", 2048, 4, qb3_amd.QB3_U8, "NOISY3", qb3_amd.QB3M_BEST, "x4 uint8 NOISY3, QB3M_BEST"),
                                                       ("uint16x8_base", 2048, 8, qb3_amd.QB3_U16, "LANDSAT16", qb3_amd.QB3M_BASE, "x8 uint16 LANDSAT16, QB3M_BASE"),
                                                       ("uint16x8_best", 1024, 8, qb3_amd.QB3_U16, "LANDSAT16", qb3_amd.QB3M_BEST, "x8 uint16 LANDSAT16, QB3M_BEST"),
                                                       ("uint8x2_ftl", 2048, 2, qb3_amd.QB3_U8, "NOISY3", qb3_amd.QB3M_FTL, "x2 uint8 NOISY3, QB3M_FTL"),
                                                       ("uint16x2_base", 4096, 2, qb3_amd.QB3_U16, "LANDSAT16", qb3_amd.QB3M_BASE, "x2 uint16 LANDSAT16, QB3M_BASE"),
                                                       ("uint8x5_best", 2048, 5, qb3_amd.QB3_U8, "NOISY3", qb3_amd.QB3M_CF_H, "x5 uint8 NOISY3, QB3M_CF_H"),
                                                       ("uint16x7_base", 2048, 7, qb3_amd.QB3_U16, "LANDSAT16", qb3_amd.QB3M_BASE, "x7 uint16 LANDSAT16, QB3M_BASE"),
                                                       ("uint16x3_best", 2048, 3, qb3_amd.QB3_U16, "LANDSAT16", qb3_amd.QB3M_CF_H, "x3 uint16 LANDSAT16, QB3M_CF_H"),
                                                       ("int32x2_base", 2048, 2, qb3_amd.QB3_I32, "DEM", qb3_amd.QB3M_BASE, "x2 int32 DEM, QB3M_BASE")):
            pimg = synth.generate(pw, pw, pb, pdt_, pgen, 4, device=dev)
            plain[ptag] = {"workload": f"{pw}x{pw}{pname} seed 4, plain container, index = NULL"}
            plain[ptag].update(plain_decode(pimg, pw, pb, pdt_, pmode))
            del pimg
        torch.cuda.empty_cache()

    roofline = roofline_of(avg, algo, ENC_KERNELS + DEC_KERNELS, extra={"restart_table_in_container": int(n) - stream_bytes})
    if roofline is not None:
        if args.size == 16384:      # (the PMC passes are of this raster; the step decodes from the container's table: level 2 = the BL variant)
            attach_traffic(roofline, algo, None, from_table=args.table_level == 2)
        roofline["device_copy_GBps"] = copy_peak(torch, dev)
        if roofline.get("traffic"):
            # what the kernel actually moves (PMC: more than the algorithmic bytes -- slots, index) against what a plain copy reaches here
            dom_ms = avg[roofline["kernel"]][0]
            roofline["traffic_GBps"] = round(roofline["traffic"] / (dom_ms * 1e-3) / 1e9, 1)
            roofline["traffic_frac_of_device_copy"] = round(roofline["traffic_GBps"] / roofline["device_copy_GBps"], 3)

    # the reference's own entry points on host buffers (qb3_encode / qb3_read_data: upload or download included) -- reported
    # beside the line, never part of `value`
    host_api = None
    if not args.no_workloads:
        host_api = host_api_times(qb3_amd, img, W, H, args.table_level)
    workloads = None
    if not args.no_workloads and args.size == 16384:
        del img, out, enc, dec, dst
        torch.cuda.empty_cache()
        workloads = {}
        for wl in ("c2best", "c3", "c3cf", "c4", "c5", "shapes"):
            workloads.update(run_other(wl, args, torch, qb3_amd, synth, qdev, dev))

    cpu = None if args.no_cpu_baseline else cpu_baseline()
    line = headline(args, W, H, dt, {"table_level": args.table_level, "table_bytes": table_bytes(host),
                                     "stream_bytes": stream_bytes, "ratio": round(stream_bytes / raw_bytes, 4), "container_bytes": int(n),
                                     "bit_identical_to_reference": ident, "fnv1a64_without_table_chunks": fnv})
    line.update({
        "encode_MPixel_s_kernels": round(W * H / enc_ms / 1e3, 1) if enc_ms else None,
        "decode_MPixel_s_kernels": round(W * H / dec_ms / 1e3, 1) if dec_ms else None,
        "decode": {"from_container_ms_kernels": round(dec_ms, 4), "out_of_band_index_ms_kernels": round(oob_ms, 4),
                   "out_of_band_index_MPixel_s_kernels": round(W * H / oob_ms / 1e3, 1) if oob_ms else None,
                   "out_of_band_index_bytes": oob_index_bytes if workloads is None else None, "other_table_level": other,
                   "fresh_handle_per_container": fresh, "plain_container": plain},
        "sustained": {"seconds": round(sustained, 2), "steps": sustained_steps, "MPixel_s": round(sustained_steps * W * H / sustained / 1e6, 1)},
        "kernels": kernels,
        "roofline": roofline,
        "cpu_baseline": cpu,
        "host_api_ms": host_api,
        "workloads": workloads,
    })
    print(json.dumps(line))


def headline(args, W, H, dt, config):
    """the fields of the N = 1 line that a plain run and --full share; dt: seconds of the args.steps timed steps"""
    return {
        "metric": "MPixel/s encode+decode (QB3M_FTL, 8-bit 3-band)",
        "value": round(W * H / (dt / args.steps) / 1e6, 1),
        "unit": "MPixel/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u8", "data": "synthetic",
        "config": {"workload": f"{W}x{H}x3 uint8 NOISY3 seed 2; QB3M_FTL qb3x_encode_device (self-indexed container, table level {args.table_level}) + "
                               "qb3x_decode_device of that container alone (index = NULL, restart table inside the container)", **config},
        "value_uses": "decode_from_container",
    }


DUMP_SAMPLE = 1 << 22       # bytes of each large output written by --dump-outputs (as float32: 16 MB a file)
DUMP_HEAD = 1 << 20         # leading container bytes written whole (header and restart-table chunks)


def dump_outputs(path, torch, container, decoded, sizes=None, seed=20261016):
    """--dump-outputs: what a caller of the timed step receives -- the container sizes (float64; sizes: of the containers
    that lie back to back in `container`, default one), the first DUMP_HEAD container bytes, and the bytes of the container(s)
    and of the decoded raster(s) at DUMP_SAMPLE positions drawn from a fixed seed (sorted; the positions depend only on the seed
    and the length sampled), float32"""
    import numpy as np
    os.makedirs(path, exist_ok=True)

    def sample(t, salt):
        n = t.numel()
        if n <= DUMP_SAMPLE:
            return t.float().cpu().numpy()
        pos = np.sort(np.random.default_rng([seed, salt]).integers(0, n, DUMP_SAMPLE, dtype=np.int64))
        return t[torch.from_numpy(pos).to(t.device)].float().cpu().numpy()

    files = {"container_sizes": np.array(sizes or [container.numel()], dtype=np.float64),
             "container_head": container[:DUMP_HEAD].float().cpu().numpy(),
             "container_sample": sample(container, 1),
             "decoded_sample": sample(decoded, 2)}
    for name, a in files.items():
        np.save(os.path.join(path, name + ".npy"), a)


def host_api_times(qb3_amd, img, W, H, table_level):
    """qb3_encode / qb3_read_data of the headline raster through HOST pointers (the literal drop-in calls): best of three,
    the host link included (upload, coding and download of different strips at once: qb3_api.cpp, encode_pipelined /
    decode_pipelined) -- not part of `value`"""
    import numpy as np
    L = qb3_amd.lib
    host = np.ascontiguousarray(img.cpu().numpy()).reshape(H, W, 3)
    out = {}
    for name, level in (("plain_container", 0), ("self_indexed_container", table_level)):
        p = L.qb3_create_encoder(W, H, 3, qb3_amd.QB3_U8)
        L.qb3_set_encoder_mode(p, qb3_amd.QB3M_FTL)
        if level:
            L.qb3x_set_encoder_index_chunk(p, level)
        dst = np.empty(L.qb3_max_encoded_size(p), dtype=np.uint8)
        t_enc = []
        for _ in range(3):
            L.qb3_reset_encoder(p)
            L.qb3_set_encoder_mode(p, qb3_amd.QB3M_FTL)
            t0 = time.perf_counter()
            n = L.qb3_encode(p, host.ctypes.data, dst.ctypes.data)
            t_enc.append(time.perf_counter() - t0)
        L.qb3_destroy_encoder(p)
        rec = {"qb3_encode_ms": round(min(t_enc) * 1e3, 2), "container_bytes": int(n)}
        if level:           # (a plain container of this size takes the serial walk: seconds, reported under decode.plain_container)
            back = np.empty(W * H * 3, dtype=np.uint8)
            t_dec = []
            for _ in range(3):
                dims = (qb3_amd._sz * 3)()
                d = L.qb3_read_start(dst.ctypes.data, n, dims)
                ok = d and L.qb3_read_info(d)
                t0 = time.perf_counter()
                m = L.qb3_read_data(d, back.ctypes.data) if ok else 0
                t_dec.append(time.perf_counter() - t0)
                L.qb3_destroy_decoder(d)
            rec["qb3_read_data_ms"] = round(min(t_dec) * 1e3, 2)
            rec["exact"] = bool(m == back.size and np.array_equal(back, host.ravel()))
        out[name] = rec
    return out


def run_other(wl, args, torch, qb3_amd, synth, qdev, dev):
    """configs 3, 4 and 5 on one GPU, a few steps each"""
    steps = max(3, min(args.steps, 5))
    out = {}
    if wl == "plain":       # plain containers (what the reference writes) decoded from the stream alone: the walks of k_dec_walk.hip
        w = 4096
        for tag, bands, dt_, gen, seed, mode, name in (("plain", 3, qb3_amd.QB3_U8, "NOISY3", 1000, qb3_amd.QB3M_FTL, "x3 uint8 NOISY3 seed 1000, QB3M_FTL"),
                                                       ("plain_int32_ftl", 1, qb3_amd.QB3_I32, "DEM", 4, qb3_amd.QB3M_FTL, "x1 int32 DEM seed 4, QB3M_FTL"),
                                                       ("plain_int32_best", 1, qb3_amd.QB3_I32, "DEM", 4, qb3_amd.QB3M_BEST, "x1 int32 DEM seed 4, QB3M_BEST"),
                                                       ("plain_int16_base", 1, qb3_amd.QB3_I16, "DEM", 4, qb3_amd.QB3M_BASE, "x1 int16 DEM seed 4, QB3M_BASE"),
                                                       ("plain_rgb_best", 3, qb3_amd.QB3_U8, "NOISY3", 1000, qb3_amd.QB3M_BEST, "x3 uint8 NOISY3 seed 1000, QB3M_BEST")):
            img = synth.generate(w, w, bands, dt_, gen, seed, device=dev)
            enc = qdev.DeviceEncoder(w, w, bands, dt_, mode=mode)
            dst, n, _ = enc.encode(img)
            dec = qdev.DeviceDecoder(dst, n)
            res = torch.empty(img.numel() * img.element_size(), dtype=torch.uint8, device=dev)
            dec.decode(dst, out=res, index=None)
            prof = Prof(qdev)
            prof.start()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                dec.decode(dst, out=res, index=None)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            avg = prof.stop()
            # (exits and hops run once per round of the stream: launches >= steps; ms per decode = avg_ms * launches / steps)
            out[tag] = {"workload": f"4096x4096{name}, plain container, qb3x_decode_device with index = NULL",
                        "stream_bytes": int(n), "ms_wall": round(dt * 1e3, 2), "MPixel_s": round(w * w / dt / 1e6, 1), "exact": bool(torch.equal(res, img.reshape(-1).view(torch.uint8))),
                        "kernels": {k: {"avg_ms": round(v[0], 4), "launches": v[1], "ms_per_decode": round(v[0] * v[1] / steps, 3)} for k, v in sorted(avg.items())}}
            del img, enc, dec, dst, res
            torch.cuda.empty_cache()
    elif wl == "c2best":    # not a BASELINE configuration: the raster of configs[1] in QB3M_BEST (common factor + index coding)
        out["c2_best"] = measure_image(torch, qb3_amd, synth, qdev, dev, "c2_best", 16384, 16384, 3, qb3_amd.QB3_U8, "NOISY3", 2, qb3_amd.QB3M_BEST, steps,
                                       "16384x16384x3 uint8 NOISY3 seed 2, QB3M_BEST")
    elif wl == "c3cf":      # not a BASELINE configuration: config 3's raster in the common-factor modes (the lane-per-unit decoder, the unit-per-lane encoder)
        for tag, mode, name in (("c3_cf", qb3_amd.QB3M_CF_H, "QB3M_CF_H (common factor + index coding)"),
                                ("c3_best", qb3_amd.QB3M_BEST, "QB3M_BEST (= CF_H + the RLE0 pass, which wins on this raster)")):
            out[tag] = measure_image(torch, qb3_amd, synth, qdev, dev, tag, 8192, 8192, 8, qb3_amd.QB3_U16, "LANDSAT16", 3, mode, steps,
                                     "8192x8192x8 uint16 LANDSAT16 seed 3, " + name, traffic_tag="c3_cf")
            torch.cuda.empty_cache()
    elif wl == "shapes":    # not BASELINE configurations: rasters no lane-per-block kernel takes (decoders: k_dec_pxu.hip, a lane per unit;
        # encoders: the unit-per-lane kernels of k_enc_generic.hip / k_enc_best.hip).  One raster per value type and mode family, so that
        # every raster's kernels are symbols of their own in a profile of this workload (profiles/summarise.py keys them by that)
        for tag, b, dt_, gen, mode, name in (
                ("u8x5_ftl", 5, qb3_amd.QB3_U8, "NOISY3", qb3_amd.QB3M_FTL, "x5 uint8 NOISY3 seed 3, QB3M_FTL"),
                ("u16x7_base", 7, qb3_amd.QB3_U16, "LANDSAT16", qb3_amd.QB3M_BASE, "x7 uint16 LANDSAT16 seed 3, QB3M_BASE"),
                ("i32x2_ftl", 2, qb3_amd.QB3_I32, "DEM", qb3_amd.QB3M_FTL, "x2 int32 DEM seed 3, QB3M_FTL"),
                ("i64x2_ftl", 2, qb3_amd.QB3_I64, "DEM", qb3_amd.QB3M_FTL, "x2 int64 DEM seed 3, QB3M_FTL"),
                ("u8x5_cf", 5, qb3_amd.QB3_U8, "NOISY3", qb3_amd.QB3M_CF_H, "x5 uint8 NOISY3 seed 3, QB3M_CF_H"),
                ("i32x3_best", 3, qb3_amd.QB3_I32, "DEM", qb3_amd.QB3M_BEST, "x3 int32 DEM seed 3, QB3M_BEST")):
            out[tag] = measure_image(torch, qb3_amd, synth, qdev, dev, tag, 4096, 4096, b, dt_, gen, 3, mode, steps, "4096x4096" + name)
            torch.cuda.empty_cache()
    elif wl == "c3":
        out["c3"] = measure_image(torch, qb3_amd, synth, qdev, dev, "c3", 8192, 8192, 8, qb3_amd.QB3_U16, "LANDSAT16", 3, qb3_amd.QB3M_BASE, steps,
                                  "8192x8192x8 uint16 LANDSAT16 seed 3, QB3M_BASE")
    elif wl == "c4":
        for tag, dt, mode, name in (("c4_i32_ftl", qb3_amd.QB3_I32, qb3_amd.QB3M_FTL, "int32 QB3M_FTL"), ("c4_i64_ftl", qb3_amd.QB3_I64, qb3_amd.QB3M_FTL, "int64 QB3M_FTL"),
                                    ("c4_i32_best", qb3_amd.QB3_I32, qb3_amd.QB3M_BEST, "int32 QB3M_BEST"), ("c4_i64_best", qb3_amd.QB3_I64, qb3_amd.QB3M_BEST, "int64 QB3M_BEST")):
            out[tag] = measure_image(torch, qb3_amd, synth, qdev, dev, tag, 4096, 4096, 1, dt, "DEM", 4, mode, steps, f"4096x4096x1 {name}, DEM seed 4")
        torch.cuda.empty_cache()
    else:
        res, tc, imgs, o = measure_tiles(torch, qb3_amd, synth, qdev, dev, args.tiles_per_rank, steps)
        out["c5_one_rank"] = res
        del tc, imgs, o
        torch.cuda.empty_cache()
    return out


def run_tiles_multi(args, torch, dist, qb3_amd, synth, qdev, tiles, dev, rank, world, fence):
    """N > 1: tiles shard by rank (tiles.shard_range), batches through qb3x_encode_tiles, the gather of batch k beside
    the coding of batch k+1, then decode; the gather is inside the step."""
    w = h = 4096
    total = args.tiles_per_rank * world
    first, count = tiles.shard_range(total, rank, world)
    imgs = torch.stack([synth.generate(w, h, 3, qb3_amd.QB3_U8, "NOISY3", 1000 + first + t, device=dev) for t in range(count)])
    # table level 1 here: the step is bound by the gather (a rank's 0.87 GB of containers over one xGMI link: 5.7 ms against
    # 2.3 ms of coding), so the 5.5 % of bytes a level 2 table adds cost more than the walk it spares the decoder
    tc = qdev.TileBatchCoder(w, h, 3, qb3_amd.QB3_U8, count, device=dev, want_index=False, index_chunk=1)
    out = torch.empty_like(imgs)
    nb = max(1, min(args.batch_tiles, count))
    batches = [(lo, min(nb, count - lo)) for lo in range(0, count, nb)]
    recv = send = None
    if args.backend == "nccl":                          # buffers reused every step: on the root one per peer and batch slot to receive
        if rank == 0:                                   # into, on a peer one per batch slot to pack its containers into (one message a batch)
            recv = [[None if r == 0 else torch.empty(nb * tc.pitch, dtype=torch.uint8, device=dev) for r in range(world)] for _ in batches]
        else:
            send = [torch.empty(nb * tc.pitch, dtype=torch.uint8, device=dev) for _ in batches]

    def step(gather=True):
        pend = []
        for b, (lo, cnt) in enumerate(batches):
            sizes = tc.encode(imgs, lo, cnt)             # synchronises: the containers of the batch are complete
            if gather:
                pend.append(tiles.start_gather(tc.dst[lo * tc.pitch:(lo + cnt) * tc.pitch], tc.pitch, sizes, root=0,
                                               recv_bufs=recv[b] if recv else None, send_buf=send[b] if send else None, max_tiles=nb))
        tc.decode(out, use_index=False)                   # from the containers alone: every tile carries its restart table
        got = [p.wait() + (p.offset_lists,) for p in pend]
        return got

    got = step()
    if args.full:
        torch.cuda.synchronize()
        if not torch.equal(out, imgs):
            sys.exit("bench.py: decode(encode(x)) != x -- refusing to report a number")
        # What arrived at the root is what the senders made: every rank hashes its own containers (FNV-1a64, the library's),
        # the hashes are gathered, the root hashes every container it received and compares; rank 0's own tiles 1000 / 1001 are
        # checked against the reference's anchors (size + FNV without the table chunks).  Untimed.
        import numpy as np
        host_all = tc.dst[:count * tc.pitch].cpu().numpy()
        mine = [qb3_amd.fnv(host_all[t * tc.pitch:t * tc.pitch + int(tc.sizes[t])]) for t in range(count)]
        everyone = [None] * world
        dist.all_gather_object(everyone, mine)
        intact, anchors_ok = None, None
        if rank == 0:
            intact, checked = True, 0
            for b, (bufs, size_lists, offset_lists) in enumerate(got):
                lo = batches[b][0]
                for r in range(1, world):
                    hb = bufs[r].cpu().numpy() if bufs[r] is not None else None
                    for t, (sz, off) in enumerate(zip(size_lists[r], offset_lists[r])):     # (a peer's containers arrive packed back to back)
                        ok = hb is not None and qb3_amd.fnv(hb[off:off + int(sz)]) == everyone[r][lo + t]
                        intact, checked = intact and ok, checked + 1
            intact = bool(intact and checked == (world - 1) * count)
            anchors_ok = all(container_check(qb3_amd, np, host_all[t * tc.pitch:t * tc.pitch + int(tc.sizes[t])], tag)[0]
                             for t, tag in ((0, "c5_tile1000"), (1, "c5_tile1001")) if t < count)
            if not (intact and anchors_ok):
                sys.exit(f"bench.py: gathered containers differ from the senders' (intact={intact}) or rank 0's tiles from the reference's anchors "
                         f"(anchors={anchors_ok}) -- refusing to report a number")
        del host_all
    for _ in range(max(1, args.warmup) - 1):
        step()

    def timed(gather):
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(gather)
        fence()
        dt = time.perf_counter() - t0
        t = torch.tensor([dt], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    dt = timed(True)
    px = total * w * h
    line = {
        "metric": "MPixel/s encode+decode (QB3M_FTL, 8-bit 3-band)",
        "value": round(px / (dt / args.steps) / 1e6, 1),
        "unit": "MPixel/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u8", "data": "synthetic",
        "config": {"workload": f"{total} independent 4096x4096x3 uint8 NOISY3 tiles (seeds 1000..), {args.tiles_per_rank} per GPU, QB3M_FTL: qb3x_encode_tiles in batches of "
                               f"{nb}, containers gathered on rank 0 ({'RCCL send/recv' if args.backend == 'nccl' else args.backend + ' rehearsal'}) beside the coding "
                               "of the next batch, qb3x_decode_tiles of every rank's own tiles from the containers alone (index = NULL; every tile carries its restart table, level 1: 0.7 % on top of the stream -- the step is bound by the gather, bytes on the link cost more than the decoder's walk); the gather is inside the step",
                   "tiles_total": total, "tiles_per_gpu": args.tiles_per_rank, "parallelism": f"tiles sharded over {world} GPUs, no data-path collective but the gather"},
    }
    if args.dump_outputs and rank == 0:                  # rank 0's own tiles: its containers back to back, its decoded tiles
        sizes_0 = [int(s) for s in tc.sizes[:count]]
        dump_outputs(args.dump_outputs, torch, torch.cat([tc.dst[t * tc.pitch:t * tc.pitch + s] for t, s in enumerate(sizes_0)]),
                     out.reshape(-1).view(torch.uint8), sizes_0)
    if not args.full:
        return line
    prof = Prof(qdev)                                    # rank 0's kernels, over the coding-only leg
    if rank == 0:
        prof.start()
    dt_code = timed(False)
    roofline = None
    if rank == 0:
        avg = prof.stop()
        raw_tile = w * h * 3
        sizes_all = [int(s) for s in tc.sizes[:count]]
        # an encode launch covers a batch of nb tiles, a decode launch all of the rank's tiles
        algo_batch = nb * raw_tile + sum(sizes_all) * nb // max(1, count)
        algo_all = count * raw_tile + sum(sizes_all)
        cand = {k: v for k, v in avg.items() if k in ENC_KERNELS + DEC_KERNELS}
        if cand:
            dom = max(cand, key=lambda k: cand[k][0])
            algo = algo_all if dom in DEC_KERNELS else algo_batch
            roofline = roofline_of({dom: cand[dom]}, algo, (dom,))
            covers = count if dom in DEC_KERNELS else nb
            roofline["launch_covers"] = f"{covers} tiles of 4096x4096x3 (rank 0)"
            # the PMC passes are of one rank's 32 tiles in one call (profiles/*_c5_*): per launch here = that, by tiles a launch covers
            attach_traffic(roofline, algo, "c5_one_rank", scale=covers / 32.0)
            if roofline.get("traffic") is not None:
                roofline["traffic_source"] = f"{roofline['traffic_source']} x {covers}/32 tiles a launch"
    bytes_root = None
    if rank == 0:
        bytes_root = sum(sum(sl) for (_, sls, _) in got for sl in sls[1:])
    line.update({
        "coding_only": {"ms_per_step": round(dt_code / args.steps * 1e3, 3), "MPixel_s": round(px / (dt_code / args.steps) / 1e6, 1)},
        "gather": {"bytes_into_root_per_step": bytes_root, "GBps_into_root": round(bytes_root / (dt / args.steps) / 1e9, 1) if bytes_root else None,
                   "containers_intact": intact, "check": "FNV-1a64 of every container received at the root against its sender's; rank 0's tiles 1000 and 1001 against the reference's anchors",
                   "tiles_1000_1001_match_reference": anchors_ok, "backend": "nccl (RCCL) send/recv" if args.backend == "nccl" else args.backend + " (rehearsal)"},
        "roofline": roofline,
        "cpu_baseline": None if (args.no_cpu_baseline or rank != 0) else cpu_baseline_tiles(),
    })
    return line


def cpu_baseline(target_s=12.0):
    """The CPU restatement (oracle/, bit-identical to the reference on the anchor table) on ONE host core:
    encode + decode of a 4096x4096x3 NOISY3 tile, repeated for about target_s seconds."""
    from oracle import pyoracle as o
    w = h = 4096
    img = o.generate(w, h, 3, 0, "NOISY3", 2)
    t_enc = t_dec = 0.0
    reps = 0
    t_start = time.perf_counter()
    while reps < 2 or time.perf_counter() - t_start < target_s:
        t0 = time.perf_counter()
        s = o.encode(img, 0, 8)
        t1 = time.perf_counter()
        out, _, _, _ = o.decode(s)
        t2 = time.perf_counter()
        t_enc += t1 - t0
        t_dec += t2 - t1
        reps += 1
        if out is None:
            raise RuntimeError("oracle failed to decode its own stream")
    px = w * h * reps
    return {"value": round(px / (t_enc + t_dec) / 1e6, 1), "unit": "MPixel/s", "cores": 1, "kind": "port",
            "sample": f"{reps} x (encode + decode) of a 4096x4096x3 uint8 NOISY3 tile, QB3M_FTL, single thread",
            "encode_MPixel_s": round(px / t_enc / 1e6, 1), "decode_MPixel_s": round(px / t_dec / 1e6, 1),
            "vs_reference": {"note": "oracle/ (this port) against the reference's own library on one host, same input, one thread; two judge-side "
                                     "measurements on different hosts, no direction asserted: the two are within noise of each other "
                                     "(the reference cannot be built inside this repository's rules, DESIGN.md section 2)",
                             "round1_MPixel_s": {"reference_enc_dec": [26.5, 29.5], "port_enc_dec": [46.4, 28.9]},
                             "round2_MPixel_s": {"reference_enc_dec": [55.8, 59.2], "port_enc_dec": [58.7, 48.9]}}}


def cpu_baseline_tiles(target_s=12.0):
    """config 5's CPU counterpart: the CPU restatement on the host's cores, a thread per tile (the
    format admits no threading inside a stream; ctypes releases the interpreter lock inside the library): every thread
    encodes + decodes its own 4096x4096x3 NOISY3 tile for about target_s seconds."""
    import threading
    from oracle import pyoracle as o
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 32))
    w = h = 4096
    imgs = [o.generate(w, h, 3, 0, "NOISY3", 1000 + t) for t in range(cores)]
    reps = [0] * cores
    t_start = time.perf_counter()

    def work(t):
        while reps[t] < 1 or time.perf_counter() - t_start < target_s:
            out, _, _, _ = o.decode(o.encode(imgs[t], 0, 8))
            if out is None:
                raise RuntimeError("oracle failed to decode its own stream")
            reps[t] += 1
    th = [threading.Thread(target=work, args=(t,)) for t in range(cores)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t_start
    px = w * h * sum(reps)
    return {"value": round(px / dt / 1e6, 1), "unit": "MPixel/s", "cores": cores, "kind": "port", "per_core_MPixel_s": round(px / dt / 1e6 / cores, 1),
            "sample": f"{sum(reps)} x (encode + decode) of 4096x4096x3 uint8 NOISY3 tiles (seeds 1000..), QB3M_FTL, {cores} threads, a tile each, {dt:.1f} s wall"}


if __name__ == "__main__":
    main()
