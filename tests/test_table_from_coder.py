"""Level-2 restart tables of the 8-bit lane-per-block FTL/BASE coder (k_enc_px.hip): the coding kernel writes the entries, the
concatenation launch their stream positions, chunk heads and checks.  Every table here is checked byte for byte against one
rebuilt in numpy from the out-of-band index of the same encode (layout: qb3_dev.h, IndexView; table: IxTable, include/qb3x.h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FTL, BASE = 8, 4
IX_HEAD = 12


def _a8(v):
    return (v + 7) & ~7


def rebuild_table(index, w, h, b):
    """the level-2 table (an entry per 64-block segment: position, rungs, entering values, sixteen groups of four ten-bit block
    lengths), its chunks with heads, pads and checks, and the closing "DT", from the index of an 8-bit raster of b bands"""
    index = np.asarray(index, np.uint8)
    nblocks = ((w + 3) // 4) * ((h + 3) // 4)
    nseg = (nblocks + 63) // 64
    off = 0
    bitpos = np.frombuffer(index[:8 * nseg].tobytes(), "<u8")
    off += _a8(8 * nseg)
    prev = index[off:off + nseg * b].reshape(nseg, b)
    off += 2 * _a8(nseg * b)                            # entering values, then the factors (none in FTL / BASE)
    rung = index[off:off + nseg * b].reshape(nseg, b)
    off += _a8(nseg * b)
    ulen = index[off:off + nblocks * b].reshape(nblocks, b).astype(np.uint64)
    bl = np.zeros(nseg * 64, np.uint64)
    bl[:nblocks] = ulen.sum(1)
    g = bl.reshape(nseg, 16, 4)
    packed = g[:, :, 0] | g[:, :, 1] << np.uint64(10) | g[:, :, 2] << np.uint64(20) | g[:, :, 3] << np.uint64(30)
    lens = ((packed[:, :, None] >> (np.uint64(8) * np.arange(5, dtype=np.uint64))) & np.uint64(255)).astype(np.uint8).reshape(nseg, 80)
    pos = ((bitpos[:, None] >> (np.uint64(8) * np.arange(6, dtype=np.uint64))) & np.uint64(255)).astype(np.uint8)
    entries = np.concatenate([pos, rung, prev, lens], axis=1)
    E = entries.shape[1]
    per_chunk = (65535 - IX_HEAD) // E
    out = []
    for c0 in range(0, nseg, per_chunk):
        body = entries[c0:c0 + per_chunk].reshape(-1)
        i = np.arange(len(body), dtype=np.uint64)
        s = int(((body.astype(np.uint64) + np.uint64(1)) * ((i * np.uint64(0x9E3779B1) + np.uint64(1)) & np.uint64(0xFFFFFFFF))).sum()) & 0xFFFFFFFF
        f = (s ^ (s >> 16)) & 0xFFFF
        ln = IX_HEAD + len(body)
        head = bytes([ord("i"), ord("x"), ln & 255, ln >> 8, 3, 2, f & 255, f >> 8]) + (64).to_bytes(4, "little")
        out.append(head + body.tobytes() + b"zz\x04\x00")
    return b"".join(out) + b"DT"


def table_span(c):
    """[start, end) of a container's table chunks, "DT" included"""
    pos, t0 = 11, None
    c = bytes(c)
    while pos + 4 <= len(c):
        sig, ln = c[pos:pos + 2], c[pos + 2] | c[pos + 3] << 8
        if sig == b"DT":
            assert t0 is not None, "no table"
            return t0, pos + 2
        if sig in (b"ix", b"zz"):
            t0 = pos if t0 is None else t0
            pos += ln
        elif sig in (b"CB", b"QV", b"SC"):
            pos += 4 + ln
        else:
            raise AssertionError("unexpected chunk %r at %d" % (sig, pos))
    raise AssertionError("no DT")


def check_container(oracle, host, index, img_host, w, h, b, mode):
    t0, t1 = table_span(host)
    want = rebuild_table(index, w, h, b)
    got = bytes(host[t0:t1])
    assert len(got) == len(want), (len(got), len(want))
    if got != want:
        d = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError("table differs from the index's at byte %d of %d" % (d, len(got)))
    ref = oracle.encode(img_host, 0, mode)
    dt_at = bytes(ref).index(b"DT", 11)
    assert t0 == dt_at
    assert bytes(host[:t0]) == bytes(ref[:dt_at]) and bytes(host[t1 - 2:]) == bytes(ref[dt_at:]), "minus its table, the oracle's container"


SHAPES = [(509, 259, 3, FTL), (509, 259, 3, BASE), (333, 77, 4, BASE), (1021, 13, 1, FTL), (1000, 4, 3, FTL),
          (1012, 4, 4, BASE), (1024, 4, 1, FTL), (508, 508, 3, FTL), (1030, 1027, 3, FTL), (1030, 1027, 4, BASE), (2050, 1029, 1, BASE)]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "%dx%dx%d-m%d" % c)
def test_table_matches_the_index(qb3, oracle, case):
    """widths and heights that are not multiples of 4 (or of a chunk's blocks), 1 / 3 / 4 bands, FTL and BASE, one block row (a
    single chunk whose last entry reaches past it), a last chunk of one block (508 x 508: 252 * 64 + 1 blocks), several table
    chunks: the same table whether the index is asked for or not, the index's table, decoded from the table alone"""
    import torch
    from qb3_amd import device as qdev
    w, h, b, mode = case
    himg = oracle.generate(w, h, b, 0, "NOISY3", 17)
    img = torch.from_numpy(himg.copy()).cuda().view(-1)
    e1 = qdev.DeviceEncoder(w, h, b, 0, mode=mode, want_index=True, index_chunk=2)
    d1, n1, index = e1.encode(img)
    host = d1[:n1].cpu().numpy()
    check_container(oracle, host, index.cpu().numpy(), himg, w, h, b, mode)
    e0 = qdev.DeviceEncoder(w, h, b, 0, mode=mode, want_index=False, index_chunk=2)
    d0, n0, _ = e0.encode(img)
    assert n0 == n1 and np.array_equal(d0[:n0].cpu().numpy(), host)
    dec = qdev.DeviceDecoder(d0, n0)
    assert torch.equal(dec.decode(d0, index=None), img)
    assert qb3.lib.qb3x_last_decode_status(dec.p) == 0


def test_table_matches_the_index_in_tile_batches(qb3, oracle):
    """qb3x_encode_tiles: every tile's table is its index's; decoded from the containers alone"""
    import torch
    from qb3_amd import device as qdev, synth
    w, h, n = 509, 387, 5
    imgs = torch.stack([synth.generate(w, h, 3, 0, "NOISY3", 900 + t) for t in range(n)])
    tc = qdev.TileBatchCoder(w, h, 3, 0, n, want_index=True, index_chunk=2)
    tc.encode(imgs)
    host, idx = tc.dst.cpu().numpy(), tc.index.cpu().numpy()
    for t in range(n):
        c = host[t * tc.pitch:t * tc.pitch + tc.sizes[t]]
        check_container(oracle, c, idx[t * tc.index_bytes:(t + 1) * tc.index_bytes], imgs[t].cpu().numpy(), w, h, 3, FTL)
    t2 = qdev.TileBatchCoder(w, h, 3, 0, n, want_index=False, index_chunk=2)
    t2.encode(imgs)
    for t in range(n):
        assert t2.sizes[t] == tc.sizes[t]
        assert torch.equal(t2.dst[t * t2.pitch:t * t2.pitch + t2.sizes[t]], tc.dst[t * tc.pitch:t * tc.pitch + tc.sizes[t]])
    out = torch.zeros_like(imgs)
    t2.decode(out, use_index=False)
    assert torch.equal(out, imgs)


@pytest.mark.parametrize("case", [(8192, 4099, 3, FTL), (8192, 4100, 4, BASE)], ids=lambda c: "%dx%dx%d-m%d" % c)
def test_table_of_the_pipelined_host_call(qb3, oracle, case):
    """qb3_encode on a raster large enough for the strip pipeline writes the table the one-shot device call writes, which is the
    index's; the container decodes"""
    import torch
    from qb3_amd import device as qdev
    w, h, b, mode = case
    himg = oracle.generate(w, h, b, 0, "NOISY3", 23)
    img = torch.from_numpy(himg.copy()).cuda().view(-1)
    d, n, index = qdev.DeviceEncoder(w, h, b, 0, mode=mode, want_index=True, index_chunk=2).encode(img)
    dev = d[:n].cpu().numpy()
    check_container(oracle, dev, index.cpu().numpy(), himg, w, h, b, mode)
    got = qb3.encode(himg, 0, mode, index_chunk=2)
    assert len(got) == n and np.array_equal(got, dev)
    out, dims, _, _ = qb3.decode(got)
    assert dims == (w, h, b) and np.array_equal(out, himg.ravel())
