"""Level-2 restart tables of the 8-bit lane-per-block FTL/BASE coder (k_enc_px.hip): the coding kernel writes the entries, the
concatenation launch their stream positions, chunk heads and checks.  Every table here is checked byte for byte against one
rebuilt from the out-of-band index of the same encode (layout: qb3_dev.h, IndexView) -- the coder agrees with itself -- and against
the one tests/qb3_table_spec.py builds from the CPU oracle's unit trace and the pixels -- and with a truth that is not its own.  The
entry packing, the chunk heads and the check are the spec module's (include/qb3x.h in numpy), stated there once."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_table_spec as T  # noqa: E402
from qb3_table_spec import table_span  # noqa: E402,F401

pytestmark = pytest.mark.gpu

FTL, BASE = 8, 4


def _a8(v):
    return (v + 7) & ~7


def rebuild_table(index, w, h, b):
    """the level-2 table (an entry per 64-block segment: position, rungs, entering values, a ten-bit length per block), its chunks
    with heads, pads and checks, and the closing "DT", from the index of an 8-bit raster of b bands"""
    index = np.asarray(index, np.uint8)
    nblocks = ((w + 3) // 4) * ((h + 3) // 4)
    nseg = (nblocks + 63) // 64
    off = 0
    t = T.Table()
    t.lay = T.layout(0, b, FTL, 2)
    t.pos = np.frombuffer(index[:8 * nseg].tobytes(), "<u8")
    off += _a8(8 * nseg)
    t.prev = index[off:off + nseg * b].reshape(nseg, b).astype(np.uint64)
    off += 2 * _a8(nseg * b)                            # entering values, then the factors (none in FTL / BASE)
    t.rungs = index[off:off + nseg * b].reshape(nseg, b)
    off += _a8(nseg * b)
    ulen = index[off:off + nblocks * b].reshape(nblocks, b).astype(np.int64)
    bl = np.zeros(nseg * 64, np.int64)
    bl[:nblocks] = ulen.sum(1)
    t.cf, t.fields = None, bl.reshape(nseg, 64)
    return T.assemble(t)


def check_container(oracle, host, index, img_host, w, h, b, mode):
    t0, t1 = table_span(host)
    want = rebuild_table(index, w, h, b)
    got = bytes(host[t0:t1])
    assert len(got) == len(want), (len(got), len(want))
    if got != want:
        d = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError("table differs from the index's at byte %d of %d" % (d, len(got)))
    img = np.ascontiguousarray(img_host).reshape(h, w, b)
    spec_bytes, spec = T.build(T.units(oracle, img, 0, mode), T.entering_values(img, 0), 0, mode, 2)
    assert T.compare(bytes(host), spec_bytes, spec, 0, mode) == (t0, t1)
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
