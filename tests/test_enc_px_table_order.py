"""The level-2 table that enc_px_kernel writes (k_enc_px.hip, px_table_entries) at the places where its address arithmetic can go wrong:
a workgroup's entries lie in two table chunks, a chunk of one block, entries that begin inside a chunk of the coder.  Wherever in the
kernel the entries are emitted and however their addresses are made (DESIGN "The coding kernels: sixteen bytes a lane in the decoder's
staging" tells of a move that was measured and not kept), the bytes are these.  Every container is held, byte for byte, to
tests/qb3_table_spec.py fed with the CPU oracle's unit trace (as tests/test_table_spec.py does), into a destination filled with 0x00 and
again with 0xA5, and is decoded from its table alone.

uint8, level 2.  Rasters: one band, three bands with the default R-G, G, B-G map and with the identity map, four bands.  Modes: FTL and
BASE on the Hilbert curve, BASE on the Z curve (QB3M_BASE_Z: the format has no FTL on the Z curve).  Shapes:
  1008 x 4     252 blocks: exactly one chunk of the coder
  1012 x 4     253 blocks: the last chunk is one block, and the last entry's empty groups are written behind it
  509 x 259    shifted edge blocks; chunks that start inside a segment (252 is no multiple of 64)
  1024 x 772   three bands only: 49 408 blocks, 772 entries of 92 bytes, more than the 712 a table chunk holds -- a workgroup's entries
               straddle a chunk's head and pad"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_table_spec as T  # noqa: E402
import test_table_spec as TS  # noqa: E402

U8 = 0
FTL, BASE, BASE_Z = 8, 4, 0
MODE_NAME = {FTL: "FTL", BASE: "BASE", BASE_Z: "BASE_Z"}
SMALL = [(1008, 4), (1012, 4), (509, 259)]
BIG = (1024, 772)
RASTERS = [(1, None, "x1"), (3, None, "x3-rgb"), (3, [0, 1, 2], "x3-identity"), (4, None, "x4")]


class Case:
    def __init__(self, bands, cband, name, mode, shape):
        self.dtype, self.bands, self.cband, self.mode, self.shape = U8, bands, cband, mode, shape
        self.id = "%s-%s-%dx%d" % (name, MODE_NAME[mode], shape[0], shape[1])


CASES = [Case(b, cb, name, mode, shape) for b, cb, name in RASTERS for mode in (FTL, BASE, BASE_Z) for shape in SMALL]
CASES += [Case(3, None, "x3-rgb", mode, BIG) for mode in (FTL, BASE, BASE_Z)]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES) == 39
ids = lambda c: c.id      # noqa: E731

_made = {}


def made(oracle, c, seed=0):
    """(raster, the spec's table bytes, its Table, the expected container): made once a case, shared, left unchanged"""
    key = (c.id, seed)
    if key not in _made:
        w, h = c.shape
        img = TS.mixed_raster(w, h, c.bands, U8, 300 + seed + len(c.id), False)
        u = T.units(oracle, img, U8, c.mode, c.cband)
        ev = T.entering_values(img, U8, c.cband, T.curve_order(c.mode))
        want_bytes, want = T.build(u, ev, U8, c.mode, 2)
        ref = oracle.encode(img, U8, c.mode, cband=c.cband)
        _made[key] = (img, want_bytes, want, TS.with_table(ref, want_bytes))
    return _made[key]


def held(c, container, want_bytes, want, expected, what):
    try:
        T.compare(container, want_bytes, want, U8, c.mode)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None
    assert bytes(container) == expected, "%s: minus its table, the oracle's container" % what


def decoded_from_the_table(qb3, container):
    import torch
    from qb3_amd import device as qdev
    n = len(container)
    d = torch.zeros((n + 3) // 4 * 4, dtype=torch.uint8, device="cuda")
    d[:n] = torch.from_numpy(np.frombuffer(container, dtype=np.uint8).copy())
    dec = qdev.DeviceDecoder(d, n)
    out = dec.decode(d, index=None).cpu().numpy()
    status = qb3.lib.qb3x_last_decode_status(dec.p)
    dec.close()
    return out, status


# ------------------------------------------------------------------------------------------------------------------- CPU: the cases


def test_shapes_are_what_their_case_says():
    lay = T.layout(U8, 3, FTL, 2)
    assert lay["blocks"] == 64 and lay["entry_bytes"] == 92
    blocks = lambda s: ((s[0] + 3) // 4) * ((s[1] + 3) // 4)      # noqa: E731
    assert [blocks(s) for s in SMALL] == [252, 253, 128 * 65] and blocks(BIG) == 49408
    per_chunk = (T.CHUNK_MAX - 12) // 92
    assert per_chunk == 712 and 712 < 49408 // 64 == 772, "more than one table chunk"
    # the workgroup of the chunk that holds block 64 * 712 also holds blocks of the entry in front of it: its entries straddle the head
    assert (64 * 712) % 252 != 0
    # 253 blocks: four entries cover 256 blocks; the groups of blocks 256.. do not exist, those of 253..255 are the last chunk's own
    assert (253 + 63) // 64 == 4


# ------------------------------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=ids)
def test_table_is_the_specs_whatever_the_destination_held(qb3, oracle, c):
    img, want_bytes, want, expected = made(oracle, c)
    zero, a5 = (TS.device_encode(qb3, c, img, 2, False, fill) for fill in (0x00, 0xA5))
    assert zero == a5, "the container depends on what the destination held"
    held(c, zero, want_bytes, want, expected, "the device call")
    got = T.parse(zero)[0]
    assert got.lay["kind"] == T.BLOCK10
    if c.shape == BIG:
        assert len(got.heads) == 2, "more than one chunk"
    out, status = decoded_from_the_table(qb3, zero)
    assert status == 0
    assert np.array_equal(out, img.reshape(-1)), "decode(index=None) does not give the pixels"


@pytest.mark.gpu
def test_with_the_out_of_band_index_asked_for(qb3, oracle):
    """the same coder writes the index's arrays and the table's entries: the container does not depend on it"""
    c = BY_ID["x3-rgb-FTL-509x259"]
    img, want_bytes, want, expected = made(oracle, c)
    for fill in (0x00, 0xA5):
        held(c, TS.device_encode(qb3, c, img, 2, True, fill), want_bytes, want, expected, "with the index, fill %#x" % fill)


@pytest.mark.gpu
def test_tile_batch_of_two(qb3, oracle):
    """qb3x_encode_tiles, two tiles (blockIdx.y in play): every container its own table, at its own place"""
    import torch
    from qb3_amd import device as qdev
    c = BY_ID["x3-rgb-BASE-509x259"]
    tiles = [made(oracle, c, seed) for seed in (0, 1)]
    w, h = c.shape
    tc = qdev.TileBatchCoder(w, h, c.bands, U8, 2, mode=c.mode, want_index=False, index_chunk=2)
    for fill in (0x00, 0xA5):
        tc.dst.fill_(fill)
        tc.encode(torch.from_numpy(np.stack([t[0] for t in tiles]).reshape(-1).copy()).cuda())
        host = tc.dst.cpu().numpy()
        for t, (img, want_bytes, want, expected) in enumerate(tiles):
            held(c, host[t * tc.pitch:t * tc.pitch + tc.sizes[t]].tobytes(), want_bytes, want, expected, "tile %d, fill %#x" % (t, fill))
    tc.close()
