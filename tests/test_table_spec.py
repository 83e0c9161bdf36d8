"""The restart table's bytes, field by field, against tests/qb3_table_spec.py: the format of include/qb3x.h in numpy, fed with the CPU
oracle's unit trace and the pixels -- a truth the library had no hand in.

CPU part: the truth is held to account first (parse inverts build; positions, rungs and entering values decode the stream; lengths add
up; the last entering values are the oracle's band state) and every raster of the GPU matrix is shown to exercise what its case is
about.  GPU part: the table of every encoder flavour (device call with and without the out-of-band index, into destinations filled
with 0x00 and with 0xA5; host call; tile batch) and of reindex equals build(...) byte for byte, reported through parse.

No quantised rasters: the entering values would be those of the quantised pixels (qb3_table_spec does not model them)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_spec as S  # noqa: E402
import qb3_table_spec as T  # noqa: E402

BASE_Z, CF, BASE, CF_H, BEST, FTL = 0, 1, 4, 5, 7, 8
U8, U16, I16, U32, I32, U64, I64 = 0, 2, 3, 4, 5, 6, 7
NPTYPE = (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64)
SHAPES = [(260, 20), (64, 64), (258, 18)]       # 325 blocks; exactly 4 segments of 64; a shifted last column and row
MODE_NAME = {FTL: "FTL", BASE: "BASE", CF: "CF", CF_H: "CF_H", BEST: "BEST"}
TYPE_NAME = {U8: "u8", U16: "u16", I16: "i16", U32: "u32", I32: "i32", U64: "u64", I64: "i64"}


class Case:
    def __init__(self, cls, dtype, bands, mode, shape, cband=None, kind="mixed"):
        self.cls, self.dtype, self.bands, self.mode, self.shape, self.kind = cls, dtype, bands, mode, shape, kind
        self.cband = cband if cband is not None else (None if bands in (1, 3, 4) else list(range(bands)))
        self.cf = mode not in T.PLAIN_MODES
        self.id = "%s-%s-x%d%s-%s-%s" % (cls, TYPE_NAME[dtype], bands, "-map" if cband is not None else "", MODE_NAME[mode],
                                         kind if shape is None else "%dx%d" % shape)


def _matrix():
    cases, n = [], 0

    def add(cls, dtype, bands, modes, **kw):
        nonlocal n
        for mode in modes:
            cases.append(Case(cls, dtype, bands, mode, kw.pop("shape", None) or SHAPES[n % 3], **kw))
            n += 1

    for b in (1, 3, 4):
        add("A", U8, b, (FTL, BASE))
    for b in (1, 2, 3, 4, 6, 8, 10, 12):
        add("B", U16, b, (FTL, BASE))
        add("B", I16, b, (FTL, BASE))
    for dt in (U32, I64):
        for mode in (FTL, BASE):
            cases.append(Case("C", dt, 1, mode, None, kind="units"))
    for dt, b in ((U8, 2), (U8, 5), (U8, 16), (U16, 5), (U16, 7), (I32, 3), (U64, 2)):
        add("D", dt, b, (FTL, BASE))
    for b in (1, 3, 4):
        add("E", U8, b, (CF, CF_H, BEST))
    for dt in (U16, I32, I64):
        cases.append(Case("F", dt, 1, CF_H, None, kind="units"))
    for dt, b in ((U8, 2), (U8, 5), (U16, 8), (I32, 2)):
        add("G", dt, b, (CF_H,))
    add("G", U16, 8, (CF_H,), cband=[1, 1, 1, 3, 4, 5, 6, 7])
    cases.append(Case("H", U8, 3, BEST, (260, 37), kind="const"))
    # a patch of noise in a flat raster: blocks of four 8-bit bands and 16-bit band pairs longer than 511 bits
    cases.append(Case("A", U8, 4, FTL, (64, 68), kind="patch"))
    cases.append(Case("B", U16, 4, FTL, (64, 68), kind="patch"))
    return cases


MATRIX = _matrix()
# more than one chunk: 719 entries of 92 bytes (712 a chunk), 318 entries of 207 bytes (316 a chunk)
BIG = [Case("A", U8, 3, BASE, (860, 856)), Case("E", U8, 3, CF_H, (576, 564))]
# one case a class for the other writers (host call, tile batch, reindex): the first, for B the first with band pairs
FIRST_OF_CLASS = {}
for _c in MATRIX:
    if _c.cls != "B" or _c.bands == 4:
        FIRST_OF_CLASS.setdefault(_c.cls, _c)


def mixed_raster(w, h, b, dtype, seed, cf):
    """blocks whose values spread over 2^k, k drawn a block and band from 0 to the type's width (rungs on both sides of every
    threshold); for the common-factor modes runs of four blocks that are multiples of one factor (the first unit behind a change
    brings the factor, the next keep it), blocks of three distinct values (index units) and 64-bit spreads held to 2^40 (no unit
    near the 800 bits of SURVEY B-2)"""
    rng = np.random.default_rng(seed)
    tsz = T.TYPESIZE[dtype]
    bits = 8 * tsz
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    top = min(bits, 40) if cf else bits
    k = rng.integers(0, top + 1, (nby, nbx, b))
    full = (1 << bits) - 1
    masks = np.array([[[full if e >= bits else (1 << int(e)) - 1 for e in row] for row in plane] for plane in k], dtype=np.uint64)
    r = rng.integers(0, 1 << 63, (4 * nby, 4 * nbx, b), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (4 * nby, 4 * nbx, b), dtype=np.uint64)
    up = lambda a: np.repeat(np.repeat(a, 4, axis=0), 4, axis=1)      # noqa: E731
    img = (np.uint64(1 << (bits - 2)) + (r & up(masks))) & np.uint64(full)
    if cf:
        facs = [3, 5, 7] if tsz == 1 else [3, 257, 11] if tsz == 2 else [5, (1 << 20) + 3, 9]
        run = (np.arange(nbx)[None, :] // 4 + np.arange(nby)[:, None])           # a factor a run of four blocks
        fac = np.array(facs, dtype=np.uint64)[run % 3]
        is_cf = (run % 2 == 0)
        kk = np.minimum(k[..., 0], bits - 2 - np.array([int(f).bit_length() for f in facs])[run % 3]).clip(1)
        small = np.array([[(1 << int(e)) - 1 for e in row] for row in kk], dtype=np.uint64)
        mult = up(fac)[..., None] * (np.uint64(1) + (r & up(small)[..., None]))
        img = np.where(up(is_cf)[..., None], mult, img)
        pal = rng.integers(0, 1 << min(bits - 1, 30), (nby, nbx, b, 3), dtype=np.uint64)
        pick = rng.integers(0, 3, (4 * nby, 4 * nbx, b))
        palv = np.take_along_axis(up(pal), pick[..., None], axis=-1)[..., 0]
        is_ix = (~is_cf) & ((np.arange(nbx)[None, :] + np.arange(nby)[:, None]) % 3 == 0)
        img = np.where(up(is_ix)[..., None], palv, img)
    return np.ascontiguousarray(img[:h, :w].astype(T.UNSIGNED[dtype]).view(NPTYPE[dtype]))


def units_raster(dtype, best):
    """qb3_spec.unit_raster stacked three high; FTL / BASE: the last block is a checkerboard of 0 and 2^(bits - 1) -- every delta the
    type's largest, every code the longest (65 bits at 64) -- the longest unit there is"""
    tsz = T.TYPESIZE[dtype]
    img = np.vstack([S.unit_raster(tsz, bool(dtype & 1), best, seed) for seed in (3, 4, 5)])
    if not best:
        yy, xx = np.mgrid[0:4, 0:4]
        img[-4:, -4:] = (((xx + yy) & 1).astype(np.uint64) << np.uint64(8 * tsz - 1)).astype(T.UNSIGNED[dtype]).view(img.dtype)
    return np.ascontiguousarray(img.reshape(img.shape[0], img.shape[1], 1))


def without_dropped_units(oracle, img, dtype, mode):
    """64-bit common-factor rasters: a plain unit at a rung near 50 and above is longer than 800 bits, and the reference drops such a
    unit where it cannot be an index unit (SURVEY B-2) -- qb3_spec.unit_raster has two, where a run of multiples begins.  Such a block
    is made flat (its first value): two distinct deltas, an index unit; the multiples behind it still bring and keep their factor"""
    img = img.copy()
    nbx = img.shape[1] // 4
    for _ in range(4):
        _, n, rows, _ = T._raw_trace(oracle, img, dtype, mode, None, fix_b2=True)
        long = np.flatnonzero(np.diff(np.append(rows[:, 0].astype(np.int64), n)) > 800)
        if not len(long):
            return img
        for i in long:
            y, x = 4 * (int(i) // nbx), 4 * (int(i) % nbx)
            img[y:y + 4, x:x + 4] = img[y, x]
    raise AssertionError("units above 800 bits remain")


@functools.lru_cache(maxsize=None)
def _raster(cid, seed):
    from oracle import pyoracle         # (what the `oracle` fixture hands out)
    c = BY_ID[cid]
    if c.kind == "units":
        img = units_raster(c.dtype, c.cf)
        return without_dropped_units(pyoracle, img, c.dtype, c.mode) if c.cf and T.TYPESIZE[c.dtype] == 8 else img
    w, h = c.shape
    if c.kind == "const":               # the raster of test_window_best_plan.py::test_const_is_the_container_whose_rle_pass_won
        return pyoracle.generate(w, h, c.bands, c.dtype, "CONST", 1)
    if c.kind == "patch":
        rng = np.random.default_rng(5 + seed)
        img = np.full((h, w, c.bands), 1000 % (1 << 8 * T.TYPESIZE[c.dtype]), dtype=NPTYPE[c.dtype])
        img[8:24, 16:48] = rng.integers(0, 1 << 8 * T.TYPESIZE[c.dtype], (16, 32, c.bands))
        return img
    return mixed_raster(w, h, c.bands, c.dtype, 100 + seed, c.cf)


BY_ID = {c.id: c for c in MATRIX + BIG}
assert len(BY_ID) == len(MATRIX) + len(BIG)


def raster(c, seed=0):
    return _raster(c.id, seed)


_truth = {}


def truth(oracle, c, seed=0):
    """(Units, entering values) of a case's raster: made once, shared, left unchanged"""
    key = (c.id, seed)
    if key not in _truth:
        img = raster(c, seed)
        _truth[key] = (T.units(oracle, img, c.dtype, c.mode, c.cband), T.entering_values(img, c.dtype, c.cband, T.curve_order(c.mode)))
    return _truth[key]


_built = {}


def built(oracle, c, level, seed=0):
    key = (c.id, level, seed)
    if key not in _built:
        u, ev = truth(oracle, c, seed)
        _built[key] = T.build(u, ev, c.dtype, c.mode, level)
    return _built[key]


def oracle_container(oracle, c, seed=0):
    return oracle.encode(raster(c, seed), c.dtype, c.mode, cband=c.cband)


def with_table(ref, table):
    """the oracle's container with the table's chunks in front of its "DT" """
    ref = bytes(ref)
    at = ref.index(b"DT", 11)
    return ref[:at] + table + ref[at + 2:]


ids = lambda c: c.id      # noqa: E731

# ------------------------------------------------------------------------------------------------------------------- CPU: the truth


@pytest.mark.parametrize("c", MATRIX, ids=ids)
def test_parse_inverts_build(oracle, c):
    for level in (1, 2):
        want_bytes, want = built(oracle, c, level)
        got, t0, t1 = T.parse(with_table(oracle_container(oracle, c), want_bytes))
        assert T.explain(got, want) is None, T.explain(got, want)
        assert got.heads == want.heads and t1 - t0 == len(want_bytes)
        assert T.assemble(got) == want_bytes
        for (ln, ver, flags, chk, blocks), body in zip(got.heads, got.bodies):
            assert ver == 3 and ln == 12 + len(body) <= 65535 and chk == T.chunk_check(body)


def test_layouts_as_the_header_words_them():
    """every sentence of qb3x.h's table that gives a number"""
    L = T.layout
    assert L(U8, 3, FTL, 1) == dict(blocks=64, entry_bytes=12, kind=T.NONE, flags=0, fields=0, fixed=12, bands=3, tsz=1)
    assert L(U8, 3, FTL, 2)["entry_bytes"] == 12 + 80 and L(U8, 3, BASE, 2)["flags"] == 2
    assert [L(U16, b, FTL, 2)["blocks"] for b in (1, 2, 3, 4, 6, 8)] == [64, 64, 64, 64, 21, 32]
    assert L(U16, 1, FTL, 2)["entry_bytes"] == 9 + 80 and L(I16, 4, BASE, 2)["entry_bytes"] == 18 + 160
    assert [(L(U16, b, FTL, 2)["blocks"], L(U16, b, FTL, 2)["flags"]) for b in (10, 12, 14, 16)] == [(12, 0), (21, 0), (9, 0), (16, 0)]
    assert L(U32, 1, FTL, 2)["entry_bytes"] == 6 + 5 + 96 and L(I64, 1, FTL, 2)["blocks"] == 64
    assert L(U8, 5, FTL, 2) == dict(blocks=12, entry_bytes=6 + 10 + 90, kind=T.UNIT12, flags=2, fields=60, fixed=16, bands=5, tsz=1)
    assert L(U16, 7, BASE, 2)["entry_bytes"] == 6 + 21 + (63 * 12 + 7) // 8
    for level in (1, 2):
        assert L(U8, 3, CF_H, level)["entry_bytes"] == 6 + 3 * 3 + 192 and L(U8, 3, BEST, level)["flags"] == 3
        assert L(I64, 1, CF_H, level)["entry_bytes"] == 7 + 16 + 192
        assert L(U16, 8, CF_H, level)["entry_bytes"] == 6 + 8 * 5 + 3 * 8 * 8 and L(U16, 8, CF_H, level)["blocks"] == 8
        assert L(U8, 5, CF, level)["entry_bytes"] == 6 + 5 * 3 + 3 * 12 * 5


@pytest.mark.parametrize("c", [c for c in MATRIX + BIG if not c.cf], ids=ids)
def test_entries_decode_the_stream(oracle, c):
    """from every entry's position, with the entry's rungs and entering values, the first block's pixels come out of the stream"""
    u, ev = truth(oracle, c)
    _, t = built(oracle, c, 1)
    img = raster(c)
    h, w, b = img.shape
    tsz = T.TYPESIZE[c.dtype]
    bits, mask = 8 * tsz, (1 << 8 * tsz) - 1
    cb = T.band_map(b, c.cband)
    order = T.curve_order(c.mode)
    nbx = (w + 3) // 4
    px = img.view(T.UNSIGNED[c.dtype]).astype(object)
    for k in range(len(t.pos)):
        blk = k * t.lay["blocks"]
        x0, y0 = min(4 * (blk % nbx), w - 4), min(4 * (blk // nbx), h - 4)
        at = int(t.pos[k])
        end = int(u.start[blk + 1, 0]) if blk + 1 < u.nblocks else u.nbits
        stream, pos = (u.stream >> at) & ((1 << (end - at + 128)) - 1), 0       # (the block's bits and a few more: short integers)
        for band in range(b):
            if stream >> pos & 1:
                delta, sig, ln = S.decode_switch_noflag(stream, pos + 1, S.UB[tsz])
                assert not sig
                pos += 1 + ln
            else:
                delta, pos = 0, pos + 1
            r = (int(t.rungs[k, band]) + delta) % (1 << S.UB[tsz])
            g, pos = S.decode_group(stream, pos, r, tsz, c.mode != FTL)
            v = int(t.prev[k, band])
            for i, m in enumerate(g):
                v = (v + S.smag(m, bits)) & mask
                nib = (order >> (60 - 4 * i)) & 15
                p = px[y0 + (nib >> 2), x0 + (nib & 3)]
                want = p[band] if cb[band] == band else (p[band] - p[cb[band]]) & mask
                assert v == want, "entry %d, band %d, value %d of block %d" % (k, band, i, blk)
        assert at + pos == end


@pytest.mark.parametrize("c", MATRIX + BIG, ids=ids)
def test_the_truth_adds_up(oracle, c):
    """lengths sum to the stream; the entering values of a block behind the last are the oracle's band state, as are the rungs and
    factors the trace ends with; the oracle's container is coded and its stream is the traced one"""
    u, ev = truth(oracle, c)
    assert int(u.length.sum()) == u.nbits and (u.length > 0).all()
    assert [int(v) for v in ev[-1]] == [s[0] for s in u.state]
    assert [int(v) for v in u.rung[-1]] == [s[1] for s in u.state]
    assert [int(v) for v in u.factor_after] == [s[2] for s in u.state]
    ref = bytes(oracle_container(oracle, c))
    assert ref[10] != 255, "coded, not stored"
    if c.kind == "const":
        assert ref[10] == 7, "the RLE0 pass won"
    else:
        assert ref[10] == (5 if c.mode == BEST else c.mode)
        data = ref[ref.index(b"DT", 11) + 2:]
        assert len(data) == (u.nbits + 7) // 8 and int.from_bytes(data, "little") == u.stream


@pytest.mark.parametrize("c", [c for c in MATRIX + BIG if c.kind != "const"], ids=ids)
def test_rasters_exercise_their_case(oracle, c):
    u, _ = truth(oracle, c)
    tsz = T.TYPESIZE[c.dtype]
    bits = 8 * tsz
    lay = T.layout(c.dtype, c.bands, c.mode, 2)
    K = (u.nblocks + lay["blocks"] - 1) // lay["blocks"]
    assert K >= 2 and (u.nblocks % lay["blocks"] or c.shape == (64, 64)), "several entries, a partial last one"
    if c.cf:
        kinds = set(u.kind.ravel())
        assert {"C", "I"} <= kinds, kinds
        cfu = u.kind == "C"
        own = u.factor - np.uint64(2) != u.factor_before
        assert (cfu & own).any() and (cfu & ~own).any(), "factors of their own and kept factors"
        assert u.length.max() < 800
        if tsz == 1 and c.bands in (1, 3, 4):
            assert u.rung_in.max() == 7
    elif tsz >= 2:
        assert (u.rung < 8).any() and (u.rung > 8).any(), "both sides of the table / arithmetic split of the codes"
    if c.kind == "units" and not c.cf:
        assert u.rung.max() == bits - 1
        ub = S.UB[tsz]
        assert u.length.max() >= 16 * (bits + 1) - (2 if c.mode == BASE else 0) + 1, "the longest unit: sixteen longest codes"
        assert u.length.max() <= 16 * (bits + 1) + ub + 2
        if tsz == 8:
            assert u.length.max() > 1023, "ten bits would not do"
    if c.kind == "patch":
        if tsz == 1:
            assert u.length.sum(1).max() > 511
        else:
            assert (u.length[:, 0] + u.length[:, 1]).max() > 511 and (u.length[:, 2] + u.length[:, 3]).max() > 511
        assert u.length.sum(1).min() == 2 * c.bands, "and flat blocks of two bits a band"


def test_a_wrong_field_is_named(oracle):
    """what a failure says"""
    c = next(c for c in MATRIX if c.cls == "B" and c.bands == 4)
    want_bytes, want = built(oracle, c, 2)
    bad = bytearray(with_table(oracle_container(oracle, c), want_bytes))
    t0, _ = T.table_span(bad)
    e = t0 + 12 + 2 * want.lay["entry_bytes"] + want.lay["fixed"]
    f = int(want.fields[2, 0])
    bad[e] = (f + 1) & 255
    got, _, _ = T.parse(bad)
    assert T.explain(got, want) == "entry 2, field 0 (block 128, bands 0-1): %d != %d" % ((f & ~255) | ((f + 1) & 255), f)
    assert T.explain(got, want) is not None and got.heads == want.heads


# ------------------------------------------------------------------------------------------------------------------- GPU

GUARD = 64


def device_encode(qb3, c, img, level, want_index, fill):
    """qb3x_encode_device into a destination of qb3_max_encoded_size + 64 bytes filled with `fill`: the container's bytes; the guard
    must be untouched"""
    import torch
    from qb3_amd import device as qdev
    h, w, b = img.shape
    enc = qdev.DeviceEncoder(w, h, b, c.dtype, mode=c.mode, cband=c.cband, want_index=want_index, index_chunk=level)
    room = (enc.max_size + 3) // 4 * 4
    dst = torch.full((room + GUARD,), fill, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(img.view(np.uint8).reshape(-1).copy()).cuda()
    _, n, _ = enc.encode(src, dst=dst)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    enc.close()
    assert n <= enc.max_size and (host[room:] == fill).all(), "bytes behind the destination were written"
    return host[:n].tobytes()


def check(oracle, c, container, level, seed=0, what="the device call"):
    """the container's table is the spec's, and minus its table the container is the oracle's"""
    want_bytes, want = built(oracle, c, level, seed)
    try:
        t0, t1 = T.compare(container, want_bytes, want, c.dtype, c.mode)
    except AssertionError as e:
        raise AssertionError("%s, level %d: %s" % (what, level, e)) from None
    assert bytes(container) == with_table(oracle_container(oracle, c, seed), want_bytes), "%s: minus its table, the oracle's container" % what
    return T.parse(container)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("c", MATRIX + BIG, ids=ids)
def test_encoder_writes_the_table(qb3, oracle, c, level):
    img = raster(c)
    runs = [device_encode(qb3, c, img, level, wi, fill) for fill in (0x00, 0xA5) for wi in (True, False)]
    got = check(oracle, c, runs[0], level)
    for i, r in enumerate(runs[1:]):
        assert r == runs[0], "the container depends on %s" % ("the index being asked for", "what the destination held", "both")[i]
    lay = got.lay
    if c.cls == "B" and level == 2:
        assert (got.fields is not None) == (c.bands <= 8), "length fields up to eight bands, none above"
    if c.cls == "D":
        assert got.heads[0][4] == 64 // c.bands and (level == 1 or lay["kind"] == T.UNIT12)
    if c.cls in ("A", "C") and level == 2:
        assert lay["kind"] == (T.BLOCK10 if c.cls == "A" else T.UNIT12)
    if c in BIG:
        assert len(got.heads) == (2 if level == 2 or c.cls == "E" else 1), "more than one chunk"


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in MATRIX if c.cls == "E"] + BIG[1:], ids=ids)
def test_block_field_tables_do_not_depend_on_the_level(qb3, oracle, c):
    """8-bit common-factor streams: the same table at level 1 and 2, three bits of entering rung a band"""
    img = raster(c)
    one, two = (device_encode(qb3, c, img, level, False, 0xA5) for level in (1, 2))
    assert one == two
    got = check(oracle, c, one, 1)
    assert got.lay["kind"] == T.BLOCK24_R3 and got.heads[0][2] == 3 and (got.fields >> (12 + 3 * c.bands)).max() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("c", list(FIRST_OF_CLASS.values()), ids=ids)
def test_host_call_writes_the_table(qb3, oracle, c, level):
    """qb3_encode on host pointers"""
    got = qb3.encode(raster(c), c.dtype, c.mode, cband=c.cband, index_chunk=level)
    check(oracle, c, got.tobytes(), level, what="qb3_encode")


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("c", list(FIRST_OF_CLASS.values()), ids=ids)
def test_tile_batch_writes_the_table(qb3, oracle, c, level):
    """qb3x_encode_tiles, three tiles: every container its own table"""
    import torch
    from qb3_amd import device as qdev
    n = 3 if c.kind == "mixed" else 1           # (the one-raster kinds: the same tile three times)
    imgs = [raster(c, s % n) for s in range(3)]
    h, w, b = imgs[0].shape
    tc = qdev.TileBatchCoder(w, h, b, c.dtype, 3, mode=c.mode, want_index=False, index_chunk=level)
    if c.cband is not None:
        assert qb3.lib.qb3_set_encoder_coreband(tc.p, b, (qdev._sz * b)(*c.cband))
    tc.dst.fill_(0xA5)
    tc.encode(torch.from_numpy(np.stack(imgs).view(np.uint8).reshape(-1).copy()).cuda())
    host = tc.dst.cpu().numpy()
    for t in range(3):
        check(oracle, c, host[t * tc.pitch:t * tc.pitch + tc.sizes[t]].tobytes(), level, seed=t % n, what="tile %d" % t)
    tc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("c", list(FIRST_OF_CLASS.values()) + BIG, ids=ids)
def test_reindex_writes_the_table(qb3, oracle, c, level):
    """qb3x_reindex_device of the oracle's container (no table): the table of the walk's index is the spec's"""
    import torch
    from qb3_amd import device as qdev
    ref = np.ascontiguousarray(oracle_container(oracle, c))
    d_src = torch.zeros((len(ref) + 3) // 4 * 4 + 16, dtype=torch.uint8, device="cuda")
    d_src[:len(ref)] = torch.from_numpy(ref)
    dec = qdev.DeviceDecoder(ref, len(ref))
    cap = qb3.lib.qb3x_reindex_size(dec.p, level)
    assert cap
    room = (cap + 3) // 4 * 4
    out = torch.full((room + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n = qb3.lib.qb3x_reindex_device(dec.p, d_src.data_ptr(), out.data_ptr(), cap, level, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    dec.close()
    assert n and (host[room:] == 0xA5).all()
    check(oracle, c, host[:n].tobytes(), level, what="reindex")
