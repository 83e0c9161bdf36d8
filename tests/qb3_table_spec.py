"""tests/qb3_table_spec.py -- the restart table ("ix" / "zz" chunks in front of "DT") as include/qb3x.h words it, in plain numpy and
Python integers (test infrastructure: no GPU, no call into the library, nothing taken from the code that fills the table).

The truth about the stream comes from the CPU oracle's unit trace (qb3o_set_trace: a row per unit with its start bit, kind, the rung
its band is left at, its factor, the factor in force before it) and from the pixels (the values entering each block); the layout of
the bytes is written out from the sentences of qb3x.h ("Self-indexing containers").  tests/test_table_spec.py holds this module to
account before anything is compared with it: its positions, rungs and entering values decode the stream, its lengths add up.

Not modelled: quantised rasters (the entering values would be those of the quantised pixels), narrow images and STORED containers
(no table), tables of versions 1 and 2 (read, never written).
"""
import numpy as np

TYPESIZE = (1, 1, 2, 2, 4, 4, 8, 8)
UNSIGNED = (np.uint8, np.uint8, np.uint16, np.uint16, np.uint32, np.uint32, np.uint64, np.uint64)
HILBERT = 0x01548CD9AEFB7623
ZCURVE = 0x0145236789CDABEF
PLAIN_MODES = (0, 4, 8)         # QB3M_BASE_Z, QB3M_BASE_H, QB3M_FTL: every other mode's block stream is a common-factor one
IX_HEAD, IX_PAD = 12, 4
CHUNK_MAX = 65535

# field kinds: what an entry ends with
NONE = "none"                   # nothing
BLOCK10 = "block10"             # ten bits a block: its bit length
PAIR10 = "pair10"               # 16-bit rasters of several bands: two ten-bit fields a lane of the decoder's wave
UNIT12 = "unit12"               # twelve bits a unit (band-minor): its bit length
BLOCK24_R3 = "block24r3"        # three bytes a block: bits (12) | the rung each band's unit is entered with (3 bits a band) << 12
BLOCK24_R6 = "block24r6"        # three bytes a block of one band: bits (12) | the rung it is entered with << 12
UNIT24 = "unit24"               # three bytes a unit (band-minor): bits (12) | the rung it is entered with << 12
FIELD_BITS = {BLOCK10: 10, PAIR10: 10, UNIT12: 12, BLOCK24_R3: 24, BLOCK24_R6: 24, UNIT24: 24}


# ---------------------------------------------------------------------------------------------------------------- the stream's truth

def band_map(bands, cband=None):
    """the band map an encoder handle ends up with: R-G, G, B-G (, A) by default for 3 and 4 bands, identity otherwise; an explicit
    map makes every band that is subtracted a core band (reference QB3encode.cpp:70-72)"""
    if cband is None:
        cb = list(range(bands))
        if bands in (3, 4):
            cb[0] = cb[2] = 1
        return cb
    cb = [c if c < bands else i for i, c in enumerate(cband)]
    for i in range(bands):
        if cb[i] != i:
            cb[cb[i]] = cb[i]
    return cb


def curve_order(mode):
    """the scan order of a mode: the Z curve for the legacy modes 0..3, Hilbert's from QB3M_BASE_H on"""
    return ZCURVE if mode <= 3 else HILBERT


class Units:
    """the oracle's trace as arrays [block, band]: start (bit, from the stream's first), length, kind ('N' plain, '0' rung 0, 'C'
    common factor, 'I' index), rung (the band is left at), rung_in (entered with), factor (the unit's own: 0 where it has none),
    factor_before (the band-state value in force before the unit: the factor minus 2, 0 before the band's first); nbits: the stream"""


KINDS = np.array(["0", "N", "C", "I"])
_KIND_DIGIT = bytes.maketrans(b"NCI", b"123")


def _raw_trace(oracle, img, dtype, mode, cband, fix_b2=False, encoder=None):
    """(stream int, bits, rows [n, 5] of uint64, band state) of the oracle's raw encode under its trace; a row: start bit, kind (index
    into KINDS), rung the band is left at, the unit's factor, the band-state factor before it.  encoder: an oracle.Encoder of the
    raster's shape to encode with as it stands (its mode, band map and band state), not a fresh one"""
    import ctypes as C
    import tempfile
    lib = oracle.lib
    lib.qb3o_set_trace.argtypes, lib.qb3o_set_trace.restype = [C.c_char_p], None
    h, w, b = img.shape
    e = encoder or oracle.Encoder(w, h, b, dtype)
    if encoder is None:
        e.set_mode(mode)
        if cband is not None:
            e.set_coreband(cband)
        if fix_b2:                  # (keep the units the reference drops, SURVEY B-2: for a generator that looks for them)
            lib.qb3o_set_fix_b2(e.p, 1)
    dst = np.zeros(e.max_size() + 64, dtype=np.uint8)
    src = np.ascontiguousarray(img)
    with tempfile.NamedTemporaryFile("rb", suffix=".txt") as f:
        lib.qb3o_set_trace(f.name.encode())
        try:
            nbits = lib.qb3o_encode_raw(e.p, oracle._p(src), oracle._p(dst))
        finally:
            lib.qb3o_set_trace(None)
        text = f.read()
    assert nbits, "oracle raw encode failed"
    # (the kind is the second word of a line: a letter, or the digit 0 -- no other word holds a letter)
    rows = np.fromstring(text.translate(_KIND_DIGIT), dtype=np.uint64, sep=" ").reshape(-1, 5)     # (exact up to 2^64 - 1)
    stream = int.from_bytes(dst[:(nbits + 7) // 8].tobytes(), "little") & ((1 << nbits) - 1)
    return stream, nbits, rows, e.band_state()


def oracle_units(oracle, img, dtype, mode):
    """(stream int, bits, trace rows) of the oracle's raw unit stream of a 4n x 4 x 1 raster; a trace row: start bit, kind (N plain,
    0 rung 0, C common factor, I index), rung of the deltas, factor, factor before"""
    bits, n, rows, _ = _raw_trace(oracle, img.reshape(img.shape[0], img.shape[1], 1), dtype, mode, None)
    return bits, n, [(int(a), str(KINDS[int(k)]), int(r), int(c), int(p)) for a, k, r, c, p in rows]


def units(oracle, img, dtype, mode, cband=None):
    """the Units of img (h, w, bands) under mode and band map, from the oracle's trace of its raw encode; .stream: the stream as an
    int (bit i is stream bit i), .state: the oracle's band state (value, rung, factor) behind the last block"""
    h, w, b = img.shape
    stream, nbits, rows, state = _raw_trace(oracle, img, dtype, mode, cband)
    nblocks = ((w + 3) // 4) * ((h + 3) // 4)
    assert len(rows) == nblocks * b, "a row a unit (none dropped: SURVEY B-2): %d rows, %d units" % (len(rows), nblocks * b)
    first = int(rows[0, 0])
    u = Units()
    start = rows[:, 0].astype(np.int64) - first
    u.nbits = int(nbits) - first
    u.length = np.diff(np.append(start, u.nbits)).reshape(nblocks, b)
    u.start = start.reshape(nblocks, b)
    kind = rows[:, 1].astype(np.int64).reshape(nblocks, b)
    u.kind = KINDS[kind]
    u.rung = rows[:, 2].astype(np.int64).reshape(nblocks, b)
    u.rung_in = np.vstack([np.zeros((1, b), np.int64), u.rung[:-1]])
    is_c = kind == 2
    u.factor = np.where(is_c, rows[:, 3].reshape(nblocks, b), np.uint64(0))
    # the factor in force: what the band's last common-factor unit left, its factor minus 2 (the trace's own column says the same
    # wherever the oracle looked at it, which it does not for rung-0 units)
    lastc = np.maximum.accumulate(np.where(is_c, np.arange(nblocks)[:, None], -1), axis=0)
    after = np.where(lastc >= 0, (u.factor - np.uint64(2))[np.maximum(lastc, 0), np.arange(b)[None, :]], np.uint64(0))
    u.factor_before = np.vstack([np.zeros((1, b), np.uint64), after[:-1]])
    u.factor_after = after[-1]
    looked = (kind >= 2) | ((kind == 1) & (mode not in PLAIN_MODES))
    assert np.array_equal(rows[:, 4].reshape(nblocks, b)[looked], u.factor_before[looked])
    u.stream, u.state, u.nblocks, u.bands = stream, state, nblocks, b
    return u


def entering_values(img, dtype, cband=None, order=HILBERT):
    """[block, band] for blocks 0 .. nblocks (one behind the last): the value entering each band -- the band-differenced value (the
    band map's, modulo the type's width, as an unsigned number) of the pixel the curve visits last in the block before; 0 for block
    0.  The last block column / row is shifted, not padded."""
    h, w, b = img.shape
    cb = band_map(b, cband)
    u = np.ascontiguousarray(img).view(UNSIGNED[dtype]).reshape(h, w, b)
    v = u.copy()
    for c in range(b):
        if cb[c] != c:
            v[..., c] = u[..., c] - u[..., cb[c]]       # unsigned arithmetic wraps to the type's width
    last = order & 15
    nbx, nby = (w + 3) // 4, (h + 3) // 4
    x = np.minimum(4 * np.arange(nbx), w - 4) + (last & 3)
    y = np.minimum(4 * np.arange(nby), h - 4) + (last >> 2)
    out = np.zeros((nbx * nby + 1, b), dtype=np.uint64)
    out[1:] = v[y[:, None], x[None, :]].reshape(nbx * nby, b)
    return out


# ---------------------------------------------------------------------------------------------------------------- the layout

def lanes_per_block16(bands):
    """16-bit FTL / BASE rasters of the lane-per-block decoder: (bands a lane owns, lanes a block) -- a lane owns up to four bands:
    all of them up to four, four where the count is a multiple of four, two where it is even; None: odd counts above four"""
    bg = bands if bands <= 4 else 4 if bands % 4 == 0 else 2 if bands % 2 == 0 else 0
    return (bg, bands // bg) if bg else None


def layout(dtype, bands, mode, level):
    """what qb3x.h says of the table of a raster: blocks an entry, bytes an entry, the kind of its fields, the head's flags, fields
    an entry, bytes of an entry's fixed part"""
    tsz, cf = TYPESIZE[dtype], mode not in PLAIN_MODES
    fixed = 6 + bands * (1 + tsz * (2 if cf else 1))
    if cf:
        # at EITHER level: a field per block for 8-bit rasters of 1 / 3 / 4 bands and for one band of 16/32/64 bits, a field per unit
        # for every other raster; no common-factor table is written without fields
        if tsz == 1 and bands in (1, 3, 4):
            blocks, kind, nf = 64, BLOCK24_R3, 64
        elif bands == 1:
            blocks, kind, nf = 64, BLOCK24_R6, 64
        else:
            blocks, kind = 64 // bands, UNIT24
            nf = blocks * bands
    else:
        kind = NONE
        if tsz == 1 and bands in (1, 3, 4):
            blocks, k2, nf = 64, BLOCK10, 64
        elif tsz == 2 and lanes_per_block16(bands):
            bg, ng = lanes_per_block16(bands)
            blocks = 64 // ng
            # length fields up to eight bands; the even counts above (10, 12, 14, 16) have the segments and no fields at any level
            k2, nf = (BLOCK10, 64) if bands == 1 else (PAIR10, 128) if bands <= 8 else (NONE, 0)
        elif tsz >= 4 and bands == 1:
            blocks, k2, nf = 64, UNIT12, 64
        else:                       # the lane-per-unit rasters
            blocks, k2 = 64 // bands, UNIT12
            nf = blocks * bands
        if level >= 2:
            kind = k2
    if kind == NONE:
        nf = 0
    E = fixed + ((nf * FIELD_BITS[kind] + 7) // 8 if nf else 0)
    return dict(blocks=blocks, entry_bytes=E, kind=kind, flags=(1 if cf else 0) | (2 if nf else 0), fields=nf, fixed=fixed,
                bands=bands, tsz=tsz)


def field_where(lay, k, f):
    """the words for field f of entry k"""
    B, blocks, kind = lay["bands"], lay["blocks"], lay["kind"]
    if kind in (BLOCK10, BLOCK24_R3, BLOCK24_R6):
        return "block %d" % (k * blocks + f)
    if kind in (UNIT12, UNIT24):
        return "block %d, band %d" % (k * blocks + f // B, f % B)
    bg, ng = lanes_per_block16(B)
    lane, pair = divmod(f, 2)
    slot, g = divmod(lane, ng)
    if slot >= blocks:
        return "no block: lane %d" % lane
    lo = bg * g + (pair if bg == 2 else 2 * pair)
    n = 1 if bg == 2 or (bg == 3 and pair) else 2
    return "block %d, band%s" % (k * blocks + slot, " %d" % lo if n == 1 else "s %d-%d" % (lo, lo + 1))


def fields_of(lay, u):
    """[entry, field] from the Units: zeros behind the raster's last block or unit"""
    B, blocks, kind, nf = lay["bands"], lay["blocks"], lay["kind"], lay["fields"]
    K = (u.nblocks + blocks - 1) // blocks
    if kind == NONE:
        return None
    ln = np.zeros((K * blocks, B), dtype=np.int64)
    rg = np.zeros((K * blocks, B), dtype=np.int64)
    ln[:u.nblocks], rg[:u.nblocks] = u.length, u.rung_in
    if kind == BLOCK10:
        f = ln.sum(1)
    elif kind == UNIT12:
        f = ln
    elif kind == UNIT24:
        f = ln | rg << 12
    elif kind == BLOCK24_R6:
        f = ln[:, 0] | rg[:, 0] << 12
    elif kind == BLOCK24_R3:
        f = ln.sum(1)
        for c in range(B):
            assert rg[:, c].max() < 8
            f = f | rg[:, c] << (12 + 3 * c)
    else:                           # PAIR10: lane = block of the segment x band group; two fields a lane
        bg, ng = lanes_per_block16(B)
        g = ln.reshape(K, blocks, ng, bg)
        if bg == 2:
            pairs = g
        elif bg == 3:
            pairs = np.stack([g[..., 0] + g[..., 1], g[..., 2]], axis=-1)
        else:
            pairs = np.stack([g[..., 0] + g[..., 1], g[..., 2] + g[..., 3]], axis=-1)
        f = np.zeros((K, nf), dtype=np.int64)
        f[:, :blocks * ng * 2] = pairs.reshape(K, -1)
        return f
    f = f.reshape(K, nf)
    assert f.max() < 1 << FIELD_BITS[kind]
    return f


# ---------------------------------------------------------------------------------------------------------------- bytes

def chunk_check(body):
    """the 16-bit check of a chunk's entry bytes b[i]: the sum of (b[i] + 1) * (i * 0x9e3779b1 + 1) modulo 2^32, low half XOR high half"""
    b = np.frombuffer(bytes(body), dtype=np.uint8).astype(np.uint64)
    i = np.arange(len(b), dtype=np.uint64)
    mult = (i * np.uint64(0x9E3779B1) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    s = int((((b + np.uint64(1)) * mult) & np.uint64(0xFFFFFFFF)).sum() & np.uint64(0xFFFFFFFF))
    return (s ^ (s >> 16)) & 0xFFFF


def _le_bytes(a, n):
    """[..., n] little-endian bytes of the unsigned numbers a"""
    a = np.asarray(a, dtype=np.uint64)
    return ((a[..., None] >> (np.uint64(8) * np.arange(n, dtype=np.uint64))) & np.uint64(255)).astype(np.uint8)


def _from_le(b):
    b = np.asarray(b, dtype=np.uint64)
    return (b << (np.uint64(8) * np.arange(b.shape[-1], dtype=np.uint64))).sum(-1, dtype=np.uint64)


def pack_fields(f, width):
    """[entry, bytes]: the fields of an entry as one little-endian bit string, to whole bytes"""
    K, nf = f.shape
    bits = ((f[..., None] >> np.arange(width)) & 1).astype(np.uint8).reshape(K, nf * width)
    pad = -bits.shape[1] % 8
    if pad:
        bits = np.concatenate([bits, np.zeros((K, pad), np.uint8)], axis=1)
    return np.packbits(bits, axis=1, bitorder="little")


def unpack_fields(b, nf, width):
    bits = np.unpackbits(np.asarray(b, dtype=np.uint8), axis=1, bitorder="little").astype(np.int64)
    tail = bits[:, nf * width:]
    return (bits[:, :nf * width].reshape(-1, nf, width) << np.arange(width)).sum(-1), tail


class Table:
    """a table in parts: lay (layout), heads [(length, version, flags, check, blocks)], pos [K], rungs / prev / cf [K, bands] (cf:
    None without flag bit 0), fields [K, F] or None, slack [K, n]: the bits of an entry's last byte behind its last field"""


def make(u, entering, dtype, mode, level):
    """the Table of a raster from its Units and entering values [nblocks + 1, bands]"""
    lay = layout(dtype, u.bands, mode, level)
    t = Table()
    t.lay = lay
    first = np.arange(0, u.nblocks, lay["blocks"])
    t.pos = u.start[first, 0].astype(np.uint64)
    t.rungs = u.rung_in[first].astype(np.uint8)
    t.prev = entering[first].astype(np.uint64)
    t.cf = u.factor_before[first].astype(np.uint64) if lay["flags"] & 1 else None
    t.fields = fields_of(lay, u)
    nb = lay["entry_bytes"] - lay["fixed"]
    t.slack = np.zeros((len(first), 8 * nb - lay["fields"] * FIELD_BITS[lay["kind"]]), np.int64) if lay["fields"] else None
    t.heads = None
    return t


def entry_bytes(t):
    lay = t.lay
    K, B, tsz = len(t.pos), lay["bands"], lay["tsz"]
    parts = [_le_bytes(t.pos, 6), t.rungs, _le_bytes(t.prev, tsz).reshape(K, B * tsz)]
    if t.cf is not None:
        parts.append(_le_bytes(t.cf, tsz).reshape(K, B * tsz))
    if t.fields is not None:
        parts.append(pack_fields(t.fields, FIELD_BITS[lay["kind"]]))
    e = np.concatenate(parts, axis=1)
    assert e.shape[1] == lay["entry_bytes"], (e.shape, lay)
    return e


def assemble(t):
    """the chunks of a Table, "DT" behind the last pad; fills t.heads"""
    lay = t.lay
    e = entry_bytes(t)
    E = lay["entry_bytes"]
    per_chunk = (CHUNK_MAX - IX_HEAD) // E
    out, t.heads = [], []
    for c0 in range(0, len(e), per_chunk):
        body = e[c0:c0 + per_chunk].tobytes()
        ln, chk = IX_HEAD + len(body), chunk_check(body)
        t.heads.append((ln, 3, lay["flags"], chk, lay["blocks"]))
        out.append(b"ix" + ln.to_bytes(2, "little") + bytes([3, lay["flags"]]) + chk.to_bytes(2, "little") + lay["blocks"].to_bytes(4, "little")
                   + body + b"zz" + IX_PAD.to_bytes(2, "little"))
    return b"".join(out) + b"DT"


def build(u, entering, dtype, mode, level):
    """(bytes, Table): the whole run of chunks with "DT" at the end"""
    t = make(u, entering, dtype, mode, level)
    return assemble(t), t


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
            assert t0 is None, "the table stands directly in front of DT"
            pos += 4 + ln
        else:
            raise AssertionError("unexpected chunk %r at %d" % (sig, pos))
    raise AssertionError("no DT")


def parse(container, dtype=None, bands=None, mode=None):
    """(Table, start, end) of a container's table; the layout is the one the heads' flags name (fields: the raster's level-2 layout)
    for the type, band count and mode of the container's header"""
    c = bytes(container)
    assert c[:4] == b"QB3\x80"
    dtype, bands, mode = c[9] if dtype is None else dtype, c[8] + 1 if bands is None else bands, c[10] if mode is None else mode
    t0, t1 = table_span(c)
    pos, heads, bodies = t0, [], []
    while c[pos:pos + 2] == b"ix":
        ln = c[pos + 2] | c[pos + 3] << 8
        heads.append((ln, c[pos + 4], c[pos + 5], c[pos + 6] | c[pos + 7] << 8, int.from_bytes(c[pos + 8:pos + 12], "little")))
        bodies.append(c[pos + IX_HEAD:pos + ln])
        pos += ln
        assert c[pos:pos + 4] == b"zz" + IX_PAD.to_bytes(2, "little"), "a pad chunk behind every ix chunk (at %d)" % pos
        pos += IX_PAD
    assert c[pos:pos + 2] == b"DT" and pos + 2 == t1
    flags = heads[0][2]
    lay = layout(dtype, bands, mode, 2 if flags & 2 else 1)
    assert (flags & 1) == (lay["flags"] & 1), "flag bit 0 %d for mode %d" % (flags & 1, mode)
    E, B, tsz = lay["entry_bytes"], bands, lay["tsz"]
    for i, bd in enumerate(bodies):
        assert len(bd) % E == 0, "chunk %d: %d bytes are no whole entries of %d" % (i, len(bd), E)
    e = np.frombuffer(b"".join(bodies), dtype=np.uint8).reshape(-1, E)
    K = len(e)
    t = Table()
    t.lay, t.heads, t.bodies = lay, heads, bodies
    t.pos = _from_le(e[:, :6])
    t.rungs = e[:, 6:6 + B].copy()
    o = 6 + B
    t.prev = _from_le(e[:, o:o + B * tsz].reshape(K, B, tsz))
    o += B * tsz
    t.cf = None
    if flags & 1:
        t.cf = _from_le(e[:, o:o + B * tsz].reshape(K, B, tsz))
        o += B * tsz
    assert o == lay["fixed"]
    t.fields = t.slack = None
    if lay["fields"]:
        t.fields, t.slack = unpack_fields(e[:, o:], lay["fields"], FIELD_BITS[lay["kind"]])
    return t, t0, t1


def explain(got, want):
    """None where two Tables agree, else the first difference in words"""
    if got.lay != want.lay:
        return "layout: %r != %r" % (got.lay, want.lay)
    lay = want.lay
    if len(got.pos) != len(want.pos):
        return "%d entries != %d" % (len(got.pos), len(want.pos))
    for name in ("pos", "rungs", "prev", "cf", "fields", "slack"):
        a, b = getattr(got, name), getattr(want, name)
        if (a is None) != (b is None):
            return "%s: %s != %s" % (name, "absent" if a is None else "present", "absent" if b is None else "present")
        if a is None or np.array_equal(a, b):
            continue
        a, b = np.asarray(a).reshape(len(want.pos), -1), np.asarray(b).reshape(len(want.pos), -1)
        k, j = [int(x) for x in np.argwhere(a != b)[0]]
        blk = k * lay["blocks"]
        if name == "pos":
            return "entry %d (block %d), position: %d != %d" % (k, blk, a[k, j], b[k, j])
        if name == "fields":
            msg = "entry %d, field %d (%s): %d != %d" % (k, j, field_where(lay, k, j), a[k, j], b[k, j])
            if lay["kind"] in (BLOCK24_R3, BLOCK24_R6, UNIT24):
                msg += " (bits %d != %d, rungs %#o != %#o)" % (a[k, j] & 4095, b[k, j] & 4095, a[k, j] >> 12, b[k, j] >> 12)
            return msg
        if name == "slack":
            return "entry %d, bit %d behind its last field is set" % (k, j)
        what = {"rungs": "rung", "prev": "entering value", "cf": "factor"}[name]
        return "entry %d (block %d), %s of band %d: %d != %d" % (k, blk, what, j, a[k, j], b[k, j])
    if got.heads != want.heads:
        i = next(i for i in range(max(len(got.heads), len(want.heads)))
                 if i >= len(got.heads) or i >= len(want.heads) or got.heads[i] != want.heads[i])
        names = ("length", "version", "flags", "check", "blocks per entry")
        if i >= len(got.heads) or i >= len(want.heads):
            return "%d chunks != %d" % (len(got.heads), len(want.heads))
        j = next(j for j in range(5) if got.heads[i][j] != want.heads[i][j])
        return "chunk %d, %s: %d != %d" % (i, names[j], got.heads[i][j], want.heads[i][j])
    return None


def compare(container, want_bytes, want, dtype, mode):
    """assert that a container's table is want_bytes, saying which part is not"""
    got, t0, t1 = parse(container, dtype, want.lay["bands"], mode)
    msg = explain(got, want)
    assert msg is None, msg
    have = bytes(container[t0:t1])
    assert have == want_bytes, "table byte %d differs" % next(i for i in range(min(len(have), len(want_bytes))) if have[i] != want_bytes[i])
    return t0, t1
