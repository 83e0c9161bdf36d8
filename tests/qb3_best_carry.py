"""tests/qb3_best_carry.py -- rasters that carry a band's common factor across the chunks the encoders code in parallel, at every
alignment, and the census of what they reach (test infrastructure, no GPU; tests/test_best_carry.py).

A block row of the raster is 257 blocks, a prime: against any chunk length below 257 a pattern that repeats every block row
meets every offset.  The background is flat (value 0: rung-0 units, which neither read nor write a band's factor); every built
block ends on 0 along the curve, so the flat block behind it stays flat and a block's pixels do not depend on its neighbours.
A pattern row holds a writer, a dependent directly behind it, a writer of another factor, then dependents every five blocks: the
first writer's factor again, other factors, and units whose choice between the index and the factor form hangs on whether the
band's factor is theirs ("flip" units).  Between pattern rows lie 0, 1, 2 or 9 flat rows in rotation.  Every fifth pattern row ends
in a unit of factor 2 -- the factor a fresh encoder starts from: the chunks behind it are entered with the assumed state through
a writer, not through the absence of one.
"""
import functools

import numpy as np

import qb3_spec as S
import qb3_best_spec as B
import qb3_best_cells as K

PERIOD = 257                                    # blocks a block row
GAPS = (0, 1, 2, 9)                             # flat rows between pattern rows, in rotation
QUOT = [1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 1, -1, 2, -2, 0, 0]     # eleven values that add up to 0 and share no factor
SMALL = (5, 7, 3, 11)                           # factors every width has with QUOT (11 * 5 < 128)
WIDE = {1: (), 2: (257,), 4: (65537,), 8: ((1 << 33) + 1, (1 << 40) + 15)}
FLIP_FACTORS = (5, 7)


def factor_unit(f, turn=0):
    """mag-sign deltas of a unit of factor f that adds up to 0: never index-coded (eleven values), a writer"""
    q = QUOT[turn % 16:] + QUOT[:turn % 16]
    return tuple(K.ms(f * x) for x in q)


@functools.lru_cache(maxsize=None)
def flip_unit(nbytes, f):
    """mag-sign deltas of a unit of factor f, adding up to 0, coded from rung 0 (a flat block before it): in the factor form when the
    band's factor is f, in the index form when it is another -- found by search over units of three values (a f, -b f, 0)"""
    scratch = K.Census(nbytes)
    rng = np.random.default_rng(7)
    for a in range(1, 9):
        for b in range(1, 9):
            for ka in range(1, 15):
                if (ka * a) % b or ka + ka * a // b > 16 or np.gcd(a, b) != 1:
                    continue
                kb = ka * a // b
                vals = [a * f] * ka + [-b * f] * kb + [0] * (16 - ka - kb)
                for _ in range(4):
                    g = tuple(K.ms(vals[i]) for i in rng.permutation(16))
                    if B.gcf(g) != f:
                        continue
                    same, new = B.best_unit(g, 0, f - 2, nbytes), B.best_unit(g, 0, f + 5, nbytes)
                    if same.kind == "C" and new.kind == "I":
                        scratch.writer, scratch.between = None, []
                        assert {c[:8] for c in scratch._cells(same, g, 0)} & {"flip:thr", "flip:idx"}
                        return g
    raise AssertionError("no flip unit of factor %d for %d-byte values" % (f, nbytes))


def pattern_rows(nrows, keep=None):
    """the block rows that hold the pattern: [(block row, pattern number)], the first and the last block row among them; keep: only
    those pattern numbers (the sparse raster)"""
    rows, r, i = [], 0, 0
    while r < nrows - 1:
        rows.append((r, i))
        r += 1 + GAPS[i % 4]
        i += 1
    rows.append((nrows - 1, i + (i % 5 == 4)))     # (not a row that ends in factor 2: band 0 leaves another factor than a fresh encoder has)
    return [x for x in rows if keep is None or x[1] in keep]


def row_units(nbytes, i, lead=None):
    """{column: unit} of pattern row number i (a band's own: bands pass different numbers); lead: the factor of the row's first unit"""
    facs = SMALL + WIDE[nbytes]
    n = len(facs)
    b, c, d = facs[i % n], facs[(i + 1) % n], facs[(i + 2) % n]
    xa, xb = FLIP_FACTORS[i % 2], FLIP_FACTORS[(i // 2 + 1) % 2]
    j = (5 * i) % 11                            # (the columns move from row to row: every chunk length below the period sees every offset)
    out = {1 + j % 3: flip_unit(nbytes, xa) if lead is None else factor_unit(lead),
           12: factor_unit(b), 13: factor_unit(b, 3),            # a writer, a dependent directly behind it
           40 + j: factor_unit(c, 1)}                            # a writer of another factor
    kinds = [lambda t: factor_unit(b, t), lambda t: flip_unit(nbytes, xb), lambda t: factor_unit(d, t), lambda t: flip_unit(nbytes, xa),
             lambda t: factor_unit(c, t), lambda t: flip_unit(nbytes, c if c in FLIP_FACTORS else xa)]
    for t, col in enumerate(range(56 + j, 247, 5)):
        out[col] = kinds[(t + i) % len(kinds)](t)
        if t % 5 == 2:
            out[col + 2] = flip_unit(nbytes, xb if t % 2 else xa)      # (a flip unit two blocks behind a writer: a flat block between)
    out[255] = flip_unit(nbytes, xa)                                # (the row's last: never changes the band's factor -- index-coded, or of that factor)
    if i % 5 == 4:
        out[251] = factor_unit(c, 2)
        out[253] = factor_unit(2, 5)                                # the factor a fresh encoder starts from, through a writer
    return out


class Carry:
    """a carry raster: .units {(block, band): mag-sign deltas} of the blocks that are not flat, .shape (h, w, bands), .nbytes"""

    def __init__(self, nbytes, bands, nrows, keep=None, turn=0, lead=None):
        self.nbytes, self.bands, self.nrows = nbytes, bands, nrows
        self.shape = (4 * nrows, 4 * PERIOD, bands)
        self.units = {}
        for n, (r, i) in enumerate(pattern_rows(nrows, keep)):
            for c in range(bands):
                for col, g in row_units(nbytes, i + 2 * c + turn, lead if n == 0 else None).items():
                    self.units[(r * PERIOD + col, c)] = g

    def raster(self, dtype, cband=None, order=S.HILBERT):
        """the pixels, of QB3 type dtype: a block's values are the running sums of its deltas along the curve (it is entered with 0 and
        ends on 0); the band map added back (band c holds its deltas' values plus those of band cband[c])"""
        nbits = 8 * self.nbytes
        h, w, b = self.shape
        diff = np.zeros((h, w, b), dtype=np.uint64)
        tiles = {}
        for (k, c), g in self.units.items():
            if g not in tiles:
                t, p = np.zeros((4, 4), dtype=np.uint64), 0
                for i, d in enumerate(g):
                    p = (p + S.smag(d, nbits)) & ((1 << nbits) - 1)
                    nib = (order >> (60 - 4 * i)) & 15
                    t[nib >> 2, nib & 3] = p
                assert p == 0, "a block ends on the background value"
                tiles[g] = t
            by, bx = divmod(k, PERIOD)
            diff[4 * by:4 * by + 4, 4 * bx:4 * bx + 4, c] = tiles[g]
        import qb3_table_spec as T
        cb = T.band_map(b, cband)
        img = diff.copy()
        for c in range(b):
            if cb[c] != c:
                img[..., c] = diff[..., c] + diff[..., cb[c]]
        nptype = (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64)[dtype]
        return np.ascontiguousarray(img.astype(T.UNSIGNED[dtype]).view(nptype))

    def spec(self, state=None):
        """{(block, band): (Unit, rung before, factor less 2 before)} of the units that are not flat, and the state behind the raster:
        a flat unit leaves rung 0 and the factor as it was"""
        out, end = {}, []
        cache = {}
        for c in range(self.bands):
            rung, pcf = state[c] if state else (0, 0)
            last = -1
            for k in sorted(k for k, cc in self.units if cc == c):
                if k != last + 1:
                    rung = 0
                g = self.units[(k, c)]
                key = (g, rung, pcf)
                if key not in cache:
                    cache[key] = B.best_unit(list(g), rung, pcf, self.nbytes)
                u = cache[key]
                out[(k, c)] = (u, rung, pcf)
                rung, pcf, last = u.rung, u.pcf, k
            if last != self.nrows * PERIOD - 1:
                rung = 0
            end.append((rung, pcf))
        return out, end


def census(spec, bands, nbp):
    """per band, from the spec's units and the blocks a chunk holds: offsets (in their chunk) of the dependents -- units with a factor,
    whose bits hang on the band's factor before them --, how many chunks back their last writer lies, what the units that read
    the state their chunk is entered with (no writer before them in it) turn out to be, and what each chunk with a writer leaves"""
    out = []
    for c in range(bands):
        offsets, back, readers, writer_chunks, leaves = set(), set(), set(), set(), {}
        writer = None                       # chunk of the last unit that left its factor
        for k in sorted(k for k, cc in spec if cc == c):
            u, _, _ = spec[(k, c)]
            if u.cf >= 2:
                chunk = k // nbp
                if writer is not None:
                    offsets.add(k % nbp)
                    back.add(min(chunk - writer, 3))
                    if writer < chunk:
                        same = u.info["same"]
                        flips = u.kind == "I" or any(x.startswith("flip") for x in _flip_cells(u))
                        readers.add(("flip-" if flips else "factor-") + ("same" if same else "new") + ":" + u.kind)
                if u.kind == "C":
                    writer = chunk
                    writer_chunks.add(chunk)
                    leaves[chunk] = u.cf - 2            # what the chunk's last writer leaves in the band's state
        out.append(dict(offsets=offsets, back=back, readers=readers, writer_chunks=writer_chunks, leaves=leaves, last_writer=writer))
    return out


def _flip_cells(u):
    base, fac = u.info["base"], u.info["fac"]
    if u.idx is None:
        return []
    return (["flip:thr"] if base < u.thr <= base + fac and u.idx < base else []) + (["flip:idx"] if base >= u.thr and base <= u.idx < base + fac else [])


# (type, bands, band map, block rows): the cases of tests/test_best_carry.py, by the front end that codes them
CASES = [(0, 1, None, 256), (0, 3, None, 256),              # k_enc_px_best.hip
         (5, 1, None, 256), (7, 1, None, 256),              # pxw_front
         (0, 2, (0, 1), 256), (0, 16, tuple(range(16)), 256), (7, 8, tuple(range(8)), 128)]      # enc_front
SPARSE_KEEP = (25,)     # the one pattern row the sparse raster keeps: a chunk seam of every case's plan lies inside it, and band 0 does not
                        # end on the factor a fresh encoder starts from (both asserted with the plans)
MANY_CHUNKS = {(0, 16): 4096, (7, 8): 2048}     # chunks these must exceed: the scan across chunks works in parts of whole multiples of 2048
