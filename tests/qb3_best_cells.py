"""tests/qb3_best_cells.py -- rasters built to stand on every boundary of the common-factor modes' coding decision, and the census
that says which boundaries ("cells") a sequence of units reaches (test infrastructure, no GPU).

The units are found by search over the sizes tests/qb3_best_spec.py computes, with a fixed seed: a candidate is kept when, coded
from the state the sequence has reached, it stands in a cell nothing before it stands in.  tests/test_best_spec.py asserts from
the census that every cell a width can have is there (REQUIRED less ABSENT), and that the spec's stream for the sequence is the
oracle's, before any GPU test uses the rasters.

Cell names (UB: the rung-switch bits of the width; size: the plain or factor form's bits; thr = 36 + 3 UB + 2 rung):
  try:*    whether the index form is looked at (rung 3 | 4, 62 | 63, size = thr - 1 | thr)
  win:*    whether it wins (idx = size - 1 | size, eight | nine values, the count profiles, equal counts in both orders)
  fac:*    where a factor is written, each entered with the same factor before it (:same) and another (:new)
  flip:*   units for which only same-or-new decides between the index and the factor form
  pcf:*    an index-coded unit with a factor of its own leaves the band's factor alone
  gcd:*    what the factor search must get right
"""
import functools
from math import gcd

import numpy as np

import qb3_spec as S
import qb3_best_spec as B

NBITS = {1: 8, 2: 16, 4: 32, 8: 64}


def ms(x):
    """mag-sign of a signed integer"""
    return 2 * x if x >= 0 else -2 * x - 1


def _counts(g):
    c = {}
    for v in g:
        c[v] = c.get(v, 0) + 1
    return sorted(c.values(), reverse=True)


class Census:
    """the cells a band's units reach, one after another: feed(unit, group, rung before) returns the unit's cells; .cells: all so far,
    .where: cell -> the first unit's number"""

    def __init__(self, nbytes):
        self.nbytes, self.ub, self.nbits = nbytes, S.UB[nbytes], NBITS[nbytes]
        self.cells, self.where, self.n = set(), {}, 0
        self.first_factor = True
        self.writer = None              # the factor of the last unit that left one behind
        self.between = []               # (kind, factor) of the units since

    def copy(self):
        c = Census(self.nbytes)
        c.cells, c.where, c.n = set(self.cells), dict(self.where), self.n
        c.first_factor, c.writer, c.between = self.first_factor, self.writer, list(self.between)
        return c

    def feed(self, u, g, oldrung):
        out = self._cells(u, g, oldrung)
        for c in out:
            self.where.setdefault(c, self.n)
        self.cells |= out
        self.n += 1
        return out

    def _cells(self, u, g, oldrung):
        ub, nbytes, out = self.ub, self.nbytes, set()
        if u.kind == "0":
            self.between.append(("0", 0))
            return out
        cnt, f = _counts(g), "cf" if u.cf >= 2 else "nocf"
        mag = [B.magsabs(v) for v in g]
        # ------------------------------------------------------------------------------------- is the index form looked at
        if u.rung in (3, 63) and len(cnt) <= 8 and B.index_unit(g, u.rung, oldrung, nbytes).n < u.size:
            out.add("try:rung%d:a-shorter-index-form-not-tried" % u.rung)
        if u.rung in (4, 62) and u.kind == "I":
            out.add("try:rung%d:index" % u.rung)
        if u.idx is not None and u.size == u.thr - 1 and u.idx < u.size:
            out.add("try:size=thr-1:a-shorter-index-form-not-tried")
        if u.tried and u.size == u.thr:
            out.add("try:size=thr:" + ("index" if u.kind == "I" else "kept"))
        # ------------------------------------------------------------------------------------- does it win
        if u.tried:
            if u.idx == u.size - 1:
                out.add("win:idx=size-1:" + f)
            if u.idx == u.size:
                out.add("win:idx=size:" + f)
            if len(cnt) == 9:
                out.add("win:nine-values")
            if u.kind == "I":
                if len(cnt) == 8:
                    out.add("win:eight-values")
                for name, prof in (("15+1", [15, 1]), ("8+8", [8, 8]), ("4x4", [4] * 4), ("9+1x7", [9] + [1] * 7)):
                    if cnt == prof:
                        out.add("win:" + name)
                if cnt == [8, 8]:
                    out.add("win:8+8:the-%s-value-first" % ("smaller" if g[0] == min(g) else "larger"))
        # ------------------------------------------------------------------------------------- the factor
        if u.cf >= 2:
            i = u.info
            t, c, cfm = i["trung"], i["cfrung"], i["cfm"]
            sfx = ":same" if i["same"] else ":new"
            if u.kind == "C":
                fc = set()
                if cfm <= 1:
                    fc.add("fac:cf=%d:trung%s" % (u.cf, "=0" if t == 0 else "<UB" if t < ub else ">=UB"))
                else:
                    for name, tt in (("cfrung-1", c - 1), ("cfrung", c), ("cfrung+UB-1", c + ub - 1), ("cfrung+UB", c + ub)):
                        if t == tt:
                            fc.add("fac:trung=" + name)
                    if i["own_if_new"] and c < t:
                        fc.add("fac:own-rung-switch-wraps")
                if t < oldrung:
                    fc.add("fac:group-switch-wraps")
                for r in range(1, 8):
                    if t == r and cfm == 1 << r:
                        fc.add("fac:cf-2=2^%d:at-rung-%d" % (r, r))
                    if t == r and cfm == (1 << r) - 1 and cfm > 0:
                        fc.add("fac:cf-2=2^%d-1:at-rung-%d" % (r, r))
                if u.cf == 1 << (self.nbits - 1):
                    fc.add("fac:largest")
                out |= {x + sfx for x in fc}
                if t == 0:
                    out.add("fac:trung=0:" + ("kept" if i["same"] else "own-rung" if i["own"] else "group-rung"))
                if self.first_factor and u.cf == 2 and i["same"]:
                    out.add("fac:first-of-the-image-is-2:same")
            if u.idx is not None:
                base, fac = i["base"], i["fac"]
                if base < u.thr <= base + fac and u.idx < base:
                    out.add("flip:thr" + sfx)
                if base >= u.thr and base <= u.idx < base + fac:
                    out.add("flip:idx" + sfx)
            # --------------------------------------------------------------------------------- who writes the band's factor
            if u.kind == "C" and self.writer is not None:
                idx_f = [cf for k, cf in self.between if k == "I" and cf >= 2 and cf != self.writer]
                gap = ":with-other-units-between" if {"0", "N"} <= {k for k, _ in self.between} else ""
                if idx_f and u.cf == self.writer:
                    assert i["same"]
                    out.add("pcf:index-unit-does-not-write:same" + gap)
                if idx_f and u.cf == idx_f[-1]:
                    assert not i["same"]
                    out.add("pcf:index-unit-does-not-write:new" + gap)
            # --------------------------------------------------------------------------------- the factor search
            nz = [m for m in mag if m]
            if u.kind == "C":
                if len(nz) < 16 and len(nz) > 1:
                    out.add("gcd:zeros")
                if len(nz) == 1:
                    out.add("gcd:one-non-zero-value")
                if any(v & 1 for v in g):
                    out.add("gcd:negative-values")
                if max(mag) == 256:
                    out.add("gcd:magnitude-256:rung-%d" % u.rung)
                if nbytes == 2:
                    for name, cf, top in (("2", 2, 1 << 15), ("3", 3, 32766), ("16381", 16381, 32762)):
                        if u.cf == cf and max(mag) == top:
                            out.add("gcd:16-bit:factor-%s-to-%d" % (name, top))
                if nbytes >= 4 and max(mag) == (1 << 23) - 1 and u.cf >= 1 << 10:
                    out.add("gcd:2^23-1-with-a-large-factor")
                if nbytes == 8 and u.cf > 1 << 32:
                    out.add("gcd:factor-above-2^32")
        else:
            nz = [m for m in mag if m]
            ones = [m for m in nz if m == 1]
            rest = [m for m in nz if m != 1]
            if len(ones) == 1 and len(rest) >= 2 and functools.reduce(gcd, rest) >= 2:
                out.add("gcd:a-magnitude-of-1-among-multiples")
        if u.kind == "C":
            self.first_factor = False
            self.writer, self.between = u.cf, []
        else:
            self.between.append((u.kind, u.cf))
        return out


def required(nbytes):
    """(the cells a width must show, {cell the width cannot have: why})"""
    ub, nbits = S.UB[nbytes], NBITS[nbytes]
    both = lambda names: [n + s for n in names for s in (":same", ":new")]      # noqa: E731
    fac = ["fac:cf=2:trung=0", "fac:cf=3:trung=0", "fac:cf=2:trung<UB", "fac:cf=3:trung<UB", "fac:cf=2:trung>=UB", "fac:cf=3:trung>=UB",
           "fac:trung=cfrung-1", "fac:trung=cfrung", "fac:trung=cfrung+UB-1", "fac:trung=cfrung+UB", "fac:own-rung-switch-wraps",
           "fac:group-switch-wraps", "fac:largest"]
    fac += ["fac:cf-2=2^%d:at-rung-%d" % (r, r) for r in range(1, 8)] + ["fac:cf-2=2^%d-1:at-rung-%d" % (r, r) for r in range(2, 8)]
    req = ["try:rung3:a-shorter-index-form-not-tried", "try:rung4:index", "try:size=thr-1:a-shorter-index-form-not-tried",
           "try:size=thr:index", "try:size=thr:kept",
           "win:idx=size-1:cf", "win:idx=size-1:nocf", "win:idx=size:cf", "win:idx=size:nocf", "win:eight-values", "win:nine-values",
           "win:15+1", "win:8+8", "win:4x4", "win:9+1x7", "win:8+8:the-smaller-value-first", "win:8+8:the-larger-value-first",
           "fac:trung=0:kept", "fac:trung=0:own-rung", "fac:trung=0:group-rung", "fac:first-of-the-image-is-2:same",
           "flip:thr:same", "flip:thr:new", "flip:idx:same", "flip:idx:new",
           "pcf:index-unit-does-not-write:same", "pcf:index-unit-does-not-write:new",
           "pcf:index-unit-does-not-write:same:with-other-units-between", "pcf:index-unit-does-not-write:new:with-other-units-between",
           "gcd:zeros", "gcd:one-non-zero-value", "gcd:negative-values", "gcd:a-magnitude-of-1-among-multiples",
           "gcd:magnitude-256:rung-8", "gcd:magnitude-256:rung-9"] + both(fac)
    absent = {}
    if nbytes == 8:
        req += ["try:rung62:index", "try:rung63:a-shorter-index-form-not-tried", "gcd:factor-above-2^32"]
    if nbytes >= 4:
        req += ["gcd:2^23-1-with-a-large-factor"]
    if nbytes == 2:
        req += ["gcd:16-bit:factor-2-to-32768", "gcd:16-bit:factor-3-to-32766", "gcd:16-bit:factor-16381-to-32762"]
    if nbytes == 1:
        # a delta's magnitude is 128 at the most: a factor of 2^r + 2 (2^r + 1) times a quotient at rung r, 2^(r-1) or more, is past it
        # from r = 4 on: 18 * 8 = 144, 17 * 8 = 136
        for r in range(4, 8):
            for s in (":same", ":new"):
                absent["fac:cf-2=2^%d:at-rung-%d%s" % (r, r, s)] = "(2^%d + 2) * 2^%d > 128" % (r, r - 1)
                absent["fac:cf-2=2^%d-1:at-rung-%d%s" % (r, r, s)] = "(2^%d + 1) * 2^%d > 128" % (r, r - 1)
        for c in ("gcd:magnitude-256:rung-8", "gcd:magnitude-256:rung-9"):
            absent[c] = "no 8-bit delta has the magnitude 256"
    return [c for c in req if c not in absent], absent


# ---------------------------------------------------------------------------------------------------------------- the search

class _Builder:
    def __init__(self, nbytes, seed):
        self.nbytes, self.ub, self.nbits = nbytes, S.UB[nbytes], NBITS[nbytes]
        self.rng = np.random.default_rng(seed)
        self.seq, self.rung, self.pcf = [], 0, 0
        self.census = Census(nbytes)
        self.lo, self.hi = -(1 << (self.nbits - 1)), (1 << (self.nbits - 1)) - 1

    def run(self, cand, census):
        rung, pcf, got = self.rung, self.pcf, set()
        for g in cand:
            u = B.best_unit(g, rung, pcf, self.nbytes)
            got |= census.feed(u, g, rung)
            rung, pcf = u.rung, u.pcf
        return got, rung, pcf

    def add(self, cand):
        _, self.rung, self.pcf = self.run(cand, self.census)
        self.seq += [list(g) for g in cand]

    def want(self, cells, gen, tries=20000, again=False):
        """candidates from gen() until every cell of `cells` is there; one is kept when it brings a cell of `cells` that is missing.
        again: missing are the cells this call has not brought yet, whatever the sequence holds already"""
        cells = [cells] if isinstance(cells, str) else list(cells)
        have = set() if again else self.census.cells
        for _ in range(tries):
            missing = {c for c in cells if c not in have}
            if not missing:
                return
            cand = gen()
            if cand is None:
                continue
            got, _, _ = self.run(cand, self.census.copy())
            if got & missing:
                self.add(cand)
                if again:
                    have |= got
        missing = [c for c in cells if c not in have]
        assert not missing, "no unit found for %s (%d-bit)" % (missing, self.nbits)

    def plain_at(self, p):
        """a unit that leaves the rung p and no factor: flat, or fifteen random values below 2^p and 2^p"""
        if p == 0:
            return [0] * 16
        return [ms(int(x)) for x in self.rng.integers(-(1 << (p - 1)), 1 << (p - 1), 15)] + [1 << p]

    def near(self, u):
        """can a unit that is u when coded from rung 0 stand on a boundary when coded from another rung?  The rung before it is in the
        sizes through the switch codes alone: at most UB + 1 bits in the plain or factor form, twice two in the index form"""
        if u.idx is None:
            return False
        slack = self.ub + 6
        if abs(u.idx - u.size) <= slack + 1 or abs(u.size - u.thr) <= slack:
            return True
        if u.cf >= 2:
            base, fac = u.info["base"], u.info["fac"]
            return u.thr - fac - slack <= base <= u.thr + slack or -slack <= u.idx - base <= fac + slack
        return False

    def tight(self, cells, gen1, tries=20000):
        """for cells that hang on a bit: a group from gen1() is coded from every rung before it, with the factor before it its own and
        another; where that reaches a missing cell, the group goes in behind a unit that leaves that factor and one that leaves that
        rung"""
        cells = [cells] if isinstance(cells, str) else list(cells)
        scratch = Census(self.nbytes)
        for _ in range(tries):
            missing = {c for c in cells if c not in self.census.cells}
            if not missing:
                return
            g = gen1()
            if g is None:
                continue
            g = g[0]
            cf = B.gcf(g)
            if not any(self.near(B.best_unit(g, 0, pcf or 0, self.nbytes)) for pcf in ((cf - 2, cf - 1) if cf >= 2 else (None,))):
                continue
            for old in range(min(self.nbits, 1 << self.ub)):
                for pcf in ((cf - 2, cf - 1) if cf >= 2 else (None,)):
                    u = B.best_unit(g, old, pcf or 0, self.nbytes)
                    scratch.writer, scratch.between = None, []      # (no history: the cells looked for here hang on the unit alone)
                    if not scratch._cells(u, g, old) & missing:
                        continue
                    cand = [self.plain_at(old), g]
                    if pcf is not None:
                        w = self.unit([(pcf + 2) * q for q in self.quotients(1)])
                        if w is None:
                            continue
                        cand = [w] + cand
                    got, _, _ = self.run(cand, self.census.copy())
                    if got & missing:
                        self.add(cand)
                        missing -= got
        missing = [c for c in cells if c not in self.census.cells]
        assert not missing, "no unit found for %s (%d-bit)" % (missing, self.nbits)

    # --- families of candidates (signed deltas, then mag-sign) ---
    def ok(self, vals):
        return all(self.lo <= v <= self.hi for v in vals)

    def unit(self, vals):
        return [ms(int(v)) for v in vals] if self.ok(vals) else None

    def spread(self, pal, counts=None):
        """sixteen values from a palette with the given counts (random ones otherwise), in random order"""
        rng, n = self.rng, len(pal)
        if counts is None:
            cuts = sorted(rng.choice(np.arange(1, 16), n - 1, replace=False)) if n > 1 else []
            counts = np.diff([0] + list(cuts) + [16])
        vals = [p for p, k in zip(pal, counts) for _ in range(int(k))]
        return [vals[i] for i in rng.permutation(16)]

    def palette(self, n, r, cf=1, tb=None):
        """n distinct signed values: magnitudes below 2^(r-1) and one with its mag-sign top bit at r -- or, with a factor, cf times
        quotients whose mag-sign top bit is tb at the most"""
        rng = self.rng
        for _ in range(100):
            if cf == 1:
                mags = {int(x) for x in rng.integers(0, 1 << (r - 1), n - 1)} | {int(rng.integers(1 << (r - 1), 1 << r))}
                pal = [m if rng.random() < 0.5 else -m for m in mags]
            else:
                q = {int(x) for x in rng.integers(-(1 << tb) // 2, (1 << tb) // 2 + 1, n)}
                pal = [cf * x for x in q]
            if len(set(pal)) == n:
                return pal
        return None

    def gen_index(self, rungs, ns=range(2, 10), counts=None, cf=False, pre=False):
        """a unit of few distinct values at one of `rungs`; pre: behind a plain unit of a random rung, so that the search meets the unit
        with every rung before it (the switch codes' lengths are part of every size)"""
        rng = self.rng

        def gen():
            out = gen1()
            if out is None or not pre:
                return out
            p = int(rng.integers(0, min(self.nbits - 1, 1 << self.ub, 41)))
            first = [0] * 16 if p == 0 else [ms(int(x)) for x in rng.integers(-(1 << (p - 1)), 1 << (p - 1), 15)] + [1 << p]
            return [first] + out

        def gen1():
            r = int(rng.choice(list(rungs)))
            n = len(counts) if counts else int(rng.choice(list(ns)))
            if cf:
                tb = int(rng.integers(1, 4))
                c = int(rng.integers(2, max(3, 1 << max(1, r - tb))))
                pal = self.palette(n, r, c, tb)
            else:
                pal = self.palette(n, r)
            return None if pal is None else self._one(self.spread(pal, counts))
        return gen

    def _one(self, vals):
        u = self.unit(vals)
        return None if u is None else [u]

    def quotients(self, t, n=16):
        """n signed quotients whose mag-sign values have their top bit at t, a 1 among them (so that their own factor is 1)"""
        rng = self.rng
        if t == 0:
            q = [int(x) for x in -rng.integers(0, 2, n)]
            q[int(rng.integers(0, n))] = -1
            return q
        top = 1 << t
        m = [int(x) for x in rng.integers(0, 2 * top, n)]
        m[0] = int(rng.integers(top, 2 * top))
        m[1] = 2 if t >= 1 else 1                        # the quotient +1
        m = [m[i] for i in rng.permutation(n)]
        return [(v >> 1) if not v & 1 else -((v + 1) >> 1) for v in m]

    def gen_factor(self, cfs, ts, pair=True):
        """a unit of factor cf (from cfs) with quotients at rung t (from ts), and a second one of the same factor and rung behind it"""
        rng = self.rng

        def gen():
            cf, t = int(rng.choice(list(cfs))), int(rng.choice(list(ts)))
            out = []
            if self.pcf == cf - 2:                       # the band's factor is this one already: another first
                out.append(self.unit([(cf + 5) * q for q in self.quotients(1)]))
                if out[0] is None:
                    return None
            for _ in range(2 if pair else 1):
                u = self.unit([cf * q for q in self.quotients(t)])
                if u is None:
                    return None
                out.append(u)
            return out
        return gen


def _cfs_at(c, rng, nbits, k=6):
    """factors whose value less 2 has its top bit at c"""
    if c == 0:
        return [2, 3]
    return sorted({(1 << c) + 2, (1 << (c + 1)) + 1} | {int(x) + 2 for x in rng.integers(1 << c, 2 << c, k)})


@functools.lru_cache(maxsize=None)
def decision_units(nbytes, seed=20):
    """(the groups of one band, the Census of them): every cell of required(nbytes) is there.  64-bit: every unit with more than eight
    values stays under 800 bits (SURVEY B-2): such units keep to rungs of 40 and below"""
    b = _Builder(nbytes, seed)
    rng, ub, nbits = b.rng, b.ub, b.nbits
    both = lambda n: [n + ":same", n + ":new"]      # noqa: E731
    hi_t = min(nbits - 4, 40)

    # the image's first factor unit has the factor 2, which the starting state calls "the same"
    b.want("fac:first-of-the-image-is-2:same", lambda: [[ms(2 * q) for q in b.quotients(2)]])

    # ---- where the factor is written, each cell entered with the same factor and with another
    def place(cell, cfs, ts, again=False):
        b.want(both(cell), b.gen_factor(cfs, ts), again=again)
    for cf in (2, 3):
        place("fac:cf=%d:trung=0" % cf, [cf], [0])
        place("fac:cf=%d:trung<UB" % cf, [cf], range(1, ub))
        place("fac:cf=%d:trung>=UB" % cf, [cf], range(ub, min(ub + 3, nbits - 3)))
    crs = [c for c in range(1, hi_t) if c + ub + 1 + 1 <= nbits - 2]          # factor rungs that leave room for quotients at c + UB
    pick = [c for c in (1, 2, 3, 5, 9, 17, 30, 40) if c in crs]
    for name, d in (("cfrung-1", -1), ("cfrung", 0), ("cfrung+UB-1", ub - 1), ("cfrung+UB", ub)):
        for c in pick:
            if c + d < 0 or (c + 1) + (c + d) > nbits - 2:
                continue
            # (every rung of `pick` goes in, not only the first that fills the cell: the census counts cells, the kernels see rungs)
            place("fac:trung=" + name, _cfs_at(c, rng, nbits), [c + d], again=True)
    b.want(both("fac:own-rung-switch-wraps"), b.gen_factor(_cfs_at(1, rng, nbits), [1 + ub]))
    for r in range(1, 8):
        if ((1 << r) + 2) << (r - 1) <= b.hi:
            place("fac:cf-2=2^%d:at-rung-%d" % (r, r), [(1 << r) + 2], [r])
            if r >= 2:
                place("fac:cf-2=2^%d-1:at-rung-%d" % (r, r), [(1 << r) + 1], [r])
    # a high rung, then a factor unit of a low one: the quotients' rung switch is negative
    b.want(both("fac:group-switch-wraps"),
           lambda: (lambda hi, f: None if hi is None or f is None else hi + f)(
               b._one([int(x) for x in rng.integers(-(1 << (nbits - 3)), 1 << (nbits - 3), 16)] if nbytes < 8 else
                      b.spread([int(x) for x in rng.integers(-(1 << 60), 1 << 60, 5)])),
               b.gen_factor([5, 6, 7], [1, 2])()))
    # the largest factor: every non-zero delta is the type's lowest value
    b.want(both("fac:largest"), lambda: [b.unit([b.lo if x else 0 for x in rng.integers(0, 2, 16)] [:15] + [b.lo]) for _ in range(2)])
    b.want(["fac:trung=0:kept", "fac:trung=0:own-rung", "fac:trung=0:group-rung"],
           b.gen_factor([2, 3, 4, 5, 9, 100], [0]))

    # ---- is the index form looked at, does it win
    b.want("try:rung3:a-shorter-index-form-not-tried", b.gen_index([3], ns=[2]))
    b.want("try:rung4:index", b.gen_index([4], ns=[2, 3]))
    small = range(4, min(nbits - 2, 13))
    for prof in ([15, 1], [8, 8], [4] * 4, [9] + [1] * 7):
        b.want("win:" + {2: "15+1" if prof[0] == 15 else "8+8", 4: "4x4", 8: "9+1x7"}[len(prof)], b.gen_index(small, counts=prof))
    b.want(["win:8+8:the-smaller-value-first", "win:8+8:the-larger-value-first"], b.gen_index(small, counts=[8, 8]))
    b.want("win:eight-values", b.gen_index(small, ns=[8]))
    b.want("win:nine-values", b.gen_index(small, ns=[9]))
    wide = range(4, min(nbits - 1, 16))
    b.tight(["win:idx=size-1:nocf", "win:idx=size:nocf"], b.gen_index(small, ns=range(5, 9)))
    b.tight(["win:idx=size-1:cf", "win:idx=size:cf"], b.gen_index(small, ns=range(3, 9), cf=True))
    b.tight(["try:size=thr-1:a-shorter-index-form-not-tried", "try:size=thr:index", "try:size=thr:kept"],
            b.gen_index(wide, ns=[2, 3], cf=True))
    # ---- same or new decides
    b.tight(["flip:thr:same", "flip:thr:new", "flip:idx:same", "flip:idx:new"], b.gen_index(wide, ns=[2, 3, 4], cf=True))

    # ---- who writes the band's factor: 5, an index-coded unit whose factor is 7, then 5 (the same) or 7 (new); with rung-0 and plain
    # units between as well
    def writers(last, gap):
        def gen():
            w = b.unit([5 * q for q in b.quotients(2)])
            pal = b.palette(2, 0, 7, 6)
            i = b.unit(b.spread(pal)) if pal else None
            d = b.unit([last * q for q in b.quotients(2)])
            if None in (w, i, d):
                return None
            flat, plain = [0] * 16, [ms(int(x)) for x in rng.integers(-9, 10, 16)]
            return [w, flat, plain, i, plain, flat, d] if gap else [w, i, d]
        return gen
    for gap in (False, True):
        sfx = ":with-other-units-between" if gap else ""
        b.want("pcf:index-unit-does-not-write:same" + sfx, writers(5, gap))
        b.want("pcf:index-unit-does-not-write:new" + sfx, writers(7, gap))

    # ---- the factor search
    def with_zeros():
        q = b.quotients(3)
        for i in rng.choice(16, 5, replace=False):
            q[int(i)] = 0
        return b._one([6 * x for x in q] if any(q) else None) if sum(1 for x in q if x) > 1 else None
    b.want("gcd:zeros", with_zeros)
    b.want("gcd:one-non-zero-value", lambda: b._one([0] * 9 + [int(rng.integers(5, 100)) * (-1 if rng.random() < 0.5 else 1)] + [0] * 6))
    b.want("gcd:negative-values", b.gen_factor([7], [3], pair=False))
    b.want("gcd:a-magnitude-of-1-among-multiples",
           lambda: b._one([6 * int(x) for x in rng.integers(-9, 10, 15)] + [-1]))
    if nbytes > 1:
        b.want("gcd:magnitude-256:rung-8", lambda: b._one(b.spread([-256, 128, -64, 0, 192], None)))
        b.want("gcd:magnitude-256:rung-9", lambda: b._one(b.spread([256, 128, -64, 0, 192], None)))
    if nbytes == 2:
        b.want("gcd:16-bit:factor-2-to-32768", lambda: b._one([2 * int(x) for x in rng.integers(-16383, 16384, 15)] + [-32768]))
        b.want("gcd:16-bit:factor-3-to-32766", lambda: b._one([3 * int(x) for x in rng.integers(-10922, 10923, 14)] + [32766, 3]))
        b.want("gcd:16-bit:factor-16381-to-32762", lambda: b._one(b.spread([16381, -16381, 32762, -32762, 0])))
    if nbytes >= 4:
        # 2^23 - 1 = 47 * 178481
        b.want("gcd:2^23-1-with-a-large-factor", lambda: b._one(b.spread([178481 * q for q in (47, -46, 1, -3, 0, 17)])))
    if nbytes == 8:
        f = (1 << 40) + 15
        b.want("gcd:factor-above-2^32", lambda: b._one(b.spread([f * q for q in (1, -3, 7, 100, -1000, 0)])))
        # rung 62 takes the index form, rung 63 never does; eight values at the most up there (SURVEY B-2)
        b.want("try:rung62:index", lambda: b._one(b.spread([1 << 61, -(1 << 60) - 5, 3])))
        b.want("try:rung63:a-shorter-index-form-not-tried", lambda: b._one(b.spread([(1 << 62) + 1, -(1 << 62), 3])))
    return b.seq, b.census


def small_magnitude_runs(nbytes, seed=21):
    """32- and 64-bit: (groups, number of groups in the first run) -- 192 factor units whose magnitudes all stay below 2^23 and reach
    2^23 - 1, then 192 of which every 64th goes past 2^23: whatever a kernel's groups of 64 consecutive units are, at least two of
    them lie in the first run, and each one that lies in the second holds exactly one large unit"""
    assert nbytes >= 4
    rng = np.random.default_rng(seed)
    facs = [178481, 2, 3, 4099, 65537, 8191]
    out = []
    for k in range(384):
        f = facs[k % len(facs)]
        lim = ((1 << 23) - 1) // f
        q = [int(x) for x in rng.integers(-lim, lim + 1, 16)]
        i = int(rng.integers(0, 16))
        q[i], q[(i + 5) % 16] = (lim if k % 2 else -lim), 1           # the run's largest magnitude; the quotients have no factor
        g = [f * x for x in q]
        if k >= 192 and k % 64 == 40:
            big = (1 << 23) // f + 1 + int(rng.integers(0, 1000))
            g[3] = f * big
            if nbytes == 8 and k == 232:
                g = [((1 << 33) + 9) * x for x in q]         # a factor above 2^32 in a group of small ones
        out.append([ms(v) for v in g])
    return out, 192


def pad_to_rows(units, ncols):
    """the groups with flat ones behind them, to whole block rows"""
    return units + [[0] * 16] * (-len(units) % ncols)


# ---------------------------------------------------------------------------------------------------------------- whole rasters

NCOLS = 20          # blocks a block row of the decision rasters


def random_units(nbytes, n, seed):
    """n groups of every family the search draws from, at random: plain units of any rung, flat and one-bit units, factor units with
    factors and quotients of any rung that fits, units of few values with and without a factor (64-bit: more than eight values only
    up to rung 40, SURVEY B-2)"""
    b = _Builder(nbytes, seed)
    rng, nbits = b.rng, b.nbits
    top = min(nbits - 1, 40)
    out = []
    while len(out) < n:
        k = int(rng.integers(0, 6))
        if k == 0:
            cand = [b.plain_at(int(rng.integers(0, top + 1)))]
        elif k == 1:
            cand = [[int(x) for x in rng.integers(0, 2, 16)] if rng.random() < 0.5 else [0] * 16]
        elif k == 2:
            c = int(rng.integers(0, top - 2))
            cand = b.gen_factor(_cfs_at(c, rng, nbits), range(0, max(1, top - c - 2)), pair=rng.random() < 0.5)()
        elif k == 3:
            cand = b.gen_index(range(1, min(nbits - 1, 62)), ns=range(1, 9), cf=rng.random() < 0.5)()
        elif k == 4:
            cand = b.gen_index(range(2, 14), ns=range(7, 11))()
        else:
            cand = b._one(b.spread([int(x) for x in rng.integers(b.lo, b.hi, 3)] + [b.lo, b.hi]))
        if cand:
            out += [g for g in cand if g is not None]
    return out[:n]


@functools.lru_cache(maxsize=None)
def case_units(nbytes):
    """the groups of a decision raster's first band: the cells, 32/64-bit the runs of small magnitudes, then all of it again turned
    round (other rungs and factors before every unit) until there are several chunks of any encoder, to whole block rows"""
    seq = list(decision_units(nbytes)[0])
    if nbytes >= 4:
        seq += small_magnitude_runs(nbytes)[0]
    out, k = list(seq), 1
    while len(out) < 560:
        r = (53 * k) % len(seq)
        out += seq[r:] + seq[:r]
        k += 1
    return pad_to_rows(out, NCOLS)


def rotated(seq, bands):
    """the sequence for each of `bands` bands, turned by a different amount a band"""
    n = len(seq)
    return [seq[(c * 97) % n:] + seq[:(c * 97) % n] for c in range(bands)]


class SpecCase:
    """the spec's stream of per-band groups: .per [band][block] Units, .cells [band][block] sets, .bits, .starts [(bit, block, band)]
    in stream order, .state [(rung, factor less 2) a band] behind the last block"""

    def __init__(self, bands, nbytes, state=None):
        self.per, self.bits = B.encode_bands(bands, nbytes, state)
        self.cells, self.starts = [], []
        for c, units in enumerate(self.per):
            cen, rung = Census(nbytes), (state[c][0] if state else 0)
            row = []
            for u, g in zip(units, bands[c]):
                row.append(cen.feed(u, g, rung))
                rung = u.rung
            self.cells.append(row)
        pos = 0
        for k in range(len(bands[0])):
            for c in range(len(bands)):
                self.starts.append((pos, k, c))
                pos += self.per[c][k].bits.n
        self.state = [(p[-1].rung, p[-1].pcf) for p in self.per]

    def explain(self, stream, nbits):
        """None where `stream` (an int, nbits bits) is the spec's, else the first differing unit in words, with its cells"""
        diff = (stream ^ self.bits.v) & ((1 << min(nbits, self.bits.n)) - 1)
        if not diff and nbits == self.bits.n:
            return None
        bit = (diff & -diff).bit_length() - 1 if diff else min(nbits, self.bits.n)
        at = max(i for i, (p, _, _) in enumerate(self.starts) if p <= bit)
        p, k, c = self.starts[at]
        u = self.per[c][k]
        return "stream of %d bits, the spec's has %d; first differing bit %d: bit %d of block %d, band %d -- a unit of kind %s, rung %d, " \
               "factor %d, %d bits (index form %s, threshold %d); cells: %s" % (
                   nbits, self.bits.n, bit, bit - p, k, c, u.kind, u.rung, u.cf, u.bits.n, u.idx, u.thr, sorted(self.cells[c][k]) or "none")
