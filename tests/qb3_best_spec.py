"""tests/qb3_best_spec.py -- the common-factor modes' coding decision, unit by unit, in plain Python integers (test infrastructure, no
GPU, nothing taken from the library or the oracle).

Beside tests/qb3_spec.py (the code of one value, the rung switch, the plain unit), written from the reference's rules:
- the factor of a unit: Euclid over the magnitudes, zeros left out (QB3encode.h:98-126)
- the factor unit: signal, the quotients' rung without a change flag, a "new factor" flag, the factor at the quotients' rung or at a
  rung of its own one rung down, the quotients; three short forms when the quotients are all 0 or -1 (QB3encode.h:283-361)
- the index unit: signal, a switch to the last rung, the real rung, sixteen indices, the table of at most eight values in order of
  descending count, the first seen first among equals (QB3encode.h:546-613)
- the choice, and who leaves a factor behind (QB3encode.h:679-713)
tests/test_best_spec.py pins all of it to the oracle's streams before anything on a GPU is compared with it.
"""
import numpy as np

import qb3_spec as S
from qb3_spec import Bits, UB, HILBERT

ZCURVE = 0x0145236789CDABEF             # reference QB3common.h: the legacy modes' scan order
NO_INDEX = 800                          # what the index form "costs" with more than eight distinct values (QB3encode.h:564)


def magsabs(v):
    """the magnitude of a mag-sign value (QB3encode.h:92)"""
    return (v >> 1) + (v & 1)


def magsdiv(v, cf):
    """a mag-sign value divided by a positive factor, still mag-sign (QB3encode.h:95)"""
    return ((magsabs(v) // cf) << 1) - (v & 1)


def gcf(g):
    """the greatest common factor of the magnitudes of a group that is not all zeros, as the reference finds it (QB3encode.h:98-126):
    the smallest value to the front, the others modulo it, zeros dropped, until one is left or the smallest is 1"""
    v = [magsabs(x) for x in g if magsabs(x)]
    while True:
        j = min(range(len(v)), key=lambda i: (v[i], i))
        m = v[j]
        if m == 1:
            return 1
        v[j] = v[0]
        v = [m] + [x % m for x in v[1:] if x % m]
        if len(v) == 1:
            return m


def _single(v, r):
    """one value by itself at rung r >= 0 (QB3encode.h:144-150): a bit at rung 0, the middle swap at rungs 3..7 only"""
    return (v, 1) if r == 0 else S.code_value(S.swap_single(v, r), r)


def factor_bits(cfm, trung, nbytes):
    """(Bits, own) of a factor (less 2) that differs from the one before, behind its flag (QB3encode.h:309-336): at the quotients'
    rung behind a 0 bit -- at rung 0 its one bit -- or, own, behind a switch to its rung, without its top bit, a rung below"""
    ub = UB[nbytes]
    cfrung = S.topbit(cfm | 1)
    b = Bits()
    if trung >= cfrung and (trung < cfrung + ub or cfrung == 0):
        b.put(0, 1)
        return b.put(*_single(cfm, trung)), False
    b.put(*S.switch_code(cfrung - trung, ub))
    return b.put(*_single(cfm ^ (1 << cfrung), cfrung - 1)), True


def factor_unit(g, cf, pcf, oldrung, nbytes):
    """(Bits, info) of the factor form of a group whose factor is cf >= 2, pcf the band's factor (less 2) before it.  info: trung,
    cfrung, same, own (None when same), base (the bits without the factor) and fac (the bits the factor takes when it differs)"""
    ub = UB[nbytes]
    q = [magsdiv(v, cf) for v in g]
    used = 0
    for v in q:
        used |= v
    cfm = cf - 2
    trung, cfrung = S.topbit(used | 1), S.topbit(cfm | 1)
    head = Bits().put(*S.signal_code(ub)).put(*S.switch_noflag_code(trung - oldrung, ub))
    # at rung 0 the quotients are sixteen bits with no flag in front (they cannot all be zero): QB3encode.h:312-317, 338-346, 352-356
    tail = S.group_codes(q, trung, True) if trung else Bits().put(sum(v << i for i, v in enumerate(q)), 16)
    fb, own = factor_bits(cfm, trung, nbytes)
    same = cfm == pcf
    b = Bits().extend(head)
    if same:
        b.put(0, 1)
    else:
        b.put(1, 1).extend(fb)
    b.extend(tail)
    return b, dict(trung=trung, cfrung=cfrung, same=same, own=None if same else own, own_if_new=own, base=head.n + 1 + tail.n, fac=fb.n,
                   cfm=cfm, quot=q)


def index_table(g):
    """the values of a group in the order the index form lists them: by descending count, the first seen first among equals (an insertion
    sort that moves an entry up only past a strictly smaller count: QB3encode.h:546-554); None with more than eight"""
    vals, cnt = [], {}
    for v in g:
        if v not in cnt:
            vals.append(v)
            cnt[v] = 0
        cnt[v] += 1
    if len(vals) > 8:
        return None
    out = []
    for v in vals:
        j = len(out)
        while j > 0 and cnt[v] > cnt[out[j - 1]]:
            j -= 1
        out.insert(j, v)
    return out


INDEX_CODE = ((0, 2), (2, 2), (1, 3), (5, 3), (3, 4), (7, 4), (11, 4), (15, 4))     # QB3encode.h:600-601: no middle swap


def index_unit(g, rung, oldrung, nbytes):
    """Bits of the index form of a group at `rung`, None with more than eight distinct values (QB3encode.h:556-613)"""
    ub = UB[nbytes]
    table = index_table(g)
    if table is None:
        return None
    b = Bits().put(*S.signal_code(ub))
    b.put(*S.switch_noflag_code((1 << ub) - 1 - oldrung, ub))
    b.put(*S.switch_noflag_code(rung - oldrung, ub))
    for v in g:
        b.put(*INDEX_CODE[table.index(v)])
    for v in table:
        b.put(*_single(v, rung))
    return b


class Unit:
    """what best_unit says of a unit: bits (Bits), kind ('0' rung 0, 'N' plain, 'C' factor, 'I' index), rung, pcf (the band's factor
    less 2 behind it), cf (the group's factor: 0 at rung 0, 1 without one), size (the plain or factor form), thr, tried (the index form
    was looked at), idx (its bits: NO_INDEX with nine values or more, None where the rung forbids it), info (factor_unit's, or None)"""


def best_unit(g, oldrung, pcf, nbytes):
    """the unit the common-factor modes write for sixteen mag-sign deltas (QB3encode.h:676-713)"""
    ub = UB[nbytes]
    u = Unit()
    used = 0
    for v in g:
        used |= v
    u.rung = rung = S.topbit(used | 1)
    u.pcf, u.info, u.idx, u.tried, u.cf, u.thr = pcf, None, None, False, 0, 36 + 3 * ub + 2 * rung
    if used <= 1:
        u.bits = Bits().put(*S.switch_code(rung - oldrung, ub)).put(*S.rung0_code(g))
        u.kind, u.size = "0", u.bits.n
        return u
    u.cf = cf = gcf(g)
    if cf >= 2:
        u.bits, u.info = factor_unit(g, cf, pcf, oldrung, nbytes)
        u.kind = "C"
    else:
        u.bits, _ = S.unit_bits(g, oldrung, nbytes, True)
        u.kind = "N"
    u.size = u.bits.n
    if 3 < rung < 63:
        ib = index_unit(g, rung, oldrung, nbytes)
        u.idx = ib.n if ib is not None else NO_INDEX
        if u.size >= u.thr:
            u.tried = True
            # (a unit longer than NO_INDEX with nine values or more is where the reference drops the unit: SURVEY B-2)
            assert ib is not None or u.size <= NO_INDEX, "a unit of %d bits with more than eight values" % u.size
            if u.idx < u.size:
                u.bits, u.kind = ib, "I"
                return u
    if cf >= 2:
        u.pcf = cf - 2
    return u


def encode_band(units, nbytes, oldrung=0, pcf=0):
    """[Unit] of a band's groups in turn, from the entering rung and factor"""
    out = []
    for g in units:
        u = best_unit(g, oldrung, pcf, nbytes)
        out.append(u)
        oldrung, pcf = u.rung, u.pcf
    return out


def encode_bands(bands, nbytes, state=None):
    """([[Unit] a band], Bits of the raster's stream: blocks in turn, bands within a block) of per-band group sequences of one length;
    state: [(rung, factor less 2) a band] entering"""
    state = state or [(0, 0)] * len(bands)
    per = [encode_band(gs, nbytes, *st) for gs, st in zip(bands, state)]
    b = Bits()
    for k in range(len(bands[0])):
        for c in range(len(bands)):
            b.extend(per[c][k].bits)
    return per, b


def bands_to_raster(bands, nbytes, ncols, cband=None, order=HILBERT, prev=None):
    """(raster [4 rows, 4 ncols, bands] of unsigned values, [last value a band]): the raster whose 4x4 blocks, in block-raster order,
    have the mag-sign deltas bands[c][k] in band c once the band map is applied (band c less band cband[c], modulo the width, where
    cband[c] != c) and the block is walked along `order`, from the entering values `prev` (zeros: a fresh encoder)"""
    nb = len(bands)
    n = len(bands[0])
    assert all(len(b) == n for b in bands) and n % ncols == 0
    nbits = 8 * nbytes
    mask = (1 << nbits) - 1
    cband = list(range(nb)) if cband is None else cband
    diff = np.zeros((4 * (n // ncols), 4 * ncols, nb), dtype=np.uint64)
    last = list(prev) if prev is not None else [0] * nb
    for c in range(nb):
        p = last[c]
        for k, g in enumerate(bands[c]):
            by, bx = divmod(k, ncols)
            for i, d in enumerate(g):
                p = (p + S.smag(d, nbits)) & mask
                nib = (order >> (60 - 4 * i)) & 15
                diff[4 * by + (nib >> 2), 4 * bx + (nib & 3), c] = p
        last[c] = p
    img = diff.copy()
    for c in range(nb):
        if cband[c] != c:
            assert cband[cband[c]] == cband[c], "a band is subtracted from a core band"
            img[..., c] = (diff[..., c] + diff[..., cband[c]]) & np.uint64(mask)
    return img, last
