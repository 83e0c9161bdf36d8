"""tests/qb3_spec.py -- the QB3 code rule, bit for bit, in plain Python integers (test infrastructure, no GPU).

What the device readers are held to (tests/test_bit_readers.py), written from the reference's rules and pinned against the
oracle's streams by tests/test_qb3_spec.py before anything is compared with it:
- one value at rung r >= 1: short r bits (.x0), middle r + 1 (.01), long r + 2 (.11) -- reference QB3decode.h:119-129,
  QB3encode.h:132-141; at rung 63 the long code is 65 bits
- the middle swap of group values at rungs 1..7 (2^r <-> 2^r - 1), and of single values (common factors) at rungs 3..7
- the rung-switch code and its "signal" (QB3decode.h:97-116, QB3encode.h:79-89)
- rung 0: a flag, then sixteen bits when it is set (QB3decode.h:150-160)
- the step and its undo (QB3encode.h:169-176, QB3decode.h:285-289)
A stream is an int whose bit i is stream bit i (LSB first, as the dwords hold it).
"""
import numpy as np

UB = {1: 3, 2: 4, 4: 5, 8: 6}           # rung-switch unit bits by bytes per value
HILBERT = 0x01548CD9AEFB7623            # reference QB3common.h:193


def code_value(v, r):
    """(code, length) of value v at rung r >= 1, no swap"""
    half, top = 1 << (r - 1), 1 << r
    assert 0 <= v < 2 * top
    if v < half:
        return v << 1, r
    if v < top:
        return ((v - half) << 2) | 1, r + 1
    return ((v - top) << 2) | 3, r + 2


def decode_value(bits, pos, r):
    """(value, length) of the code at bit `pos` of stream `bits`, rung r >= 1, no swap"""
    x = bits >> pos
    top, half = 1 << r, 1 << (r - 1)
    if not x & 1:
        return (x & (top - 1)) >> 1, r
    if not x & 2:
        return ((x >> 2) & (half - 1)) | half, r + 1
    return ((x >> 2) & (top - 1)) | top, r + 2


def swap(v, r):
    """the middle swap of group values (rungs 1..7); its own inverse"""
    top = 1 << r
    return v ^ (2 * top - 1) if 1 <= r < 8 and v in (top, top - 1) else v


def swap_single(v, r):
    """single values (common factors): swapped at rungs 3..7 only (QB3encode.h:144-150)"""
    return swap(v, r) if r >= 3 else v


def switch_code(delta, ub):
    """(code, length) of the rung switch for delta in [0, 2^ub), change flag in bit 0"""
    n = 1 << ub
    delta %= n
    if delta == 0:
        return 0, 1
    m = 2 * (delta - 1) if delta < n // 2 else 2 * (n - delta) - 1
    c, ln = code_value(m, ub - 1)
    return (c << 1) | 1, ln + 1


def signal_code(ub):
    """the switch code that never stands for a delta (m = 2^ub - 2): opens the common-factor and index forms"""
    c, ln = code_value((1 << ub) - 2, ub - 1)
    return (c << 1) | 1, ln + 1


def switch_noflag_code(delta, ub):
    """a switch without its change flag, the signal standing in for "no change" (QB3encode.h:300-305)"""
    c, ln = switch_code(delta, ub) if delta % (1 << ub) else signal_code(ub)
    return c >> 1, ln - 1


def decode_switch_noflag(bits, pos, ub):
    """(delta, signal, length) of a switch code without its flag at `pos`"""
    n = 1 << ub
    m, ln = decode_value(bits, pos, ub - 1)
    if m == n - 2:
        return 0, True, ln
    return ((n - (m + 1) // 2) % n if m & 1 else m // 2 + 1), False, ln


def rung0_code(g):
    """(code, length) of a rung-0 group: a flag, the low bits of the sixteen values when any is set"""
    bits = sum((v & 1) << i for i, v in enumerate(g))
    return (1 | bits << 1, 17) if bits else (0, 1)


def step_apply(g, r):
    """the encoder's step (a copy): the rung bits 1^n 0^(16-n), n >= 1, lose their last 1"""
    g = list(g)
    rb = sum(((v >> r) & 1) << i for i, v in enumerate(g))
    if rb and rb & (rb + 1) == 0:
        n = bin(rb).count("1")
        g[n - 1] ^= 1 << r
    return g


def step_undo(g, r):
    """the decoder's undo (a copy): rung bits 1^m 0^(16-m) get bit m back"""
    g = list(g)
    rb = sum(((v >> r) & 1) << i for i, v in enumerate(g))
    if rb & (rb + 1) == 0:
        m = bin(rb).count("1")
        if m < 16:
            g[m] ^= 1 << r
    return g


def topbit(v):
    return max(v.bit_length() - 1, 0)


def mags(v, nbits):
    """mag-sign of the two's complement value v (QB3common.h:127-130)"""
    v &= (1 << nbits) - 1
    return ((v << 1) ^ -(v >> (nbits - 1))) & ((1 << nbits) - 1)


def smag(v, nbits):
    return ((v >> 1) ^ -(v & 1)) & ((1 << nbits) - 1)


class Bits:
    """LSB-first bit builder: put(code, length) appends"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, code, length):
        assert 0 <= code < (1 << length) or length == 0
        self.v |= code << self.n
        self.n += length
        return self

    def extend(self, other):
        return self.put(other.v, other.n)


def group_codes(g, r, step):
    """Bits of sixteen mag-sign values at rung r (0: the flag form); the step applied first when `step`"""
    b = Bits()
    if r == 0:
        return b.put(*rung0_code(g))
    for v in (step_apply(g, r) if step else g):
        b.put(*code_value(swap(v, r), r))
    return b


def unit_bits(g, oldrung, nbytes, step):
    """A plain unit (FTL / BASE; QB3encode.h:439-441): switch from oldrung, then the group.  Returns (Bits, rung)."""
    used = 0
    for v in g:
        used |= v
    r = topbit(used | 1)
    b = Bits().put(*switch_code(r - oldrung, UB[nbytes]))
    return b.extend(group_codes(g, r if used > 1 else 0, step)), r


def block_to_raster(units, nbytes, order=HILBERT):
    """4n x 4 raster (rows of w values, uint) whose blocks, from an entering value of 0, have the mag-sign deltas `units`"""
    nbits = 8 * nbytes
    w = 4 * len(units)
    img = np.zeros((4, w), dtype=np.uint64)
    prev = 0
    for bx, g in enumerate(units):
        for i, d in enumerate(g):
            prev = (prev + smag(d, nbits)) & ((1 << nbits) - 1)
            nib = (order >> (60 - 4 * i)) & 15
            img[nib >> 2, 4 * bx + (nib & 3)] = prev
    return img


def decode_group(bits, pos, r, nbytes, step, end=None):
    """(sixteen mag-sign values, bit behind them) of a group at rung r read at `pos`; bits at and past `end` read as zeros"""
    if end is not None:
        bits &= (1 << end) - 1
    if r == 0:
        if not (bits >> pos) & 1:
            return [0] * 16, pos + 1
        x = (bits >> (pos + 1)) & 0xFFFF
        return [(x >> i) & 1 for i in range(16)], pos + 17
    g = []
    for _ in range(16):
        v, ln = decode_value(bits, pos, r)
        g.append(swap(v, r))
        pos += ln
    return (step_undo(g, r) if step else g), pos


def lay(bits, nbits, offset, nwords, fill=None, rng=None):
    """dwords holding `nbits` bits of `bits` from stream bit `offset`; the bits around them are zeros, or random when `fill`"""
    total = 32 * nwords
    assert offset + nbits <= total
    mask = ((1 << nbits) - 1) << offset
    v = (bits << offset) & mask
    if fill:
        junk = int.from_bytes(rng.bytes(4 * nwords), "little")
        v |= junk & ~mask & ((1 << total) - 1)
    return np.frombuffer(v.to_bytes(4 * nwords, "little"), dtype=np.uint32).copy()


def int_of(words):
    """the stream int of an array of dwords (or bytes)"""
    return int.from_bytes(np.ascontiguousarray(words).tobytes(), "little")


def unit_raster(nbytes, signed, best, seed):
    """A 4n x 4 raster of one band whose unit stream holds every form a reader meets: plain units at each width's rungs (17..20,
    30..34, 44..47 where the width has them; rung 63 for FTL / BASE), rung-0 units of both kinds, common-factor units that bring
    their own factor (small ones, coded at the group's rung, and large ones with a rung of their own) and units that keep the factor
    before them, index units (a few distinct values).  `best`: 64-bit rungs stay at 47 and below, so that no common-factor or index
    unit reaches 800 bits (SURVEY B-2).  Returns a (4, w) array of the QB3 type's numpy dtype."""
    rng = np.random.default_rng(seed)
    bits = 8 * nbytes
    mask = (1 << bits) - 1
    base = 1 << (bits - 1)
    top = min(bits - 1, 47) if best and nbytes == 8 else bits - 1
    rungs = [k for k in [1, 2, 3, 4, 5, 6, 7, 8, 11, 14, 15, 16, 17, 18, 19, 20, 24, 30, 31, 32, 33, 34, 40, 44, 45, 46, 47, 52, 60, 62]
             if k <= top - 1]

    def rnd(k, n=16):
        return [int(x) for x in rng.integers(0, 1 << k, n, dtype=np.uint64)] if k < 64 else \
            [int(x) for x in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]

    # rung 0: no bit set (after a first block that enters the level), then the sixteen bits (deltas 0 and -1)
    blocks = [[base] * 16, [base] * 16, [base - (i + 1) // 3 for i in range(16)]]
    blocks += [[base + d for d in rnd(k)] for k in rungs]                          # plain units, rung k (deltas below 2^k)
    if not best and top == bits - 1:
        blocks += [rnd(bits) for _ in range(2)]                                    # the full range: rung bits - 1 (65-bit codes at 64)
    facs = [3, 5] if nbytes == 1 else [3, 257] if nbytes == 2 else [5, (1 << 20) + 3] if nbytes == 4 else [5, (1 << 24) + 1, (1 << 40) + 7]
    for c in facs:
        for k in [k for k in rungs if (k + (c.bit_length())) < bits - 2][-4:] + [2, 5]:
            m = base // c
            for _ in range(2):                                                     # the second keeps the factor of the first
                blocks.append([(c * (m + d)) for d in rnd(k)])
    for k in [k for k in rungs if k >= 5][::3]:
        pal = [base + d for d in rnd(k, 3)]
        blocks.append([pal[int(i)] for i in rng.integers(0, 3, 16)])              # index units
    blocks.append([base] * 16)
    # pixel values along the curve of each block
    w = 4 * len(blocks)
    img = np.zeros((4, w), dtype=np.uint64)
    for bx, vals in enumerate(blocks):
        for i, v in enumerate(vals):
            nib = (HILBERT >> (60 - 4 * i)) & 15
            img[nib >> 2, 4 * bx + (nib & 3)] = v & mask
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[nbytes]
    out = img.astype(dt)
    return out.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[nbytes]) if signed else out
