"""The code rule of tests/qb3_spec.py, pinned before anything is compared with it: the codes invert, and the unit streams the
oracle writes for 4n x 4 x 1 rasters (FTL and BASE, every width, rungs across each width's range) are, bit for bit, what the
rule writes for the same deltas.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_spec as S  # noqa: E402
from qb3_table_spec import oracle_units  # noqa: E402

FTL, BASE = 8, 4
WIDTHS = {1: 0, 2: 2, 4: 4, 8: 6}            # bytes -> unsigned QB3 type


def edge_values(r):
    top, half = 1 << r, 1 << (r - 1)
    return sorted(v for v in {0, 1, half - 1, half, top - 2, top - 1, top, top + 1, 2 * top - 1} if 0 <= v < 2 * top)


@pytest.mark.parametrize("nbytes", [1, 2, 4, 8])
def test_value_codes_invert(nbytes):
    for r in range(1, 8 * nbytes):
        for v in edge_values(r):
            c, ln = S.code_value(v, r)
            assert ln == r + (v >= 1 << (r - 1)) + (v >= 1 << r) and c < 1 << ln
            for pos in (0, 5, 31, 63):
                junk = 0x5A5A5A5A5A5A5A5A5A5A << (pos + ln)
                assert S.decode_value(c << pos | junk, pos, r) == (v, ln), (r, v, pos)
            assert S.swap(S.swap(v, r), r) == v
    c, ln = S.code_value((1 << 64) - 1, 63)      # the longest code: 65 bits
    assert ln == 65 and c == (1 << 65) - 1


@pytest.mark.parametrize("ub", [3, 4, 5, 6])
def test_switch_codes_invert(ub):
    n = 1 << ub
    lens = set()
    for d in range(n):
        c, ln = S.switch_code(d, ub)
        if d == 0:
            assert (c, ln) == (0, 1)
            continue
        assert c & 1 and ln <= ub + 2
        delta, sig, l2 = S.decode_switch_noflag(c >> 1 | 0xF00 << (ln - 1), 0, ub)
        assert (delta, sig, l2) == (d, False, ln - 1)
        lens.add(ln)
    assert lens == {ub, ub + 1, ub + 2}
    c, ln = S.switch_noflag_code(0, ub)
    assert S.decode_switch_noflag(c, 0, ub) == (0, True, ln)


def test_rung0_and_step():
    rng = np.random.default_rng(1)
    assert S.rung0_code([0] * 16) == (0, 1)
    g = [int(x) for x in rng.integers(0, 2, 16)]
    c, ln = S.rung0_code(g)
    assert ln == 17 and S.decode_group(c, 0, 0, 1, False) == (g, 17)
    for r in (1, 7, 8, 31, 63):
        for n in range(17):              # every rung-bit prefix 1^n 0^(16-n)
            g = [(1 << r) | int(x) if i < n else int(x) for i, x in enumerate(rng.integers(0, 1 << min(r, 20), 16))]
            if n == 0:
                g[5] |= 1 << r           # (a group at rung r has its rung bit somewhere)
            assert S.step_undo(S.step_apply(g, r), r) == g, (r, n)
        g = [int(x) for x in rng.integers(0, 1 << min(r, 20), 16)]
        g[3] |= 1 << r
        g[9] |= 1 << r                   # not a prefix: untouched
        assert S.step_apply(g, r) == g and S.step_undo(g, r) == g


def test_lay_at_any_offset():
    rng = np.random.default_rng(2)
    b = S.Bits()
    for r in (3, 18, 63):
        b.extend(S.group_codes([int(x) for x in rng.integers(0, 1 << min(r, 30), 16)], r, False))
    for off in range(64):
        w = S.lay(b.v, b.n, off, (off + b.n + 31) // 32 + 2, fill=True, rng=rng)
        assert (S.int_of(w) >> off) & ((1 << b.n) - 1) == b.v


def _units_for_rungs(nbytes, rungs, rng):
    """one block a rung: mag-sign deltas whose largest has its top bit at the rung, with 2^r and 2^r - 1 among them; rung 0 alternates the
    two rung-0 forms; every third block's rung bits are a prefix 1^n 0^(16-n) (the step)"""
    units = []
    for k, r in enumerate(rungs):
        if r == 0:
            units.append([0] * 16 if k % 2 else [int(x) for x in rng.integers(0, 2, 16)])
            continue
        g = [int(x) for x in rng.integers(0, 1 << r, 16, dtype=np.uint64)] if r < 63 else \
            [int(x) for x in rng.integers(0, 1 << 62, 16, dtype=np.uint64)]
        g[int(rng.integers(0, 16))] |= 1 << r
        g[(k + 3) % 16] = 1 << r
        g[(k + 7) % 16] = (1 << r) - 1
        if k % 3 == 0:
            n = 1 + k % 16
            g = [v | (1 << r) if i < n else v & ~(1 << r) for i, v in enumerate(g)]
        units.append(g)
    return units


def _rungs(nbytes):
    top = 8 * nbytes - 1
    base = list(range(top + 1)) if nbytes <= 2 else [0, 1, 2, 3, 5, 7, 8, 9, 12, 15, 16, 17, 18, 19, 20, 24, 29, 30, 31]
    if nbytes == 8:
        base += [32, 33, 34, 40, 44, 45, 46, 47, 55, 61, 62, 63]
    # down and up again: every switch length, the wrap of the switch modulo 2^UB
    return base + base[::-1] + [top, 0, top, 1]


def oracle_raw_bits(oracle, img, dtype, mode):
    e = oracle.Encoder(img.shape[1], img.shape[0], 1, dtype)
    e.set_mode(mode)
    dst = np.zeros(e.max_size() + 64, dtype=np.uint8)
    src = np.ascontiguousarray(img.reshape(img.shape[0], img.shape[1], 1))
    nbits = oracle.lib.qb3o_encode_raw(e.p, oracle._p(src), oracle._p(dst))
    assert nbits, "oracle raw encode failed"
    return S.int_of(dst) & ((1 << nbits) - 1), nbits


@pytest.mark.parametrize("mode", [FTL, BASE], ids=["FTL", "BASE"])
@pytest.mark.parametrize("nbytes", [1, 2, 4, 8])
def test_spec_writes_the_oracles_units(oracle, nbytes, mode):
    rng = np.random.default_rng(10 * nbytes + mode)
    units = _units_for_rungs(nbytes, _rungs(nbytes), rng)
    img = S.block_to_raster(units, nbytes).astype(oracle.NPTYPE[WIDTHS[nbytes]])
    got, nbits = oracle_raw_bits(oracle, img, WIDTHS[nbytes], mode)
    want, old = S.Bits(), 0
    for g in units:
        b, old = S.unit_bits(g, old, nbytes, mode == BASE)
        want.extend(b)
    assert nbits == want.n, (nbits, want.n)
    diff = got ^ want.v
    assert diff == 0, "first differing bit %d of %d" % ((diff & -diff).bit_length() - 1, nbits)
    # and the rule's reader takes the oracle's bits back to the deltas
    pos, old = 0, 0
    for g in units:
        if got >> pos & 1:
            delta, sig, ln = S.decode_switch_noflag(got, pos + 1, S.UB[nbytes])
            assert not sig
            pos += 1 + ln
        else:
            delta = 0
            pos += 1
        r = (old + delta) % (1 << S.UB[nbytes])
        dec, pos = S.decode_group(got, pos, r, nbytes, mode == BASE)
        assert dec == (g if max(g) > 1 else [v & 1 for v in g]), (r, pos)
        old = r
    assert pos == nbits


@pytest.mark.parametrize("nbytes", [1, 2, 4, 8])
def test_unit_rasters_reach_every_form(oracle, nbytes):
    """the rasters tests/test_bit_readers.py decodes unit by unit hold what they are meant to: in the common-factor stream, factors
    that come with the unit and factors kept from the unit before, index units, rung 0 both ways; in the plain stream, rungs 17..20,
    30..34 and 44..47 where the width has them, and rung 63; every unit of a common-factor stream under 800 bits (SURVEY B-2)"""
    for best in (False, True):
        img = S.unit_raster(nbytes, False, best, 3)
        _, n, rows = oracle_units(oracle, img, WIDTHS[nbytes], 5 if best else FTL)
        kinds = {k for _, k, _, _, _ in rows}
        rungs = {r for _, k, r, _, _ in rows if k in "N0"}
        ends = [a for a, _, _, _, _ in rows[1:]] + [n]
        if best:
            assert {"C", "I", "N"} <= kinds, kinds
            own = [c - 2 != p for _, k, _, c, p in rows if k == "C"]
            assert any(own) and not all(own), "factors of their own and kept factors"
            assert max(e - a for e, (a, _, _, _, _) in zip(ends, rows)) < 800
        else:
            want = {r for r in (17, 18, 19, 20, 30, 31, 32, 33, 34, 44, 45, 46, 47) if r < 8 * nbytes} | {8 * nbytes - 1}
            assert want <= rungs, sorted(want - rungs)
        assert 0 in rungs
