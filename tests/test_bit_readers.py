"""The device bit readers, value by value, against the code rule (tests/qb3_spec.py, pinned to the oracle by test_qb3_spec.py).

libqb3probe.so (qb3_amd/csrc/probe_readers.hip, a test instrument) runs the product's own readers in plain kernels: get_value + unswap
through ReaderT over global memory and out of LDS, get_group, dec3_group with and without the window, wide_values_lds, and parse_unit
over whole unit streams.  One launch a primitive and width covers the sweep: every rung (rung 0 included), every start bit 0..63 -- so
that the sixteenth value of a group begins on a multiple of 32 for some start, the round-4 fault's place --, values of all three code
forms with 2^r and 2^r - 1 among them, 65-bit codes at rung 63, streams that end inside a read.  Each sweep runs three times on the
same stream: as is, and right after probe_dirty has filled LDS and registers with each of two patterns.  Any difference between the
runs or from the rule fails.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_probe as P  # noqa: E402
import qb3_spec as S  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERNS = (0xDEADBEEF, 0x0F0F5A5A)
TOO_BIG = 0xFFFFFFFF
NVALS = 20


@pytest.fixture(scope="module")
def probe(qb3):
    import torch
    torch.cuda.init()
    return P.load()


_stream = P.stream


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def runs(probe, launch, out, also=None):
    """launch() three times on the same inputs: as is, then right after probe_dirty with each pattern; returns the three outputs
    (with `also`: pairs of out and also)"""
    import torch
    res = []
    for pat in (None,) + PATTERNS:
        out.fill_(-1 if out.dtype == torch.int64 else 0x5A)
        if pat is not None:
            P.dirty(pat)
        assert launch() == 0
        torch.cuda.synchronize()
        res.append(out.cpu().numpy().copy() if also is None else (out.cpu().numpy().copy(), also.cpu().numpy().copy()))
    return res


class Layout:
    """lanes laid one after the other in one buffer of dwords: each lane's bits from its start bit, random bits between lanes
    (every lane region begins on a multiple of 64, then the lane's start bit modulo 64)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.parts, self.base, self.starts, self.ends, self.at = [], [], [], [], 0

    def add(self, bits, nbits, off, cut=None):
        """a lane of `nbits` bits at `off` bits into a fresh 64-bit aligned region; cut: the stream ends that many bits in"""
        nw = (off + nbits + 31) // 32 + 2
        nw += nw & 1
        w = S.lay(bits, nbits, off, nw, fill=True, rng=self.rng)
        self.parts.append(w)
        self.base.append(32 * self.at)
        self.starts.append(32 * self.at + off)
        self.ends.append(32 * self.at + off + (nbits if cut is None else cut))
        self.at += nw

    def lane(self, i):
        """(the stream int of lane i's region, the stream bit the region begins at)"""
        return S.int_of(self.parts[i]), self.base[i]

    def arrays(self):
        return (np.concatenate(self.parts), np.array(self.starts, dtype=np.uint64), np.array(self.ends, dtype=np.uint64))


def value_lanes(nbytes, seed):
    """every rung (0 .. 8 * nbytes - 1) at every start bit; a rung's twenty values are the same at every start.  Every sixteenth lane of
    a rung is cut: its stream ends on the dword boundary inside its later codes (what follows is random and must read as zeros)."""
    rng = np.random.default_rng(seed)
    lay = Layout(seed + 1)
    rungs, want, cuts = [], [], []
    for r in range(8 * nbytes):
        if r == 0:
            vals = [int(x) for x in rng.integers(1, 1 << 16, NVALS)]
            vals[3] = vals[11] = 0
            b = S.Bits()
            for v in vals:
                b.put(*(((v << 1) | 1, 17) if v else (0, 1)))
        else:
            top = 1 << r
            vals = [int(x) % (2 * top) for x in rng.integers(0, 1 << 63, NVALS, dtype=np.uint64)]
            vals[0:9] = [top, top - 1, 0, 2 * top - 1, top >> 1, (top >> 1) - 1, top + 1, top - 2 if r > 1 else 1, 1]
            vals[15] = top if r % 2 else top - 1           # the sixteenth value, around the swap
            b = S.Bits()
            for v in vals:
                b.put(*S.code_value(S.swap(v, r), r))
        for off in range(64):
            cut = None
            if off % 16 == 5:
                cut = (off + b.n // 2 + 31) // 32 * 32 - off     # the stream ends on a dword boundary halfway in
            lay.add(b.v, b.n, off, cut)
            rungs.append(r)
            cuts.append(cut)
            want.append(vals)
    words, starts, ends = lay.arrays()
    return words, starts, ends, np.array(rungs, dtype=np.uint32), want, cuts, lay


@pytest.mark.parametrize("nbytes", [1, 2, 4, 8])
def test_value_reads_match_the_code_rule(probe, nbytes):
    """get_value<T> + unswap through ReaderT, global memory and LDS: every rung at every start bit, 20 values a lane, cut streams"""
    import torch
    words, starts, ends, rungs, want, cuts, lay_ = value_lanes(nbytes, 100 + nbytes)
    n = len(starts)
    d_words, d_s, d_e, d_r = _dev(words), _dev(starts), _dev(ends), _dev(rungs)
    out = torch.empty(n * (NVALS + 1), dtype=torch.int64, device="cuda")
    expect = []
    for i in range(n):
        bits, base = lay_.lane(i)
        vals, pos = _spec_from_int(bits & ((1 << (int(ends[i]) - base)) - 1), int(starts[i]) - base, int(rungs[i]))
        pos += base
        if cuts[i] is None:
            assert vals == want[i], "the rule does not read back what it wrote"
        expect.append(vals + [pos])
    expect = np.array(expect, dtype=np.uint64).reshape(-1)
    for lds in (0, 1):
        res = runs(probe, lambda: probe.probe_values(C.c_void_p(d_words.data_ptr()), len(words), C.c_void_p(d_s.data_ptr()),
                                                    C.c_void_p(d_e.data_ptr()), C.c_void_p(d_r.data_ptr()), n, NVALS, nbytes, lds,
                                                    C.c_void_p(out.data_ptr()), _stream()), out)
        for k, got in enumerate(res):
            got = got.view(np.uint64)
            assert TOO_BIG not in got.reshape(n, NVALS + 1)[:, NVALS], "a workgroup's lanes did not fit the staging"
            bad = np.nonzero(got != expect)[0]
            if len(bad):
                lane, j = divmod(int(bad[0]), NVALS + 1)
                pytest.fail("%s, run %s: %d words differ; first: lane %d (rung %d, start bit %d, cut %s), %s: got %#x, rule %#x" % (
                    "LDS" if lds else "global", ("clean", "dirty A", "dirty B")[k], len(bad), lane, rungs[lane], starts[lane] % 64,
                    cuts[lane], "end bit" if j == NVALS else "value %d" % j, got[bad[0]], expect[bad[0]]))


def _spec_from_int(bits, pos, r):
    out = []
    for _ in range(NVALS):
        if r == 0:
            if (bits >> pos) & 1:
                out.append((bits >> (pos + 1)) & 0xFFFF)
                pos += 17
            else:
                out.append(0)
                pos += 1
        else:
            v, ln = S.decode_value(bits, pos, r)
            out.append(S.swap(v, r))
            pos += ln
    return out, pos


def group_lanes(nbytes, step, seed):
    """one group a rung (the same at every start bit 0..63), a sixteenth value in each form; every third rung's rung bits a
    prefix 1^n 0^(16-n) (the step)"""
    rng = np.random.default_rng(seed)
    lay = Layout(seed + 1)
    rungs, groups = [], []
    for r in range(8 * nbytes):
        if r == 0:
            g = [int(x) for x in rng.integers(0, 2, 16)] if nbytes != 2 else [0] * 16     # (both rung-0 forms)
        else:
            top = 1 << r
            g = [int(x) % (2 * top) for x in rng.integers(0, 1 << 63, 16, dtype=np.uint64)]
            g[2], g[6] = top, top - 1
            g[15] = (top, top - 1, 2 * top - 1, 0)[r % 4]
            g[int(rng.integers(0, 16))] |= top
            if r % 3 == 0:
                n = 1 + r % 16
                g = [v | top if i < n else v & ~top for i, v in enumerate(g)]
        b = S.group_codes(g, r, step)
        for off in range(64):
            lay.add(b.v, b.n, off)
            rungs.append(r)
            groups.append((g, b.n))
    words, starts, ends = lay.arrays()
    return words, starts, ends, np.array(rungs, dtype=np.uint32), groups


@pytest.mark.parametrize("step", [False, True], ids=["FTL", "STEP"])
@pytest.mark.parametrize("nbytes", [1, 2, 4, 8])
def test_group_reads_match_the_code_rule(probe, nbytes, step):
    """sixteen values through get_group (global, LDS), dec3_group without the window (global, LDS) and, for 32/64-bit data, with it
    and wide_values_lds (rungs 8 and up): every rung at every start bit, with and without the step"""
    import torch
    words, starts, ends, rungs, groups = group_lanes(nbytes, step, 200 + 2 * nbytes + step)
    n = len(starts)
    nbits = 8 * nbytes
    d_words, d_s, d_e, d_r = _dev(words), _dev(starts), _dev(ends), _dev(rungs)
    out = torch.empty(n * 17, dtype=torch.int64, device="cuda")
    gs = np.array([g + [int(s) + ln] for (g, ln), s in zip(groups, starts)], dtype=np.uint64)   # values, end bit
    runs_ = gs.copy()
    acc = np.zeros(n, dtype=object)
    for k in range(16):                             # dec3_group: the values accumulated by smag
        acc = [(a + S.smag(int(v), nbits)) & ((1 << nbits) - 1) for a, v in zip(acc, gs[:, k])]
        runs_[:, k] = np.array(acc, dtype=np.uint64)
    # rung 0: the sixteen values are the bits (mag-sign 0 / 1), the group as written
    paths = [(0, 0), (0, 1), (1, 0), (1, 1)] + ([(2, 1), (3, 1)] if nbytes >= 4 else [])
    for path, lds in paths:
        expect = runs_ if path in (1, 2) else gs
        sel = np.ones(n, dtype=bool) if path != 3 else rungs >= 8
        res = runs(probe, lambda: probe.probe_groups(C.c_void_p(d_words.data_ptr()), len(words), C.c_void_p(d_s.data_ptr()),
                                                    C.c_void_p(d_e.data_ptr()), C.c_void_p(d_r.data_ptr()), n, nbytes, int(step), path,
                                                    lds, C.c_void_p(out.data_ptr()), _stream()), out)
        for k, got in enumerate(res):
            got = got.view(np.uint64).reshape(n, 17)
            assert TOO_BIG not in got[:, 16], "a workgroup's lanes did not fit the staging"
            bad = np.nonzero((got != expect)[sel].any(axis=1))[0]
            if len(bad):
                lane = int(np.nonzero(sel)[0][bad[0]])
                j = int(np.nonzero(got[lane] != expect[lane])[0][0])
                pytest.fail("path %d %s, run %s: %d lanes differ; first: lane %d (rung %d, start bit %d), %s: got %#x, rule %#x" % (
                    path, "LDS" if lds else "global", ("clean", "dirty A", "dirty B")[k], len(bad), lane, rungs[lane], starts[lane] % 64,
                    "end bit" if j == 16 else "value %d" % j, got[lane, j], expect[lane, j]))


UNIT_TYPES = [(1, False), (2, False), (4, True), (4, False), (8, True), (8, False)]


@pytest.mark.parametrize("mode", [8, 4, 5], ids=["FTL", "BASE", "BEST"])
@pytest.mark.parametrize("t", UNIT_TYPES, ids=["u8", "u16", "i32", "u32", "i64", "u64"])
def test_unit_streams_decode_at_every_offset(probe, oracle, t, mode):
    """parse_unit<T, FTL | BASE | BEST> over the oracle's unit stream of a 4n x 4 x 1 raster holding every unit form (tests/qb3_spec.py
    unit_raster; test_qb3_spec.py checks that it does), laid at each of the 64 bit offsets, from global memory and from LDS: every copy
    decodes to the raster, ends where the stream ends, on a clean device and after probe_dirty"""
    import torch
    nbytes, signed = t
    best = mode == 5
    img = S.unit_raster(nbytes, signed, best, 3 + signed)
    dt = {(1, False): 0, (2, False): 2, (4, True): 5, (4, False): 4, (8, True): 7, (8, False): 6}[t]
    e = oracle.Encoder(img.shape[1], 4, 1, dt)
    e.set_mode(mode)
    oracle.lib.qb3o_set_fix_b2(e.p, 1)                  # (no unit dropped whatever its length: the raster is the decode's truth)
    dst = np.zeros(e.max_size() + 64, dtype=np.uint8)
    nb = oracle.lib.qb3o_encode_raw(e.p, oracle._p(np.ascontiguousarray(img.reshape(4, -1, 1))), oracle._p(dst))
    assert nb
    bits = S.int_of(dst) & ((1 << nb) - 1)
    lay = Layout(300 + nbytes)
    for off in range(64):
        lay.add(bits, nb, off)
    words, starts, ends = lay.arrays()
    w = img.shape[1]
    d_words, d_s, d_e = _dev(words), _dev(starts), _dev(ends)
    out = torch.empty(64 * 4 * w * nbytes, dtype=torch.uint8, device="cuda")
    ok = torch.empty(64, dtype=torch.int32, device="cuda")
    want = np.ascontiguousarray(img).view(np.uint8).reshape(-1)
    cm = {8: 0, 4: 1, 5: 2}[mode]
    for lds in (0, 1):
        res = runs(probe, lambda: probe.probe_units(C.c_void_p(d_words.data_ptr()), len(words), C.c_void_p(d_s.data_ptr()),
                                                   C.c_void_p(d_e.data_ptr()), 64, w, nbytes, cm, lds, C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(ok.data_ptr()), _stream()), out, ok)
        for k, (got, oks) in enumerate(res):
            oks = oks.view(np.uint32)
            assert (oks == 1).all(), ("LDS" if lds else "global", ("clean", "dirty A", "dirty B")[k],
                                      "parse failed or ended elsewhere at offsets", np.nonzero(oks != 1)[0][:8], oks[oks != 1][:8])
            got = got.reshape(64, -1)
            bad = [o for o in range(64) if not np.array_equal(got[o], want)]
            assert not bad, "%s, run %s: offsets %s decode wrong (first value at %d)" % (
                "LDS" if lds else "global", ("clean", "dirty A", "dirty B")[k], bad[:8], int(np.nonzero(got[bad[0]] != want)[0][0]) // nbytes)
