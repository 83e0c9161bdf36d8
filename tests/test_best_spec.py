"""The common-factor encoders' coding decision, held at its boundaries.

CPU: tests/qb3_best_spec.py (the rule in Python integers) writes the oracle's stream bit for bit, unit by unit of the oracle's
trace, for the decision rasters of tests/qb3_best_cells.py and for a few thousand random units a width, under both curves, the
band maps the kernels take and an entering state other than a fresh encoder's; the census finds every cell of the decision in each
width's raster.  GPU: each encoder family (the 8-bit lane-per-block kernel, the one-band front end of 16/32/64-bit data, the
unit-per-lane front end) codes those rasters to the oracle's bytes and the spec's units, and the containers decode four ways."""
import os
import sys
from math import gcd

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_spec as S  # noqa: E402
import qb3_best_spec as B  # noqa: E402
import qb3_best_cells as K  # noqa: E402
import qb3_table_spec as T  # noqa: E402

CF, CF_H, BEST = 1, 5, 7
WIDTHS = {1: 0, 2: 2, 4: 4, 8: 6}            # bytes -> unsigned QB3 type
NPTYPE = (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64)


def raster_of(bands_units, dtype, mode, cband=None, prev=None):
    """(the raster [h, w, bands] of the QB3 type, the values a next raster would be entered with)"""
    nbytes = T.TYPESIZE[dtype]
    img, last = B.bands_to_raster(bands_units, nbytes, K.NCOLS, T.band_map(len(bands_units), cband), T.curve_order(mode), prev)
    return np.ascontiguousarray(img.astype(T.UNSIGNED[dtype]).view(NPTYPE[dtype])), last


def check_against_trace(oracle, bands_units, dtype, mode, cband=None, encoder=None, state=None, prev=None):
    """the spec's units against the oracle's trace of the raster with those deltas -- start bit, kind, rung, factor, factor before, a
    row a unit with reference defect B-2 left as it is -- and its stream against the oracle's; returns the SpecCase"""
    nbytes = T.TYPESIZE[dtype]
    img, last = raster_of(bands_units, dtype, mode, cband, prev)
    stream, nbits, rows, st = T._raw_trace(oracle, img, dtype, mode, cband, encoder=encoder)
    sc = K.SpecCase(bands_units, nbytes, state)
    assert len(rows) == len(sc.starts), "a trace row a unit: %d rows, %d units" % (len(rows), len(sc.starts))
    first = int(rows[0, 0])
    before = [s[1] for s in state] if state else [0] * len(bands_units)
    for (pos, k, c), row in zip(sc.starts, rows):
        u = sc.per[c][k]
        want = (pos, u.kind, u.rung) + ((u.cf, before[c]) if u.kind != "0" else ())
        got = (int(row[0]) - first, str(T.KINDS[int(row[1])]), int(row[2])) + ((int(row[3]), int(row[4])) if u.kind != "0" else ())
        assert got == want, "block %d, band %d: the oracle's (start, kind, rung, factor, factor before) %r, the spec's %r; cells %s" % (
            k, c, got, want, sorted(sc.cells[c][k]))
        before[c] = u.pcf
    msg = sc.explain(stream >> first, nbits - first)
    assert msg is None, msg
    assert [(int(r), int(f)) for _, r, f in st] == sc.state, "the band state behind the raster"
    return sc, last


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_gcf_is_the_greatest_common_factor():
    rng = np.random.default_rng(4)
    for _ in range(3000):
        f = int(rng.integers(1, 1 << int(rng.integers(1, 40))))
        g = [K.ms(f * int(x)) for x in rng.integers(-1000, 1000, 16)]
        if not any(g):
            continue
        want = 0
        for v in g:
            want = gcd(want, B.magsabs(v))
        assert B.gcf(g) == want
    assert B.gcf([0] * 15 + [K.ms(-128)]) == 128 and B.gcf([K.ms(6), K.ms(-9)] + [0] * 14) == 3 and B.gcf([K.ms(6), 1] + [0] * 14) == 1
    assert [B.magsdiv(K.ms(v), 3) for v in (6, -6, 0, -3)] == [K.ms(2), K.ms(-2), 0, K.ms(-1)]


def test_index_table_order():
    """by descending count; among equal counts the value seen first comes first (the order is in the bytes)"""
    assert B.index_table([5] * 8 + [3] * 8) == [5, 3] and B.index_table([3] * 8 + [5] * 8) == [3, 5]
    assert B.index_table([1, 2, 2, 3, 3, 3] + [4] * 10) == [4, 3, 2, 1]
    assert B.index_table([7, 8, 9, 9] + [7] * 6 + [8] * 6) == [7, 8, 9]
    assert B.index_table(list(range(9)) + [0] * 7) is None and B.index_table(list(range(8)) + [0] * 8) == [0, 1, 2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("nbytes", [1, 2, 4, 8])
def test_spec_writes_the_oracles_decision_units(oracle, nbytes):
    """one band, Hilbert's curve: the decision raster (cells, runs, and all of it again in other states)"""
    check_against_trace(oracle, [K.case_units(nbytes)], WIDTHS[nbytes], CF_H)


@pytest.mark.parametrize("nbytes", [1, 2, 4, 8])
def test_spec_writes_the_oracles_random_units(oracle, nbytes):
    units = K.pad_to_rows(K.random_units(nbytes, 3000, 40 + nbytes), K.NCOLS)
    sc, _ = check_against_trace(oracle, [units], WIDTHS[nbytes], CF_H)
    kinds = {u.kind for u in sc.per[0]}
    assert kinds == {"0", "N", "C", "I"}


@pytest.mark.parametrize("case", [(0, 3, None, CF_H), (0, 3, [0, 1, 2], CF), (1, 4, None, CF), (0, 2, [0, 1], CF_H), (3, 3, None, CF), (2, 5, [1, 1, 1, 3, 4], CF_H),
                                  (5, 2, [0, 1], CF), (4, 1, None, CF), (7, 2, [0, 0], CF_H), (6, 1, None, CF)],
                         ids=lambda c: "t%d-x%d-%s-m%d" % (c[0], c[1], "default" if c[2] is None else "".join(map(str, c[2])), c[3]))
def test_spec_with_band_maps_curves_and_entering_state(oracle, case):
    """several bands (each the sequence turned by another amount) under the default map of 3 and 4 bands, the identity and explicit
    maps, both curves; then a second, different raster on the same encoder: it is entered with the first one's values, rungs and
    factors"""
    dtype, bands, cband, mode = case
    nbytes = T.TYPESIZE[dtype]
    seq = K.case_units(nbytes)[:20 * K.NCOLS]
    first = K.rotated(seq, bands)
    second = [b[::-1] for b in K.rotated(seq[7:] + seq[:7], bands)]
    h, w = 4 * len(seq) // K.NCOLS, 4 * K.NCOLS
    e = oracle.Encoder(w, h, bands, dtype)
    e.set_mode(mode)
    if cband is not None:
        e.set_coreband(cband)
    sc, last = check_against_trace(oracle, first, dtype, mode, cband, encoder=e)
    assert any(f for _, f in sc.state), "the first raster leaves a factor"
    sc2, _ = check_against_trace(oracle, second, dtype, mode, cband, encoder=e, state=sc.state, prev=last)
    fresh = K.SpecCase(second, nbytes)
    assert fresh.bits.v != sc2.bits.v, "the entering state is in the second raster's bits"


@pytest.mark.parametrize("nbytes", [1, 2, 4, 8])
def test_every_cell_of_the_decision_is_in_the_raster(nbytes):
    _, census = K.decision_units(nbytes)
    required, absent = K.required(nbytes)
    missing = [c for c in required if c not in census.cells]
    assert not missing, missing
    # what a width cannot have it does not have: the reasons in required() are not excuses for a search that gave up
    assert not [c for c in absent if c in census.cells]
    # and the raster the tests use holds the same units at its front, entered from the same state
    sc = K.SpecCase([K.case_units(nbytes)], nbytes)
    have = set().union(*sc.cells[0])
    assert not [c for c in required if c not in have]


@pytest.mark.parametrize("nbytes", [4, 8])
def test_runs_of_small_magnitudes(nbytes):
    """192 consecutive factor units below 2^23 (two groups of 64 at any alignment), reaching 2^23 - 1; then 192 in which each 64th goes
    past 2^23 (every group of 64 at any alignment holds exactly one)"""
    units, n = K.small_magnitude_runs(nbytes)
    top = [max(B.magsabs(v) for v in g) for g in units]
    assert all(B.gcf(g) >= 2 for g in units)
    assert max(top[:n]) == (1 << 23) - 1
    big = [k for k in range(n, len(units)) if top[k] >= 1 << 23]
    assert big and all(b - a == 64 for a, b in zip(big, big[1:])) and big[0] - n < 64 and len(units) - big[-1] <= 64
    assert max(top[k] for k in range(n, len(units)) if k not in big) < 1 << 23
    if nbytes == 8:
        assert any(B.gcf(g) > 1 << 32 for g in units)


# ------------------------------------------------------------------------------------------------------------------- GPU

# (type, bands, band map, source pointer offset): the three encoder families
PX_BEST = [(0, 1, None, 0), (0, 3, None, 0), (0, 3, [0, 1, 2], 0), (0, 4, None, 0)]                       # k_enc_px_best.hip
PXW_FRONT = [(2, 1, None, 0), (3, 1, None, 0), (4, 1, None, 0), (5, 1, None, 0), (6, 1, None, 0), (7, 1, None, 0)]     # k_enc_best.hip, one band
ENC_FRONT = [(0, 2, [0, 1], 0), (0, 5, [0, 1, 2, 3, 4], 0), (2, 3, None, 0), (5, 2, [0, 1], 0), (6, 2, [0, 1], 0),
             (4, 1, None, 2)]                                                                               # ... every other raster
GPU_CASES = [c + (m,) for fam in (PX_BEST, PXW_FRONT, ENC_FRONT) for c in fam for m in (CF_H, CF)] + \
            [fam[0] + (BEST,) for fam in (PX_BEST, PXW_FRONT, ENC_FRONT)]

_cases = {}


def gpu_case(oracle, dtype, bands, cband, mode):
    """(raster, SpecCase, the oracle's container): made once, shared, left unchanged"""
    key = (dtype, bands, None if cband is None else tuple(cband), mode)
    if key not in _cases:
        nbytes = T.TYPESIZE[dtype]
        units = K.rotated(K.case_units(nbytes), bands)
        skey = (nbytes, bands)
        if skey not in _cases:
            _cases[skey] = K.SpecCase(units, nbytes)
        img, _ = raster_of(units, dtype, mode, cband)
        _cases[key] = (img, _cases[skey], oracle.encode(img, dtype, mode, cband=cband))
    return _cases[key]


def payload(container):
    c = bytes(container)
    at = c.index(b"DT", 11) if b"ix" not in c[11:15] else T.table_span(c)[1] - 2
    return c[at + 2:]


def same_container(got, ref, sc, what):
    """the oracle's bytes; where they are not, the first unit that is not the spec's, and its cells"""
    got, ref = bytes(got), bytes(ref)
    if got == ref:
        return
    msg = "no unit differs from the spec's"
    if got[10] in (CF, CF_H):       # (the container's own mode byte: not a stream that went through the zero-run pass)
        p = payload(got)
        msg = sc.explain(int.from_bytes(p, "little") & ((1 << sc.bits.n) - 1), sc.bits.n if 8 * len(p) >= sc.bits.n else 8 * len(p)) or msg
    raise AssertionError("%s: %d bytes, the oracle's %d, first differing byte %d; %s" % (
        what, len(got), len(ref), next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref))), msg))


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "t%d-x%d-%s%s-m%d" % (c[0], c[1], "default" if c[2] is None else "identity", "-off%d" % c[3] if c[3] else "", c[4]))
def test_encoders_on_the_decision_rasters(qb3, oracle, case):
    import torch
    from qb3_amd import device as qdev
    dtype, bands, cband, off, mode = case
    img, sc, ref = gpu_case(oracle, dtype, bands, cband, mode)
    h, w, _ = img.shape
    if ref[10] in (CF, CF_H):       # the oracle's own container holds the spec's units
        assert sc.explain(int.from_bytes(payload(ref), "little") & ((1 << sc.bits.n) - 1), sc.bits.n) is None
    same_container(qb3.encode(img, dtype, mode, cband=cband), ref, sc, "qb3_encode")
    raw = torch.from_numpy(img.view(np.uint8).reshape(-1).copy())
    buf = torch.zeros(raw.numel() + 8, dtype=torch.uint8, device="cuda")
    src = buf[off:off + raw.numel()]
    src.copy_(raw)
    enc = qdev.DeviceEncoder(w, h, bands, dtype, mode=mode, cband=cband)
    dst, n, index = enc.encode(src)
    same_container(dst[:n].cpu().numpy(), ref, sc, "the device call")
    dec = qdev.DeviceDecoder(dst, n)
    assert torch.equal(dec.decode(dst, index=index), src), "decode with the out-of-band index"
    assert torch.equal(dec.decode(dst, index=None), src), "decode with index=None"
    # self-indexed containers: decoded from their table, which is the one the table spec builds from the oracle's trace
    for level in (1, 2):
        e2 = qdev.DeviceEncoder(w, h, bands, dtype, mode=mode, cband=cband, want_index=False, index_chunk=level)
        d2, n2, _ = e2.encode(src)
        host = d2[:n2].cpu().numpy().tobytes()
        assert host[10] != 255 and n2 > n, "every decision raster gets a table (level %d)" % level
        dec2 = qdev.DeviceDecoder(d2, n2)
        assert qb3.lib.qb3x_decoder_table_entries(dec2.p) > 0, level
        assert torch.equal(dec2.decode(d2, index=None), src), "decode from the self-indexed container, level %d" % level
        assert qb3.lib.qb3x_last_decode_status(dec2.p) == 0, (level, qb3.lib.qb3x_last_decode_status(dec2.p))
        want_bytes, want = T.build(T.units(oracle, img, dtype, mode, cband), T.entering_values(img, dtype, cband, T.curve_order(mode)), dtype, mode, level)
        T.compare(host, want_bytes, want, dtype, mode)
        at = bytes(ref).index(b"DT", 11)
        assert host == bytes(ref[:at]) + want_bytes + bytes(ref[at + 2:]), "minus its table, the oracle's container (level %d)" % level
