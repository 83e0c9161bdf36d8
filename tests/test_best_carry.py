"""A band's common factor across the chunks the encoders code in parallel, at every alignment (rasters: tests/qb3_best_carry.py).

CPU: the chunks come from plan_encode itself (a mode of tests/dec_route_harness.cpp prints them; no encoder constant is written
here); the census of each case's raster -- a dependent at every offset of a chunk, last writers 0, 1, 2 and more chunks back, every
chunk seam crossed from a writer to a dependent -- is asserted from the spec's units, which are the oracle's.  GPU: three regimes of
the encoders (one pass without a sample, two passes, one pass chosen by the sample), each a process of its own."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_best_carry as C  # noqa: E402
import qb3_table_spec as T  # noqa: E402
import test_decode_routes as R  # noqa: E402

CF_H = 5
FRONTS = ["px_best", "px_best", "pxw_front", "pxw_front", "enc_front", "enc_front", "enc_front"]
ids = lambda c: "t%d-x%d" % c[:2]      # noqa: E731


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(type, bands): (blocks a chunk, chunks, front end, the chunks a sample looks at)} of the cases, from plan_encode"""
    exe = R._build(R._objects(os.path.join(R.CSRC, "build"), True), str(tmp_path_factory.mktemp("plans")))
    args = []
    for dtype, bands, cband, nrows in C.CASES:
        args += [4 * C.PERIOD, 4 * nrows, bands, T.TYPESIZE[dtype], 1 if cband is None and bands == 3 else 0]
    out = subprocess.run([exe, "plan"] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
    print(out)
    got = {}
    for line, (dtype, bands, _, _) in zip(out.splitlines(), C.CASES):
        f = dict(x.split("=") for x in line.split()[6:])
        got[(dtype, bands)] = (int(f["nbp"]), int(f["nchunks"]), f["front"], [int(x) for x in f["sampled"].split(",")])
    return got


needs_hipcc = R.needs_hipcc


def test_the_period_meets_every_offset_of_every_chunk_length():
    """257 is prime: the blocks of the pattern (of band 0) fall on every offset of chunks of 2 .. 256 blocks"""
    a = C.Carry(1, 1, 256)
    blocks = np.array(sorted(k for k, _ in a.units))
    for n in range(2, 257):
        assert len(np.unique(blocks % n)) == n, n


@needs_hipcc
def test_the_plans_are_what_the_rasters_aim_at(plans):
    for (dtype, bands, _, _), front in zip(C.CASES, FRONTS):
        nbp, nchunks, got, _ = plans[(dtype, bands)]
        assert got == front, (dtype, bands, got)
        assert 2 <= nbp < C.PERIOD
        if (dtype, bands) in C.MANY_CHUNKS:
            assert nchunks > C.MANY_CHUNKS[(dtype, bands)], (dtype, bands, nchunks)


_spec = {}


def spec_of(case):
    if case not in _spec:
        dtype, bands, cband, nrows = case
        a = C.Carry(T.TYPESIZE[dtype], bands, nrows)
        _spec[case] = (a,) + a.spec()
    return _spec[case]


@needs_hipcc
@pytest.mark.parametrize("case", C.CASES, ids=ids)
def test_census_of_the_dense_raster(plans, case):
    dtype, bands, cband, nrows = case
    nbp, nchunks, _, sampled = plans[(dtype, bands)]
    a, spec, _ = spec_of(case)
    cens = C.census(spec, bands, nbp)
    for c, cen in enumerate(cens):
        assert cen["offsets"] == set(range(nbp)), "band %d: no dependent at offsets %s" % (c, sorted(set(range(nbp)) - cen["offsets"]))
        assert cen["back"] == {0, 1, 2, 3}, "band %d: last writers %s chunks back" % (c, sorted(cen["back"]))
        assert {"factor-same:C", "factor-new:C", "flip-same:C", "flip-new:I"} <= cen["readers"], (c, cen["readers"])
        # a writer in the first chunk, a dependent in one of the last two (the very last may hold nothing but the raster's last, flat
        # block): wherever the scan across chunks cuts its parts, a seam lies between a writer and its dependent
        assert 0 in cen["writer_chunks"] and max(k for k, cc in spec if cc == c) // nbp >= nchunks - 2
    # which regime QB3_BEST_SAMPLE_MIN=0 runs hangs on the sampled chunks alone, and on those whose last writer moves the band's factor
    # away from the state a fresh encoder starts with: far more than one (chunk, band) pair in eight of the sample here -- twice what makes
    # the encoders go for two passes -- so a pattern that fell in step with the sample's stride could not pass for dense
    assert moved_in_sample(cens, sampled) * 8 > len(sampled) * bands, (moved_in_sample(cens, sampled), len(sampled) * bands)


def moved_in_sample(cens, sampled):
    """(chunk, band) pairs of the sampled chunks whose last writer leaves another factor than a fresh encoder's (2: the state holds 0)"""
    return sum(1 for cen in cens for k in sampled if cen["leaves"].get(k, 0) != 0)


@needs_hipcc
@pytest.mark.parametrize("case", C.CASES, ids=ids)
def test_census_of_the_sparse_raster(plans, case):
    dtype, bands, cband, nrows = case
    nbp, nchunks, _, sampled = plans[(dtype, bands)]
    a = C.Carry(T.TYPESIZE[dtype], bands, nrows, C.SPARSE_KEEP)
    spec, end = a.spec()
    assert end[0][1] != 0, "band 0 leaves a factor that a fresh encoder does not start from: the raster behind it shows the state"
    cens = C.census(spec, bands, nbp)
    for c, cen in enumerate(cens):
        assert 0 < len(cen["writer_chunks"]) * 64 < nchunks, (c, len(cen["writer_chunks"]), nchunks)
        assert cen["back"] - {0}, "band %d: a dependent whose last writer lies in a chunk before its own" % c
    # ... and of the sampled (chunk, band) pairs fewer than one in 32 -- half of what would make the encoders go for two passes
    assert moved_in_sample(cens, sampled) * 32 < len(sampled) * bands, (moved_in_sample(cens, sampled), len(sampled) * bands)


@pytest.mark.parametrize("case", C.CASES, ids=ids)
def test_the_specs_units_are_the_oracles(oracle, case):
    """every unit of the dense raster that is not flat, against the oracle's trace and stream: start, kind, rung, factor, the factor
    before it, its bits; every other unit is a rung-0 unit.  Then a second raster on the same encoder, whose first unit has the factor
    the first raster ends on: "the same" through the state alone"""
    dtype, bands, cband, nrows = case
    nbytes = T.TYPESIZE[dtype]
    a, spec, end = spec_of(case)
    h, w, _ = a.shape
    e = oracle.Encoder(w, h, bands, dtype)
    e.set_mode(CF_H)
    if cband is not None:
        e.set_coreband(list(cband))
    b = C.Carry(nbytes, bands, nrows, turn=3, lead=end[0][1] + 2)
    spec_b, end_b = b.spec(end)
    first = min(k for k, c in spec_b if c == 0)
    assert spec_b[(first, 0)][0].info["same"] and b.spec()[0][(first, 0)][0].info["same"] is False
    for car, sp, st_end in ((a, spec, end), (b, spec_b, end_b)):
        stream, nbits, rows, state = T._raw_trace(oracle, car.raster(dtype, cband), dtype, CF_H, cband, encoder=e)
        assert len(rows) == nrows * C.PERIOD * bands
        kinds = rows[:, 1].astype(np.int64)
        buf = stream.to_bytes((nbits + 7) // 8 + 160, "little")           # (slices of bytes: a shift of the whole stream a unit is slow)
        flat = np.ones(len(rows), bool)
        starts = np.append(rows[:, 0], np.uint64(nbits)).astype(np.int64)
        for (k, c), (u, rung, pcf) in sp.items():
            i = k * bands + c
            flat[i] = False
            got = (str(T.KINDS[kinds[i]]), int(rows[i, 2]), int(rows[i, 3]), int(rows[i, 4]), int(starts[i + 1] - starts[i]))
            assert got == (u.kind, u.rung, u.cf, pcf, u.bits.n), "block %d, band %d: the oracle's (kind, rung, factor, factor before, bits) %r, the spec's %r" % (
                k, c, got, (u.kind, u.rung, u.cf, pcf, u.bits.n))
            at = int(starts[i])
            have = int.from_bytes(buf[at >> 3:(at >> 3) + 160], "little") >> (at & 7)
            assert have & ((1 << u.bits.n) - 1) == u.bits.v, "block %d, band %d: the unit's bits" % (k, c)
        assert (kinds[flat] == 0).all() and (rows[flat, 2] == 0).all(), "every other unit is flat"
        assert [(int(r), int(f)) for _, r, f in state] == st_end, "the band state behind the raster"


def run_regime(regime, env_value):
    env = {k: v for k, v in os.environ.items() if k != "QB3_BEST_SAMPLE_MIN"}
    if env_value is not None:
        env["QB3_BEST_SAMPLE_MIN"] = env_value
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "best_carry_run.py"), regime],
                       env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (regime, env_value, r.stdout[-2000:] + r.stderr[-4000:])


@pytest.mark.gpu
def test_one_pass_without_a_sample(qb3):
    """the default: a raster of fewer chunks than the sampling starts at is coded once, assuming the starting state, and every chunk
    that looked at a wrong entering factor is listed and coded again"""
    run_regime("dense", None)


@pytest.mark.gpu
def test_two_passes_chosen_by_the_sample(qb3):
    """QB3_BEST_SAMPLE_MIN=0 on the dense raster: the sample finds writers everywhere, the first pass collects the chunk summaries,
    the last codes every chunk with its true entering factor"""
    run_regime("dense", "0")


@pytest.mark.gpu
def test_one_pass_chosen_by_the_sample(qb3):
    """QB3_BEST_SAMPLE_MIN=0 on the sparse raster (a writer in fewer than one chunk of 64): the sample chooses one pass, the list
    holds the few chunks behind the pattern rows"""
    run_regime("sparse", "0")
