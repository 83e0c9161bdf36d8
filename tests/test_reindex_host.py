"""Reindex (qb3x_reindex_size, qb3x_reindex_device, qb3x_reindex; include/qb3x.h), the part that needs no device: the symbols, the
chunk surgery of level 0, the containers for which the encoder writes no table, the size bound, the refusals.  The containers are
the oracle's (the CPU restatement tests/test_oracle_anchors.py uses); a table is spliced into them as bytes -- a run of "ix" + "zz"
chunks that parses, with entries that mean nothing: what is dropped is never read."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import qb3_window as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTL, BASE, CF_H, BEST, RLE_H, STORED = 8, 4, 5, 7, 6, 255
QB3E_ERR = 3
IX_HEAD, IX_PAD = 12, 4


def dt_offset(c):
    """offset of "DT" in a container (an ignorable, lower-case chunk's length counts from the chunk's start)"""
    pos, c = 11, bytes(c)
    while c[pos:pos + 2] != b"DT":
        assert c[pos:pos + 2] in (b"CB", b"QV", b"SC") or c[pos] & 0x20, c[pos:pos + 2]
        pos += (c[pos + 2] | c[pos + 3] << 8) + (0 if c[pos] & 0x20 else 4)
    return pos


def splice_table(c, entry_bytes, entries, per_chunk, flags, version=3, blocks=64, filler=0xA5):
    """the container with a run of "ix" chunks (a "zz" pad behind each from version 2 on) in front of "DT": heads that parse,
    entries of filler bytes"""
    c = np.asarray(c, np.uint8)
    at = dt_offset(c)
    run = b""
    for k0 in range(0, entries, per_chunk):
        here = min(per_chunk, entries - k0)
        ln = IX_HEAD + here * entry_bytes
        run += b"ix" + bytes([ln & 255, ln >> 8, version, flags, 0, 0]) + blocks.to_bytes(4, "little") + bytes([filler]) * (here * entry_bytes)
        if version >= 2:
            run += b"zz\x04\x00"
    return np.concatenate([c[:at], np.frombuffer(run, np.uint8), c[at:]])


def reindex_host(qb3, c, level, cap=None, guard=64):
    """qb3x_reindex into a buffer of cap bytes (default: the bound) with a guard region behind it; returns (n, bytes, guard intact)"""
    c = np.ascontiguousarray(c, np.uint8)
    if cap is None:
        p, _ = W.open_handle(qb3.lib, c)
        cap = qb3.lib.qb3x_reindex_size(p, level)
        qb3.lib.qb3_destroy_decoder(p)
        assert cap
    out = np.full(cap + guard, 0x5C, np.uint8)
    n = qb3.lib.qb3x_reindex(c.ctypes.data, c.size, out.ctypes.data, cap, level)
    return n, out[:n].copy(), bool((out[cap:] == 0x5C).all())


def test_symbols_are_declared_exported_and_harmless_with_null(qb3):
    text = open(os.path.join(ROOT, "include", "qb3x.h")).read()
    for name in ("qb3x_reindex_size", "qb3x_reindex_device", "qb3x_reindex"):
        assert re.search(r"\bsize_t\s+%s\s*\(" % name, text), name
        assert hasattr(qb3.lib, name) and name in qb3.EXPORTED
    L = qb3.lib
    buf = np.zeros(64, np.uint8)
    assert L.qb3x_reindex_size(None, 1) == 0
    assert L.qb3x_reindex_device(None, None, None, 0, 1, None) == 0
    assert L.qb3x_reindex_device(None, buf.ctypes.data, buf.ctypes.data, 64, 1, None) == 0
    assert L.qb3x_reindex(None, 0, None, 0, 0) == 0
    assert L.qb3x_reindex(None, 64, buf.ctypes.data, 64, 0) == 0
    assert L.qb3x_reindex(buf.ctypes.data, 64, None, 64, 0) == 0
    assert L.qb3x_reindex(buf.ctypes.data, 64, buf.ctypes.data, 64, 0) == 0          # (zeros are not a container)
    for name in ("reindex_fill", "reindex_finish"):
        assert name in text, "profile name %s is not listed in the qb3x_profile_enable comment" % name


CASES = [(64, 48, 3, 0, "NOISY3", FTL), (67, 45, 1, 0, "NOISY3", BASE), (40, 40, 4, 2, "LANDSAT16", CF_H), (33, 21, 2, 5, "DEM", BEST),
         (64, 64, 3, 0, "NOISY3", 0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-t%d-%s-m%d" % c)
def test_level_0_strips_the_table_on_the_host(qb3, oracle, case):
    """C1- and C2-like fixtures (and a version 1 table, one chunk without a pad; and several chunks): level 0 gives the oracle's bytes
    back exactly; a plain container comes back as it is"""
    w, h, b, dt, gen, mode = case
    ref = oracle.encode(oracle.generate(w, h, b, dt, gen, 5), dt, mode)
    n, got, ok = reindex_host(qb3, ref, 0)
    assert n == len(ref) and np.array_equal(got, ref) and ok
    for entry_bytes, entries, per_chunk, flags, version in ((6 + 2 * b, 40, 4096, 0, 3), (6 + 2 * b + 80, 40, 4096, 2, 3), (6 + 2 * b, 40, 4096, 0, 1),
                                                             (6 + 2 * b + 80, 1500, 600, 2, 3), (6 + 2 * b, 33, 4096, 1, 2)):
        c = splice_table(ref, entry_bytes, entries, per_chunk, flags, version)
        assert len(c) > len(ref)
        p, _ = W.open_handle(qb3.lib, c)
        assert qb3.lib.qb3x_reindex_size(p, 0) == len(ref)
        qb3.lib.qb3_destroy_decoder(p)
        n, got, ok = reindex_host(qb3, c, 0)
        assert n == len(ref) and np.array_equal(got, ref) and ok, (entry_bytes, entries, per_chunk, flags, version)


def test_level_0_keeps_foreign_chunks(qb3, oracle):
    """an ignorable chunk that is not the table's stays where it is, between the chunks that are dropped"""
    ref = oracle.encode(oracle.generate(64, 48, 3, 0, "NOISY3", 5), 0, FTL)
    at = dt_offset(ref)
    foreign = np.frombuffer(b"ab\x09\x00hello", np.uint8)
    want = np.concatenate([ref[:at], foreign, ref[at:]])
    c = splice_table(want, 12, 7, 4096, 0)          # (spliced in front of DT: behind the foreign chunk)
    c = np.concatenate([c[:at], np.frombuffer(b"zz\x04\x00", np.uint8), c[at:]])       # ... and a stray pad in front of it
    n, got, ok = reindex_host(qb3, c, 0)
    assert n == len(want) and np.array_equal(got, want) and ok


def test_stored_and_narrow_containers_come_back_without_a_device(qb3, oracle):
    """where the encoder writes no table the output is the source without its ix / zz chunks, at every level"""
    stored = oracle.encode(oracle.generate(64, 32, 3, 0, "RANDOM", 9), 0, FTL)          # noise does not compress: the raw fallback
    assert stored[10] == STORED
    tiny = oracle.encode(oracle.generate(4, 4, 3, 0, "NOISY3", 9), 0, FTL)              # one block: stored
    assert tiny[10] == STORED
    narrow = oracle.encode(oracle.generate(3, 200, 1, 0, "GRAD", 9), 0, BASE)
    narrow2 = oracle.encode(oracle.generate(300, 2, 3, 2, "LANDSAT16", 9), 2, FTL)
    assert narrow[10] != STORED and narrow2[10] != STORED
    for ref in (stored, tiny, narrow, narrow2):
        for level in (0, 1, 2):
            n, got, ok = reindex_host(qb3, ref, level)
            assert n == len(ref) and np.array_equal(got, ref) and ok
    for ref in (narrow, narrow2):                   # (a STORED container's parser does not take a table: it has none to lose)
        c = splice_table(ref, 9, 5, 4096, 0)
        for level in (0, 1, 2):
            n, got, ok = reindex_host(qb3, c, level)
            assert n == len(ref) and np.array_equal(got, ref) and ok


SIZE_CASES = [(512, 512, 3, 0), (509, 259, 1, 0), (640, 384, 4, 0), (256, 256, 5, 0), (256, 256, 3, 2), (256, 128, 5, 2), (300, 200, 4, 3),
              (700, 300, 1, 2), (320, 240, 6, 3), (256, 256, 1, 7), (128, 128, 2, 4), (131, 67, 8, 2)]


@pytest.mark.parametrize("case", SIZE_CASES, ids=lambda c: "%dx%dx%d-t%d" % c)
def test_size_bound_is_the_source_minus_its_table_plus_the_new_one(qb3, oracle, case):
    """qb3x_reindex_size needs no device.  Level 0: the source without its ix / zz bytes.  Levels 1, 2: that plus the table of the
    container's mode -- and qb3_max_encoded_size grows, with qb3x_set_encoder_index_chunk, by the larger of the FTL/BASE table and the
    common-factor one (tests/test_abi.py, test_room_for_the_restart_table): the same figure from the other side of the library"""
    w, h, b, dt = case
    L = qb3.lib
    e = L.qb3_create_encoder(w, h, b, dt)
    base = L.qb3_max_encoded_size(e)
    grow = {}
    for level in (1, 2):
        L.qb3x_set_encoder_index_chunk(e, level)
        grow[level] = L.qb3_max_encoded_size(e) - base
    L.qb3_destroy_encoder(e)
    gen = "LANDSAT16" if dt in (2, 3) else "NOISY3"
    img = oracle.generate(w, h, b, dt, gen, 3)
    delta = {1: [], 2: []}
    for mode in (FTL, BASE, CF_H):
        ref = oracle.encode(img, dt, mode)
        assert ref[10] == mode
        withtab = splice_table(ref, 6 + 2 * b, 11, 4096, 0)
        for c in (ref, withtab):
            p, _ = W.open_handle(L, c)
            assert L.qb3x_reindex_size(p, 0) == len(ref)
            sizes = {lv: L.qb3x_reindex_size(p, lv) for lv in (1, 2)}
            assert L.qb3x_reindex_size(p, 3) == 0 and L.qb3x_reindex_size(p, -1) == 0
            assert W.handle_error(p) == W.QB3E_OK                       # a question, not a call that can fail the handle
            L.qb3_destroy_decoder(p)
            assert len(ref) < sizes[1] <= sizes[2]
            for lv in (1, 2):
                assert 0 < sizes[lv] - len(ref) <= grow[lv]
        for lv in (1, 2):
            delta[lv].append(sizes[lv] - len(ref))
    assert delta[1][0] == delta[1][1] and delta[2][0] == delta[2][1]    # FTL and BASE streams share a layout
    for lv in (1, 2):
        assert max(delta[lv]) == grow[lv], (delta, grow)


def test_refusals_that_need_no_device(qb3, oracle):
    L = qb3.lib
    ref = oracle.encode(oracle.generate(64, 48, 3, 0, "NOISY3", 5), 0, FTL)
    dims = (C.c_size_t * 3)()
    dst = np.full(len(ref) + 4096, 0x5C, np.uint8)
    # a handle that is not past qb3_read_info
    p = L.qb3_read_start(ref.ctypes.data, ref.size, dims)
    assert p and L.qb3x_reindex_size(p, 1) == 0
    assert L.qb3x_reindex_device(p, ref.ctypes.data, dst.ctypes.data, dst.size, 1, None) == 0 and W.handle_error(p) == W.QB3E_EINV
    L.qb3_destroy_decoder(p)
    # one that holds only the container's head
    head = ref[:64].copy()
    p = L.qb3x_read_start(head.ctypes.data, head.size, ref.size, dims)
    assert p and L.qb3_read_info(p)
    assert L.qb3x_reindex_size(p, 1) == 0
    assert L.qb3x_reindex_device(p, ref.ctypes.data, dst.ctypes.data, dst.size, 1, None) == 0 and W.handle_error(p) == W.QB3E_EINV
    L.qb3_destroy_decoder(p)
    # a level outside 0..2, a short destination, misaligned pointers, NULL: each on a fresh handle (an error stays on a handle)
    need = len(ref)
    for args in ((ref.ctypes.data, dst.ctypes.data, dst.size, 3), (ref.ctypes.data, dst.ctypes.data, dst.size, -1),
                 (ref.ctypes.data, dst.ctypes.data, need - 1, 0), (ref.ctypes.data + 1, dst.ctypes.data, dst.size, 0),
                 (ref.ctypes.data, dst.ctypes.data + 2, dst.size - 2, 0), (None, dst.ctypes.data, dst.size, 0), (ref.ctypes.data, None, dst.size, 0)):
        p, _ = W.open_handle(L, ref)
        assert L.qb3x_reindex_device(p, *args, None) == 0 and W.handle_error(p) == W.QB3E_EINV, args
        L.qb3_destroy_decoder(p)
    assert (dst == 0x5C).all()
    # the host call: the same refusals, nothing written
    for level, cap in ((3, dst.size), (-1, dst.size), (0, need - 1), (1, need), (2, need)):
        assert L.qb3x_reindex(ref.ctypes.data, ref.size, dst.ctypes.data, cap, level) == 0, (level, cap)
    assert L.qb3x_reindex(ref.ctypes.data, 10, dst.ctypes.data, dst.size, 0) == 0
    assert (dst == 0x5C).all()
    n, got, ok = reindex_host(qb3, ref, 0, cap=need)
    assert n == need and ok
