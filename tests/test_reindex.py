"""Reindex on the GPU (qb3x_reindex_device, qb3x_reindex; include/qb3x.h).  The oracle of the feature: let C0, C1, C2 be the containers
this library's encoder writes for one raster with qb3x_set_encoder_index_chunk 0, 1 and 2; then reindex(Ca, level b) == Cb byte for
byte, for all nine pairs -- the table reindex makes from the walk's index is the table the encoder makes from its own, and nothing
else of the container moves."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qb3_window as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTL, BASE, CF_H, BASE_Z, BEST = 8, 4, 5, 0, 7
QB3E_ERR = 3
TYPESIZE = (1, 1, 2, 2, 4, 4, 8, 8)


def gen_for(dt, mode):
    """a generator whose raster codes (never STORED) in the mode and, in a common-factor mode, has factors to find"""
    cf = mode in (CF_H, BEST)
    if dt == 0:
        return "FEW" if cf else "NOISY3"
    if dt == 2:
        return "TERRACE" if cf else "LANDSAT16"
    return "TERRACE" if cf else "DEM"


def own(t, n):
    """the first n bytes of a device tensor in a buffer of their own (fresh: aligned; zeros behind the end)"""
    import torch
    out = torch.zeros((n + 3) // 4 * 4 + 16, dtype=torch.uint8, device=t.device)
    out[:n] = t[:n]
    return out


def encode_levels(img, w, h, b, dt, mode):
    """[(device buffer, size, host bytes)] for qb3x_set_encoder_index_chunk 0, 1, 2"""
    import torch
    from qb3_amd import device as qdev
    raw = img.reshape(-1).view(torch.uint8)
    out = []
    for level in (0, 1, 2):
        enc = qdev.DeviceEncoder(w, h, b, dt, mode=mode, want_index=False, index_chunk=level)
        dst, n, _ = enc.encode(raw)
        d = own(dst, n)
        out.append((d, n, d[:n].cpu().numpy()))
        enc.close()
    return out


def reindex_dev(qb3, host, d_src, level, cap=None, guard=256):
    """qb3x_reindex_device through a handle over the host copy; returns (n, device bytes [:n], guard intact, status, handle error)"""
    import torch
    L = qb3.lib
    host = np.ascontiguousarray(host, np.uint8)
    p, _ = W.open_handle(L, host)
    try:
        if cap is None:
            cap = L.qb3x_reindex_size(p, level)
            assert cap
        room = (cap + 3) // 4 * 4
        out = torch.full((room + guard,), 0x5C, dtype=torch.uint8, device=d_src.device)
        n = L.qb3x_reindex_device(p, d_src.data_ptr(), out.data_ptr(), cap, level, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return n, out[:n], bool((out[cap:] == 0x5C).all()), L.qb3x_last_decode_status(p), W.handle_error(p)
    finally:
        L.qb3_destroy_decoder(p)


def check_matrix(qb3, img, w, h, b, dt, mode, want_mode=None):
    import torch
    cs = encode_levels(img, w, h, b, dt, mode)
    assert cs[0][2][10] == (mode if want_mode is None else want_mode), "the raster did not code in the mode the case is about"
    assert cs[0][1] < cs[1][1] <= cs[2][1], "the encoder wrote no table: the case shows nothing"
    for a in range(3):
        for lv in range(3):
            n, got, ok, status, err = reindex_dev(qb3, cs[a][2], cs[a][0], lv)
            tag = "reindex(C%d, %d) of %dx%dx%d type %d mode %d" % (a, lv, w, h, b, dt, mode)
            assert n == cs[lv][1], (tag, n, cs[lv][1], status, err, qb3.last_error())
            if not torch.equal(got, cs[lv][0][:n]):
                g, want = got.cpu().numpy(), cs[lv][2]
                at = int(np.flatnonzero(g != want)[0])
                raise AssertionError("%s differs from C%d at byte %d of %d (%d bytes differ; the coded bytes start at %d)" %
                                     (tag, lv, at, n, int((g != want).sum()), bytes(want).index(b"DT", 11) + 2 if lv == 0 else n - (cs[0][1] - bytes(cs[0][2]).index(b"DT", 11) - 2)))
            assert ok and err == W.QB3E_OK and (status & ~64) == 0, tag
    return cs


SHAPES = [(0, b) for b in (1, 2, 3, 4, 5)] + [(2, b) for b in (1, 2, 3, 4, 7, 8)] + [(4, 1), (4, 2), (6, 1), (6, 2)]


@pytest.mark.parametrize("mode", [FTL, BASE, CF_H, BASE_Z], ids=lambda m: "m%d" % m)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "t%dx%d" % s)
def test_equality_matrix(qb3, shape, mode):
    """u8 x {1..5}, u16 x {1, 2, 3, 4, 7, 8}, u32 and u64 x {1, 2} bands in FTL, BASE, CF_H and BASE_Z: all nine pairs"""
    from qb3_amd import synth
    dt, b = shape
    w, h = 388, 132
    check_matrix(qb3, synth.generate(w, h, b, dt, gen_for(dt, mode), 11), w, h, b, dt, mode)


@pytest.mark.parametrize("case", [(517, 263, 3, 0, FTL), (517, 263, 4, 2, BASE), (517, 263, 1, 4, FTL), (517, 263, 3, 0, CF_H), (517, 263, 5, 2, CF_H)],
                         ids=lambda c: "%dx%dx%d-t%d-m%d" % c)
def test_equality_matrix_odd_sizes(qb3, case):
    """a shifted last block row and column"""
    from qb3_amd import synth
    w, h, b, dt, mode = case
    check_matrix(qb3, synth.generate(w, h, b, dt, gen_for(dt, mode), 12), w, h, b, dt, mode)


@pytest.mark.parametrize("case", [(2048, 2048, 3, 0, FTL), (2052, 2048, 4, 2, BASE), (2048, 2050, 1, 4, FTL), (2048, 2048, 1, 6, BASE), (2048, 2048, 3, 0, CF_H)],
                         ids=lambda c: "%dx%dx%d-t%d-m%d" % c)
def test_equality_matrix_large(qb3, case):
    """at least 2048^2 per value width: several table chunks, many segments, a payload of megabytes moved by a distance that is
    not a multiple of sixteen bytes"""
    from qb3_amd import synth
    w, h, b, dt, mode = case
    cs = check_matrix(qb3, synth.generate(w, h, b, dt, gen_for(dt, mode), 13), w, h, b, dt, mode)
    assert cs[2][1] - cs[0][1] > 65535, "one table chunk only"


def test_rle0_pass_wins_and_loses(qb3):
    """QB3M_BEST on a raster whose RLE0 pass wins (a flat raster with a patch of noise, uint32, three bands: the container keeps its
    RLE0 bytes and gets the table of the EXPANDED block stream in front of DT, as from the encoder) and on one where it loses (the
    container is the common-factor mode's)"""
    import torch
    from qb3_amd import synth
    w, h, b = 512, 256, 3
    g = torch.Generator().manual_seed(7)
    img = torch.full((h, w, b), 1000, dtype=torch.int32)
    img[64:160, 128:320, :] = torch.randint(0, 2 ** 31 - 1, (96, 192, b), generator=g, dtype=torch.int64).to(torch.int32)
    check_matrix(qb3, img.cuda(), w, h, b, 4, BEST, want_mode=BEST)
    check_matrix(qb3, synth.generate(256, 128, 3, 0, "NOISY3", 3), 256, 128, 3, 0, BEST, want_mode=CF_H)


@pytest.mark.parametrize("case", [(1024, 517, 3, 0, "NOISY3", FTL), (515, 300, 8, 2, "LANDSAT16", BASE), (300, 200, 1, 5, "TERRACE", CF_H)],
                         ids=lambda c: "%dx%dx%d-t%d-%s-m%d" % c)
def test_reference_made_input(qb3, oracle, case):
    """the reference's bytes (the oracle's encoder) reindexed at level 2: a table of one entry per segment that the decoder uses (bit 5
    clear) for the oracle's pixels, a container the reference's chunk loop still decodes, windows by the window kernel (8-bit RGB), and
    back to the original bytes at level 0"""
    import torch
    from qb3_amd import device as qdev
    w, h, b, dt, gen, mode = case
    himg = oracle.generate(w, h, b, dt, gen, 21)
    ref = oracle.encode(himg, dt, mode)
    assert ref[10] == mode
    d_ref = own(torch.from_numpy(ref).cuda(), len(ref))
    n, got, ok, status, err = reindex_dev(qb3, ref, d_ref, 2)
    assert n > len(ref) and ok and err == W.QB3E_OK, (n, status, err, qb3.last_error())
    d_c2 = own(got, n)
    c2 = d_c2[:n].cpu().numpy()
    p, _ = W.open_handle(qb3.lib, c2)
    bps = C.c_size_t()
    segs = qb3.lib.qb3x_window_segments(p, 0, 0, w, h, C.byref(bps))
    entries = qb3.lib.qb3x_decoder_table_entries(p)
    qb3.lib.qb3_destroy_decoder(p)
    nblocks = ((w + 3) // 4) * ((h + 3) // 4)
    assert bps.value and segs == (nblocks + bps.value - 1) // bps.value
    if mode != CF_H:
        assert entries == segs                          # FTL / BASE: an entry per index segment
    else:
        assert 0 < entries <= segs
    want = torch.from_numpy(himg.view(np.uint8).reshape(-1).copy()).cuda()
    dec = qdev.DeviceDecoder(d_c2, n)
    assert torch.equal(dec.decode(d_c2, index=None), want)
    assert qb3.lib.qb3x_last_decode_status(dec.p) & 32 == 0, "the decoder did not use the table reindex wrote"
    assert qb3.lib.qb3x_last_decode_status(dec.p) == 0
    o_out, _, _, _ = oracle.decode(c2, identity=True)
    assert o_out is not None and np.array_equal(o_out, himg.view(np.uint8).reshape(-1)), "the reference's chunk loop does not decode the reindexed container"
    if dt == 0 and b == 3:
        x0, y0, ww, hh = 301, 77, 200, 100
        win = dec.decode_window(d_c2, x0, y0, ww, hh)
        assert dec.last_window[0] == 1, dec.last_window
        assert np.array_equal(win.cpu().numpy(), himg[y0:y0 + hh, x0:x0 + ww])
    n0, got0, ok0, _, err0 = reindex_dev(qb3, c2, d_c2, 0)
    assert n0 == len(ref) and np.array_equal(got0.cpu().numpy(), ref) and ok0 and err0 == W.QB3E_OK


def test_upgrade_of_a_table_the_decoder_ignores_or_cannot_trust(qb3):
    """a C1 whose table says another `blocks per entry` (a container of an earlier segment size: ignored by the decoder today) and a C2
    with a damaged entry byte both become C2: the source's table is never read"""
    import torch
    from qb3_amd import synth
    w, h, b, dt = 640, 388, 3, 0
    cs = encode_levels(synth.generate(w, h, b, dt, "NOISY3", 31), w, h, b, dt, FTL)
    c1 = cs[1][2].copy()
    at = bytes(c1).index(b"ix", 11)
    blocks = int.from_bytes(bytes(c1[at + 8:at + 12]), "little")
    c1[at + 8:at + 12] = np.frombuffer((blocks * 2).to_bytes(4, "little"), np.uint8)
    p, _ = W.open_handle(qb3.lib, c1)
    qb3.lib.qb3_destroy_decoder(p)
    c2bad = cs[2][2].copy()
    at2 = bytes(c2bad).index(b"ix", 11)
    c2bad[at2 + 12 + 200] ^= 0x40
    for src in (c1, c2bad):
        d_src = own(torch.from_numpy(src).cuda(), len(src))
        n, got, ok, status, err = reindex_dev(qb3, src, d_src, 2)
        assert n == cs[2][1] and torch.equal(got, cs[2][0][:n]) and ok and err == W.QB3E_OK, (n, status, err)


def test_refusals(qb3):
    """a corrupt stream and a truncated one return 0 with QB3E_ERR; a destination one byte short returns 0 with QB3E_EINV; nothing is
    written at or behind d_dst + dst_cap in any of them"""
    import torch
    from qb3_amd import synth, device as qdev
    w, h, b, dt = 640, 388, 3, 0
    cs = encode_levels(synth.generate(w, h, b, dt, "NOISY3", 41), w, h, b, dt, BASE)
    c0 = cs[0][2]
    first = bytes(c0).index(b"DT", 11) + 2
    # a flipped bit that makes the decode fail: the first of a few candidates the plain decode refuses
    bad = None
    for bit in range(16):
        cand = c0.copy()
        cand[first + 40 + bit // 8] ^= 1 << (bit % 8)
        d_c = own(torch.from_numpy(cand).cuda(), len(cand))
        dec = qdev.DeviceDecoder(cand, len(cand))
        try:
            dec.decode(d_c, index=None)
        except RuntimeError:
            bad = (cand, d_c)
            break
        finally:
            dec.close()
    assert bad is not None, "none of the flips made the decode fail"
    n, _, ok, status, err = reindex_dev(qb3, bad[0], bad[1], 2)
    assert n == 0 and err == QB3E_ERR and ok and status != 0, (n, err, status)
    # cut short by 100 bytes
    cut = c0[:-100].copy()
    d_cut = own(torch.from_numpy(cut).cuda(), len(cut))
    n, _, ok, status, err = reindex_dev(qb3, cut, d_cut, 2)
    assert n == 0 and err == QB3E_ERR and ok and status != 0, (n, err, status)
    n, _, ok, status, err = reindex_dev(qb3, cut, d_cut, 1)
    assert n == 0 and err == QB3E_ERR and ok
    # one byte below the bound: nothing is touched at all
    p, _ = W.open_handle(qb3.lib, c0)
    need = qb3.lib.qb3x_reindex_size(p, 2)
    qb3.lib.qb3_destroy_decoder(p)
    assert need == cs[2][1]
    n, _, ok, _, err = reindex_dev(qb3, c0, cs[0][0], 2, cap=need - 1)
    assert n == 0 and err == W.QB3E_EINV and ok
    n, got, ok, _, err = reindex_dev(qb3, c0, cs[0][0], 2, cap=need)
    assert n == need and torch.equal(got, cs[2][0][:n]) and ok and err == W.QB3E_OK


def test_host_call_python_binding_and_profile_names(qb3):
    """qb3_amd.reindex (qb3x_reindex: host buffers) and DeviceDecoder.reindex give the device call's bytes; the two kernels report
    under their profile names"""
    import torch
    from qb3_amd import synth, device as qdev
    w, h, b, dt = 1030, 515, 3, 0
    cs = encode_levels(synth.generate(w, h, b, dt, "NOISY3", 51), w, h, b, dt, FTL)
    for a, lv in ((0, 2), (0, 1), (2, 0), (1, 2), (2, 2)):
        got = qb3.reindex(cs[a][2], lv)
        assert len(got) == cs[lv][1] and np.array_equal(got, cs[lv][2]), (a, lv)
    dec = qdev.DeviceDecoder(cs[0][2], cs[0][1])
    qdev.profile_enable(1)
    qdev.profile_reset()
    out, n = dec.reindex(cs[0][0], 2)
    rep = qdev.profile_report()
    qdev.profile_enable(0)
    assert n == cs[2][1] and torch.equal(out[:n], cs[2][0][:n])
    assert rep.get("reindex_fill", (0, 0))[1] == 1 and rep.get("reindex_finish", (0, 0))[1] == 1, rep
    head_only = qdev.DeviceDecoder(cs[0][0], cs[0][1])         # made from the device copy: holds the container's head only
    with pytest.raises(ValueError):
        head_only.reindex(cs[0][0], 2)


def test_qb3index_then_cqb3x_round_trips_a_pnm(qb3, tmp_path):
    """cqb3x in.ppm -> plain container; qb3index -2 -> self-indexed; cqb3x -d -> the same PNM"""
    from qb3_amd import synth
    w, h = 515, 259
    img = synth.generate(w, h, 3, 0, "NOISY3", 61).cpu().numpy()
    ppm = tmp_path / "in.ppm"
    ppm.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    tools = os.path.join(ROOT, "qb3_amd")

    def run(*cmd):
        r = subprocess.run(list(cmd), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (cmd, r.stdout, r.stderr)
        return r.stdout

    plain, indexed, back, stripped = (str(tmp_path / n) for n in ("plain.qb3", "indexed.qb3", "back.ppm", "stripped.qb3"))
    run(os.path.join(tools, "cqb3x"), str(ppm), plain)
    said = run(os.path.join(tools, "qb3index"), "-2", "-v", plain, indexed)
    assert "table entries" in said and " ms" in said
    run(os.path.join(tools, "cqb3x"), "-d", indexed, back)
    assert open(back, "rb").read() == ppm.read_bytes()
    c0, c2 = np.fromfile(plain, np.uint8), np.fromfile(indexed, np.uint8)
    assert len(c2) > len(c0)
    p, _ = W.open_handle(qb3.lib, c2)
    assert qb3.lib.qb3x_decoder_table_entries(p) == (((w + 3) // 4) * ((h + 3) // 4) + 63) // 64
    qb3.lib.qb3_destroy_decoder(p)
    run(os.path.join(tools, "qb3index"), "-0", indexed, stripped)
    assert open(stripped, "rb").read() == open(plain, "rb").read()
