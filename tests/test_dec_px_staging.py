"""The staging of dec_px_kernel (k_dec_px.hip): a segment's stream words go to LDS sixteen bytes a lane where all its four-word groups
lie in front of the stream's last word, and a dword a lane (the clamped loop) at the stream's end, on a truncated stream and for a
segment that does not fit.  Which path a segment takes is worked out HERE from the table's positions, by the kernel's rule, and every
raster is shown to take both; the decoded raster is compared byte for byte, from the table and with the out-of-band index, and the
status is 0 on every valid container.

uint8, level-2 containers.  The container is placed at byte offsets 0, 4, 8 and 12 of a 16-byte aligned device buffer (the source is
dword aligned, no more), and once at the very end of an allocation of exactly its size rounded up to 4."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_table_spec as T  # noqa: E402

pytestmark = pytest.mark.gpu

U8, FTL, BASE = 0, 8, 4
# w, h, bands, kind, mode: 16 segments; a last segment of fewer than 64 blocks (17 x 65 = 1105 blocks); one and four bands
RASTERS = [(256, 64, 3, "random", FTL), (260, 68, 3, "random", BASE), (256, 64, 1, "random", FTL), (256, 64, 4, "random", FTL),
           (256, 64, 3, "const", FTL), (260, 68, 3, "const", BASE), (260, 68, 4, "noisy", BASE)]
ids = lambda r: "%dx%dx%d-%s-m%d" % r      # noqa: E731


def raster(r):
    """host array (h, w, bands): random values of five bits (long segments -- random bytes would not compress and the container
    would be a stored one), one value (two bits a unit: segments of a few words), or the generator's noisy raster (between the two)"""
    w, h, b, kind, _ = r
    if kind == "const":
        return np.full((h, w, b), 77, dtype=np.uint8)
    if kind == "noisy":
        from oracle import pyoracle
        return pyoracle.generate(w, h, b, U8, "NOISY3", 9)
    return np.random.default_rng(w * 131 + h * 7 + b).integers(0, 32, (h, w, b), dtype=np.uint8)


_coded = {}


def coded(r):
    """(raster, container bytes, index as a host array) of one encode with table and index: made once, shared, left unchanged"""
    import torch
    from qb3_amd import device as qdev
    if r not in _coded:
        w, h, b, _, mode = r
        img = raster(r)
        enc = qdev.DeviceEncoder(w, h, b, U8, mode=mode, want_index=True, index_chunk=2)
        d, n, index = enc.encode(torch.from_numpy(img.reshape(-1)).cuda())
        torch.cuda.synchronize()
        _coded[r] = (img, d[:n].cpu().numpy().tobytes(), index.cpu().numpy().copy())
        enc.close()
    return _coded[r]


def staging(container, nbytes=None):
    """[(sixteen bytes a lane?, ndw)] a segment, by the kernel's rule from the table's positions: the stream starts behind "DT", in32 is
    the dword at or before it; a segment's words are w0 .. w0 + ndw, the stream's last word is endw - 1"""
    c = bytes(container)
    t, _, t1 = T.parse(c)
    n = len(c) if nbytes is None else nbytes
    bit0, in_bits = 8 * (t1 & 3), 8 * (n - t1)
    endw = (bit0 + in_bits + 31) >> 5
    bands = t.lay["bands"]
    cap = (64 * bands * 149 + 31) // 32 + 2         # the staging of a wave: the longest valid segment (149 bits a unit) + 2
    pos = [int(p) for p in t.pos] + [in_bits]
    out = []
    for k in range(len(t.pos)):
        w0 = (bit0 + pos[k]) >> 5
        ndw = ((bit0 + pos[k + 1] + 31) >> 5) - w0
        pad = -(1024 + (k & 3) * (cap + 8)) & 3       # (where the wave's staging does not start at a multiple of 16 bytes)
        fits = 0 <= ndw <= cap
        by16 = fits and ndw != 0 and w0 + ((ndw + 3) & ~3) < endw and pad + ((ndw + 7) & ~3) + 4 <= cap + 8
        out.append((by16, ndw if fits else 0))
    return out


def decode_at(qb3, container, index, offset, room=None):
    """decodes the container placed at `offset` bytes of a fresh device buffer of `room` bytes (default: enough), from its table and with
    the index: [(pixels, status)]"""
    import torch
    from qb3_amd import device as qdev
    n = len(container)
    buf = torch.full((offset + (n + 3) // 4 * 4 + 32 if room is None else room,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and offset + n <= buf.numel()
    buf[offset:offset + n] = torch.from_numpy(np.frombuffer(container, dtype=np.uint8).copy())
    src = buf[offset:]
    d_index = torch.from_numpy(index).cuda()
    dec = qdev.DeviceDecoder(src, n)
    got = []
    for ix in (None, d_index):
        out = dec.decode(src, index=ix)
        got.append((out.cpu().numpy(), qb3.lib.qb3x_last_decode_status(dec.p)))
    dec.close()
    return got


@pytest.mark.parametrize("r", RASTERS, ids=ids)
def test_both_paths_at_every_alignment(qb3, r):
    img, container, index = coded(r)
    st = staging(container)
    assert len(st) == (((r[0] + 3) // 4) * ((r[1] + 3) // 4) + 63) // 64
    assert any(by16 for by16, _ in st), "no segment takes the 16-byte path"
    assert not st[-1][0], "the stream's last segment takes the dword path"
    if r[3] == "random" and r[2] >= 3:
        assert max(ndw for _, ndw in st) > 512, "a second round of loads"
    if r[3] == "const":
        assert max(ndw for _, ndw in st) <= 32, "segments of a few words (64 blocks of two bits a unit): most lanes load a clamped address"
    for offset in (0, 4, 8, 12):
        for (out, status), what in zip(decode_at(qb3, container, index, offset), ("from the table", "with the index")):
            assert status == 0, (offset, what)
            assert np.array_equal(out, img.reshape(-1)), "decode %s differs, container at byte %d" % (what, offset)


def test_every_residue_of_the_segment_length(qb3):
    """ndw mod 4 on the 16-byte path (how many words of the last group are zeroed) and on the dword path"""
    fast, tail = set(), set()
    for r in RASTERS:
        for by16, ndw in staging(coded(r)[1]):
            (fast if by16 else tail).add(ndw & 3)
    assert fast == {0, 1, 2, 3}, fast
    assert tail, "no segment takes the dword path"


@pytest.mark.parametrize("r", [RASTERS[1], RASTERS[4]], ids=ids)
def test_container_at_the_end_of_its_allocation(qb3, r):
    """a tensor of exactly the container's size rounded up to 4: the last segment reads no word behind the stream's last"""
    img, container, index = coded(r)
    for (out, status), what in zip(decode_at(qb3, container, index, 0, room=(len(container) + 3) // 4 * 4), ("from the table", "with the index")):
        assert status == 0, what
        assert np.array_equal(out, img.reshape(-1)), what


def test_truncated_stream(qb3, oracle):
    """The container of 260 x 68 x 3 cut inside its last segment (both routes) and in front of it (with the index: the last segment
    begins behind the stream's end, P1 < P0, and reads as zeros).  What is expected comes from the oracle's reader, which like the
    reference's returns zeros past the end (bitstream.h:36): where it decodes, so does the library, to the same pixels, and says
    "the stream ended early" (status bit 2, value 4: the cut takes whole bytes off a stream that had at most 7 spare bits) with no
    error bit; where it does not, the call fails."""
    import torch
    from qb3_amd import device as qdev
    r = RASTERS[1]
    img, container, index = coded(r)
    t, _, t1 = T.parse(container)
    n = len(container)
    last = t1 + int(t.pos[-1]) // 8                  # the byte the last segment starts in
    assert last + 16 < n - 9
    for cut, routes in ((n - 3, (False, True)), (n - 9, (False, True)), (last + 16, (False, True)), (last - 8, (True,))):
        short = np.frombuffer(container, dtype=np.uint8)[:cut].copy()
        st = staging(container, cut)
        assert not st[-1][0], "the cut segment takes the dword path"
        want, _, _, _ = oracle.decode(short, identity=True)
        buf = torch.zeros((cut + 3) // 4 * 4, dtype=torch.uint8, device="cuda")
        buf[:cut] = torch.from_numpy(short)
        d_index = torch.from_numpy(index).cuda()
        for with_index in routes:
            dec = qdev.DeviceDecoder(buf, cut)
            what = (cut - n, "with the index" if with_index else "from the table")
            if want is None:
                with pytest.raises(RuntimeError):
                    dec.decode(buf, index=d_index if with_index else None)
            else:
                out = dec.decode(buf, index=d_index if with_index else None).cpu().numpy()
                status = qb3.lib.qb3x_last_decode_status(dec.p)
                print("truncated stream, cut %d %s: status %d" % (what + (status,)))
                # with the index: "ended early" and nothing else.  From the container alone the table of a longer stream may be
                # set aside first (bit 5, no error: include/qb3x.h) and the stream walked; no error bit (0, 1, 3, 4) either way
                assert status == 4 or (not with_index and status == 4 | 32), what
                # (a segment that begins behind the cut is entered with the rungs and values the INDEX holds, those of the whole
                # stream, the oracle's reader with what the zeros left it: its blocks are not compared)
                keep = np.ones((r[1], r[0]), dtype=bool)
                if cut <= last:
                    nbx = (r[0] + 3) // 4
                    for g in range(64 * (len(t.pos) - 1), nbx * ((r[1] + 3) // 4)):
                        keep[4 * (g // nbx):4 * (g // nbx) + 4, 4 * (g % nbx):4 * (g % nbx) + 4] = False
                    assert keep.sum() == 64 * (len(t.pos) - 1) * 16
                shape = (r[1], r[0], r[2])
                assert np.array_equal(out.reshape(shape)[keep], want.reshape(shape)[keep]), what
            dec.close()
