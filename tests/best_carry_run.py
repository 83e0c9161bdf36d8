"""tests/best_carry_run.py REGIME -- the GPU half of tests/test_best_carry.py, a process of its own because the library reads
QB3_BEST_SAMPLE_MIN once.  REGIME: "dense" or "sparse" (the one pattern row of qb3_best_carry.SPARSE_KEEP).  For every case of
qb3_best_carry.CASES: the raster A, a second raster B that begins with the factor A ends on,
and the oracle's stateful Encoder as the reference for
  - qb3_encode of A, twice on one handle with qb3_reset_encoder between: the oracle's bytes both times
  - the same through qb3x_encode_device
  - A, B, A, B on one handle WITHOUT reset, through qb3_encode and through qb3x_encode_device: the oracle's bytes each time -- the
    handle has no getter for the band state it keeps, so the state behind each call is read from the bytes of the next: the last B
    shows the state the second A left (B's first unit has the factor A ends on)
  - the device containers decode back to the pixels
Prints a line a case, then "ok"."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import qb3_best_carry as C  # noqa: E402
import qb3_amd  # noqa: E402
from qb3_amd import device as qdev  # noqa: E402
from oracle import pyoracle as o  # noqa: E402
import torch  # noqa: E402

CF_H = 5


def same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    if len(got) != len(ref) or not np.array_equal(got, ref):
        n = min(len(got), len(ref))
        d = np.nonzero(got[:n] != ref[:n])[0]
        raise AssertionError("%s: %d bytes, the oracle's %d, first differing byte %d" % (what, len(got), len(ref), int(d[0]) if len(d) else n))


def main(regime):
    L = qb3_amd.lib
    for dtype, bands, cband, nrows in C.CASES:
        nbytes = o.TYPESIZE[dtype]
        keep = C.SPARSE_KEEP if regime == "sparse" else None
        a = C.Carry(nbytes, bands, nrows, keep)
        _, end = a.spec()
        # B: other pattern numbers; its first unit has the factor band 0 of A ends on ("the same" only through the handle's state)
        b = C.Carry(nbytes, bands, nrows, keep, turn=3, lead=end[0][1] + 2)
        A, Bimg = a.raster(dtype, cband), b.raster(dtype, cband)
        h, w, _ = a.shape
        e = o.Encoder(w, h, bands, dtype)
        e.set_mode(CF_H)
        if cband is not None:
            e.set_coreband(list(cband))
        refs = [e.encode(x) for x in (A, Bimg, A, Bimg)]
        assert not np.array_equal(refs[1], o.encode(Bimg, dtype, CF_H, cband=None if cband is None else list(cband))), "the state B is entered with is in its bytes"
        what = "type %d x %d, %s" % (dtype, bands, regime)
        # ---- qb3_encode
        p = L.qb3_create_encoder(w, h, bands, dtype)
        L.qb3_set_encoder_mode(p, CF_H)
        if cband is not None:
            L.qb3_set_encoder_coreband(p, bands, (qdev._sz * bands)(*cband))
        dst = np.zeros(L.qb3_max_encoded_size(p), np.uint8)
        for rep in range(2):
            L.qb3_reset_encoder(p)
            n = L.qb3_encode(p, A.ctypes.data, dst.ctypes.data)
            same(dst[:n], refs[0], what + ": qb3_encode, fresh state, call %d" % rep)
        for i, x in enumerate((Bimg, A, Bimg)):
            n = L.qb3_encode(p, x.ctypes.data, dst.ctypes.data)
            same(dst[:n], refs[i + 1], what + ": qb3_encode without reset, raster %d" % (i + 1))
        L.qb3_destroy_encoder(p)
        # ---- qb3x_encode_device
        enc = qdev.DeviceEncoder(w, h, bands, dtype, mode=CF_H, cband=cband)
        ddst = torch.empty((enc.max_size + 3) // 4 * 4, dtype=torch.uint8, device="cuda")
        didx = torch.empty(enc.index_bytes, dtype=torch.uint8, device="cuda")
        srcs = [torch.from_numpy(x.view(np.uint8).reshape(-1)).cuda() for x in (A, Bimg)]
        for rep in range(2):
            L.qb3_reset_encoder(enc.p)
            n = L.qb3x_encode_device(enc.p, qdev._vp(srcs[0].data_ptr()), qdev._vp(ddst.data_ptr()), qdev._vp(didx.data_ptr()), qdev._stream_ptr())
            same(ddst[:n].cpu().numpy(), refs[0], what + ": qb3x_encode_device, fresh state, call %d" % rep)
        L.qb3_reset_encoder(enc.p)
        for i in range(4):
            src = srcs[i % 2]
            n = L.qb3x_encode_device(enc.p, qdev._vp(src.data_ptr()), qdev._vp(ddst.data_ptr()), qdev._vp(didx.data_ptr()), qdev._stream_ptr())
            assert n, "qb3x_encode_device failed: %s" % qb3_amd.last_error()
            same(ddst[:n].cpu().numpy(), refs[i], what + ": qb3x_encode_device without reset, raster %d" % i)
            if i < 2:
                dec = qdev.DeviceDecoder(ddst, n)
                assert torch.equal(dec.decode(ddst, index=didx), src), what + ": decode with the index, raster %d" % i
                if i == 0:
                    assert torch.equal(dec.decode(ddst, index=None), src), what + ": decode without the index"
                dec.close()
        enc.close()
        print("%s: %d + %d units that are not flat, %d bytes" % (what, len(a.units), len(b.units), len(refs[0])), flush=True)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
