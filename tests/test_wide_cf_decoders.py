"""Whole-kernel parity of the 32/64-bit common-factor decoders on a dirty device.

Every decoder that still reads values through the branchy reader (ReaderT + get_value via parse_unit / get_group) against the oracle:
  - one band: dec_pxw_best_kernel (k_dec_pxw.hip) for the index and both tables; the plain stream through the walk by exits
    (k_dec_walk_exit.hip)
  - several bands: dec_pxu_best_kernel (k_dec_pxu.hip) for the index and both tables; the plain stream through the one-wave walk
    (dec_index_walk_best, k_dec_generic.hip) and the lane-per-unit totals
  - with QB3_NO_PX (a child process): the generic dec_kernel (k_dec_generic.hip, profile name dec_segments)
The profile name of all the lane-per-block / lane-per-unit decoders is dec_units.  Rasters: a smooth field with noise times a common
factor, scaled so that the divided values code at rungs 17..20 and, for 64-bit data, above 32.  Each decode runs once right behind an
encode of the same raster -- itself behind an encode of a RANDOM raster of the same footprint whose handle was closed, so that the
pool hands its buffers on holding another call's bytes -- and once right after probe_dirty.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_probe as P  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPT = {4: np.uint32, 5: np.int32, 6: np.uint64, 7: np.int64}

# w, h, bands, dtype, mode, factor, noise bits (rung of the divided values), band map (None: identity)
CASES = [
    (64, 64, 1, 5, 7, 5, 18, None),
    (509, 259, 1, 4, 5, 5, 19, None),
    (1021, 515, 1, 7, 1, 1 << 24, 33, None),
    (640, 386, 1, 6, 3, 5, 46, None),
    (256, 130, 1, 7, 7, 1 << 56, 5, None),
    (130, 70, 2, 5, 7, 5, 17, [1, 1]),
    (1030, 514, 2, 7, 7, 5, 34, None),
    (515, 259, 3, 6, 5, 1 << 24, 20, [1, 1, 1]),
    (300, 200, 3, 7, 3, 5, 44, None),
    (257, 131, 5, 4, 1, 5, 18, [1, 1, 1, 3, 4]),
    (200, 100, 5, 7, 7, 1 << 24, 31, None),
    (4096, 4096, 2, 7, 7, 5, 20, None),
    (4096, 4096, 3, 7, 7, 5, 33, [1, 1, 1]),
]


def _ids(c):
    w, h, b, dt, mode, f, k, cb = c
    kern = "pxw_best" if b == 1 else "pxu_best"
    return "%dx%dx%d-t%d-m%d-x%d-r%d-%s%s" % (w, h, b, dt, mode, f, k, kern, "-map" if cb else "")


def raster(w, h, b, dt, factor, k, seed):
    """smooth field + noise of k bits, times the factor, in the type (the product fits)"""
    rng = np.random.default_rng(seed)
    bits = 32 if dt in (4, 5) else 64
    y, x = np.mgrid[0:h, 0:w]
    room = bits - 2 - factor.bit_length()
    amp = 1 << max(min(room, k + 2) - 1, 0)
    f = np.empty((h, w, b), dtype=np.int64)
    for c in range(b):
        smooth = (np.sin(x / 37.0 + c) * np.cos(y / 23.0) * (amp // 2)).astype(np.int64)
        noise = rng.integers(0, 1 << min(k, room), size=(h, w), dtype=np.int64)
        f[:, :, c] = smooth + noise + (amp if dt in (4, 6) else 0)
    if bits == 32:
        return (f * factor).astype(np.int64).astype(NPT[dt])
    return (f.astype(np.uint64) * np.uint64(factor)).view(np.int64).astype(NPT[dt]) if dt == 7 else (f.astype(np.uint64) * np.uint64(factor))


def kernels_of(qb3, fn):
    import ctypes as C
    L = qb3.lib
    L.qb3x_profile_enable(1)
    L.qb3x_profile_reset()
    r = fn()
    buf = C.create_string_buffer(2048)
    L.qb3x_profile_names(buf, 2048)
    L.qb3x_profile_enable(0)
    return r, set(buf.value.decode().split(","))


def run_case(qb3, oracle, case, generic=False):
    """the container is the oracle's; the four decodes right behind an encode (after another raster's pool bytes) and after probe_dirty"""
    import torch
    from qb3_amd import device as qdev
    w, h, b, dt, mode, factor, k, cb = case
    img = raster(w, h, b, dt, factor, k, w + b)
    cbm = cb if cb is not None else list(range(b))
    ref = oracle.encode(img, dt, mode, cband=cbm, fix_b2=True)
    assert ref[10] != 255, "stored raw: the case reaches no decoder"
    dimg = torch.from_numpy(img.view(np.uint8).reshape(-1).copy()).cuda()
    junk = torch.from_numpy(oracle.generate(w, h, b, dt, "RANDOM", 5).view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.empty_like(dimg)
    seen = {}
    for way, level in (("index", 0), ("plain", 0), ("table 1", 1), ("table 2", 2)):
        for dirty in (False, True):
            e0 = qdev.DeviceEncoder(w, h, b, dt, mode=mode, cband=cbm)        # another call's bytes in the pooled buffers
            e0.encode(junk)
            torch.cuda.synchronize()
            e0.close()
            enc = qdev.DeviceEncoder(w, h, b, dt, mode=mode, cband=cbm, index_chunk=level)
            dst, n, index = enc.encode(dimg)
            if level == 0:
                assert n == len(ref) and torch.equal(dst[:n].cpu(), torch.from_numpy(ref)), (way, "the device container is not the oracle's")
            dec = qdev.DeviceDecoder(dst, n)
            if dirty:
                P.dirty(0xA5C3F00F if way in ("index", "table 1") else 0x3C3C96E1)
            out.fill_(0x77)
            _, names = kernels_of(qb3, lambda: dec.decode(dst, out=out, index=index if way == "index" else None))
            torch.cuda.synchronize()
            st = qb3.lib.qb3x_last_decode_status(dec.p)
            assert st & ~64 == 0, (way, dirty, st)             # (bit 6: the walk by exits handed windows to its hopping lane, not an error)
            if not torch.equal(out, dimg):
                at = int(torch.nonzero(out != dimg)[0][0]) // img.itemsize
                pytest.fail("%s decode%s: %d bytes differ, first at value %d (x %d, y %d, band %d)" % (
                    way, " after probe_dirty" if dirty else "", int((out != dimg).sum()), at, at // b % w, at // b // w, at % b))
            seen[way] = names
            dec.close()
            enc.close()
    for way in ("index", "table 2"):
        want = "dec_segments" if generic else "dec_units"
        other = "dec_units" if generic else "dec_segments"
        assert want in seen[way] and other not in seen[way], (way, seen[way])
    return seen


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_wide_common_factor_decoders_on_a_dirty_device(qb3, oracle, case):
    run_case(qb3, oracle, case)


def test_generic_common_factor_decoder_on_a_dirty_device(qb3, oracle, tmp_path):
    """QB3_NO_PX: the same flow through the generic lane-per-segment decoder (dec_kernel, dec_segments); the switch is read once per
    process, a child process"""
    code = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import qb3_amd
from oracle import pyoracle as o
import test_wide_cf_decoders as T
for c in [T.CASES[1], T.CASES[6], T.CASES[9]]:
    T.run_case(qb3_amd, o, c, generic=True)
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, QB3_NO_PX="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
