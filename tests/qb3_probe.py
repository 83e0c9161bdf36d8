"""tests/qb3_probe.py -- ctypes binding of libqb3probe.so (qb3_amd/csrc/probe_readers.hip), the test instrument of the bit readers"""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def load():
    """the probe library (QB3_PROBE_LIB: another build of it); import qb3_amd first, so that one HIP runtime serves both"""
    global _lib
    if _lib is None:
        import qb3_amd  # noqa: F401
        lib = C.CDLL(os.environ.get("QB3_PROBE_LIB") or os.path.join(ROOT, "qb3_amd", "libqb3probe.so"))
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        lib.probe_values.argtypes = [vp, u64, vp, vp, vp, u32, u32, u32, u32, vp, vp]
        lib.probe_groups.argtypes = [vp, u64, vp, vp, vp, u32, u32, u32, u32, u32, vp, vp]
        lib.probe_units.argtypes = [vp, u64, vp, vp, u32, u32, u32, u32, u32, vp, vp, vp]
        lib.probe_dirty.argtypes = [u32, vp, u32, vp]
        for f in (lib.probe_values, lib.probe_groups, lib.probe_units, lib.probe_dirty):
            f.restype = C.c_int
        _lib = lib
    return _lib


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dirty(pattern):
    """fill every CU's LDS and a few hundred registers of every lane with `pattern` (on the current stream)"""
    import torch
    sums = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert load().probe_dirty(pattern, C.c_void_p(sums.data_ptr()), 64, stream()) == 0
    torch.cuda.synchronize()
