"""qb3_amd -- Python access to the MI355X-native QB3 library (qb3_amd/libQB3.so) through its C ABI.

The product is the shared library (sources in qb3_amd/csrc, headers in include/); this module only binds
the C entry points with ctypes so that tests and bench.py can call them.  Nothing here encodes or decodes
by itself and nothing falls back to a CPU implementation: if the library is missing, import fails.

Reference interface mirrored: QB3lib/QB3.h:85-162 (names, argument order, return conventions).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QB3_LIB_PATH") or os.path.join(_HERE, "libQB3.so")     # (QB3_LIB_PATH: a diagnostic build of the library, scratch/variant.sh)

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C qb3_amd/csrc` (there is no CPU fallback)")

# One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 and libQB3.so is linked against the
# system one (same soname).  Whichever is loaded first serves both, and torch does not see the GPU when the
# system copy wins -- so when torch is installed, load it first.  The library itself does not need torch.
try:
    import torch as _torch  # noqa: F401
except ImportError:         # pure C/ctypes use
    _torch = None

lib = C.CDLL(LIB_PATH)

# enum values as in include/QB3.h
QB3_U8, QB3_I8, QB3_U16, QB3_I16, QB3_U32, QB3_I32, QB3_U64, QB3_I64 = range(8)
QB3M_BASE_Z, QB3M_CF, QB3M_RLE, QB3M_CF_RLE, QB3M_BASE_H, QB3M_CF_H, QB3M_RLE_H, QB3M_CF_RLE_H, QB3M_FTL = range(9)
QB3M_DEFAULT, QB3M_BASE, QB3M_BEST, QB3M_STORED, QB3M_INVALID = 8, 4, 7, 255, -1
QB3X_REF_CBAND0 = 1
QB3X_WINK_U16 = 1           # qb3x_set_decoder_window_kernels: the 16-bit window kernels
QB3X_WINK_CF8 = 2           # ... the window kernels of the 8-bit common-factor modes (1, 3, 4 bands)
QB3X_WINK_UNIT = 4          # ... the window kernels of the lane-per-unit rasters and of one-band 32/64-bit rasters (FTL / BASE)
QB3X_WINK_CFU = 8           # ... the window kernels of the common-factor streams of such shapes and of one-band 16-bit rasters
TYPESIZE = (1, 1, 2, 2, 4, 4, 8, 8)

_vp, _sz, _u64 = C.c_void_p, C.c_size_t, C.c_uint64


class Window(C.Structure):
    """qb3x_window (include/qb3x.h): a rectangle of the raster and where its pixels go; dst_stride in values, 0: w * bands"""
    _fields_ = [("x0", _sz), ("y0", _sz), ("w", _sz), ("h", _sz), ("dst", _vp), ("dst_stride", _sz)]


def window_array(rects, ptrs, strides=None):
    """a qb3x_window array from (x0, y0, w, h) tuples, destination addresses and (optional) strides in values"""
    arr = (Window * len(rects))()
    for i, (x0, y0, w, h) in enumerate(rects):
        arr[i] = Window(x0, y0, w, h, ptrs[i], strides[i] if strides else 0)
    return arr


class Range(C.Structure):
    """qb3x_range (include/qb3x.h): a byte range of a container"""
    _fields_ = [("offset", _u64), ("size", _u64)]


READ_FN = C.CFUNCTYPE(C.c_int, _vp, _u64, _vp, _sz)     # qb3x_read_fn: 0 = ok


_PROTOS = {
    # name: (restype, argtypes)            -- include/QB3.h
    "qb3_create_encoder": (_vp, [_sz, _sz, _sz, C.c_int]),
    "qb3_destroy_encoder": (None, [_vp]),
    "qb3_reset_encoder": (None, [_vp]),
    "qb3_set_encoder_coreband": (C.c_bool, [_vp, _sz, C.POINTER(_sz)]),
    "qb3_set_encoder_quanta": (C.c_bool, [_vp, _u64, C.c_bool]),
    "qb3_max_encoded_size": (_sz, [_vp]),
    "qb3_set_encoder_mode": (C.c_int, [_vp, C.c_int]),
    "qb3_set_encoder_stride": (None, [_vp, _sz]),
    "qb3_encode": (_sz, [_vp, _vp, _vp]),
    "qb3_get_encoder_state": (C.c_int, [_vp]),
    "qb3_read_start": (_vp, [_vp, _sz, C.POINTER(_sz)]),
    "qb3_read_info": (C.c_bool, [_vp]),
    "qb3_read_data": (_sz, [_vp, _vp]),
    "qb3_destroy_decoder": (None, [_vp]),
    "qb3_decoded_size": (_sz, [_vp]),
    "qb3_get_type": (C.c_int, [_vp]),
    "qb3_set_decoder_stride": (None, [_vp, _sz]),
    "qb3_get_mode": (C.c_int, [_vp]),
    "qb3_get_quanta": (_u64, [_vp]),
    "qb3_get_order": (_u64, [_vp]),
    "qb3_get_coreband": (C.c_bool, [_vp, C.POINTER(_sz)]),
    # include/qb3x.h
    "qb3x_device_count": (C.c_int, []),
    "qb3x_trim": (None, []),
    "qb3x_last_decode_status": (C.c_uint, [_vp]),
    "qb3x_index_size": (_sz, [_vp]),
    "qb3x_set_encoder_index_chunk": (None, [_vp, C.c_int]),
    "qb3x_decoder_index_size": (_sz, [_vp]),
    "qb3x_encode_device": (_sz, [_vp, _vp, _vp, _vp, _vp]),
    "qb3x_decode_device": (_sz, [_vp, _vp, _vp, _vp, _vp]),
    "qb3x_encode_tiles": (_sz, [_vp, _vp, _sz, _sz, _vp, _sz, _vp, C.POINTER(_sz), _vp]),
    "qb3x_decode_tiles": (_sz, [_vp, _vp, _sz, _sz, C.POINTER(_sz), _vp, _sz, _vp, _vp]),
    "qb3x_decode_tile_ok": (C.c_int, [_vp, _sz]),
    "qb3x_mosaic_tiles": (_sz, [_sz, _sz, _sz, _sz, C.POINTER(_sz), C.POINTER(_sz)]),
    "qb3x_encode_mosaic": (_sz, [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _vp, C.POINTER(_sz), _vp]),
    "qb3x_decode_mosaic": (_sz, [_vp, _vp, _sz, C.POINTER(_sz), _sz, _sz, _vp, _sz, _vp, _vp]),
    "qb3x_mosaic_window_tiles": (_sz, [_sz] * 8 + [C.POINTER(_sz)] * 4),
    "qb3x_decode_mosaic_windows": (_sz, [_vp, _vp, _sz, C.POINTER(_sz), _sz, _sz, _vp, _sz, _vp]),
    "qb3x_last_mosaic_whole_tiles": (_sz, [_vp]),
    "qb3x_decode_window_device": (_sz, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp]),
    "qb3x_read_window": (_sz, [_vp, _sz, _sz, _sz, _sz, _vp, _sz]),
    "qb3x_window_segments": (_sz, [_vp, _sz, _sz, _sz, _sz, C.POINTER(_sz)]),
    "qb3x_last_window_path": (C.c_int, [_vp]),
    "qb3x_last_window_segments": (_sz, [_vp]),
    "qb3x_decode_windows_device": (_sz, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "qb3x_read_windows": (_sz, [_vp, _vp, _sz]),
    "qb3x_window_ok": (C.c_int, [_vp, _sz]),
    "qb3x_window_path": (C.c_int, [_vp, _sz]),
    "qb3x_decode_windows_bands_device": (_sz, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "qb3x_read_windows_bands": (_sz, [_vp, _vp, _sz, _vp, _sz]),
    "qb3x_last_window_gathers": (_sz, [_vp]),
    "qb3x_open_ranged": (_vp, [_vp, _vp, _u64, C.POINTER(_sz)]),
    "qb3x_read_windows_ranged": (_sz, [_vp, _vp, _sz]),
    "qb3x_decode_windows_ranged": (_sz, [_vp, _vp, _sz, _vp]),
    "qb3x_ranged_bytes": (_u64, [_vp]),
    "qb3x_ranged_reads": (_u64, [_vp]),
    "qb3x_set_ranged_gap": (None, [_vp, _sz]),
    "qb3x_set_ranged_cache": (None, [_vp, _sz]),
    "qb3x_ranged_table_ranges": (_sz, [_vp, _vp, _sz, _vp, _sz]),
    "qb3x_read_start": (_vp, [_vp, _sz, _sz, C.POINTER(_sz)]),
    "qb3x_read_start_device": (_vp, [_vp, _sz, C.POINTER(_sz), _vp]),
    "qb3x_header_size_bound": (_sz, [_vp, _sz]),
    "qb3x_decoder_table_entries": (_sz, [_vp]),
    "qb3x_set_decoder_compat": (None, [_vp, C.c_uint]),
    "qb3x_set_decoder_window_kernels": (None, [_vp, C.c_uint]),
    "qb3x_reindex_size": (_sz, [_vp, C.c_int]),
    "qb3x_reindex_device": (_sz, [_vp, _vp, _vp, _sz, C.c_int, _vp]),
    "qb3x_reindex": (_sz, [_vp, _sz, _vp, _sz, C.c_int]),
    "qb3_create_decoder": (_vp, [_vp, _sz, C.POINTER(_sz)]),
    "qb3_decode": (_sz, [_vp, _vp]),
    "qb3x_last_error": (C.c_char_p, []),
    "qb3x_fnv1a64": (_u64, [_vp, _sz, _u64]),
    "qb3x_rle0_device": (_sz, [_vp, _sz, _vp, _sz, C.c_int, _vp]),
    "qb3x_profile_enable": (None, [C.c_int]),
    "qb3x_profile_reset": (None, []),
    "qb3x_profile_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "qb3x_profile_names": (C.c_int, [C.c_char_p, _sz]),
}
for _name, (_res, _args) in _PROTOS.items():
    _f = getattr(lib, _name)        # AttributeError here = the library does not export a declared symbol
    _f.restype, _f.argtypes = _res, _args

EXPORTED = tuple(_PROTOS)


def last_error():
    return lib.qb3x_last_error().decode()


def fnv(*parts):
    """FNV-1a64 (hex) of the concatenation of host arrays."""
    import numpy as np
    h = 0
    for a in parts:
        a = np.ascontiguousarray(a)
        if a.nbytes:
            h = lib.qb3x_fnv1a64(a.ctypes.data_as(_vp), a.nbytes, h)
    return "%016x" % (h or 0xcbf29ce484222325)


def _np_ptr(a):
    return a.ctypes.data_as(_vp)


def encode(img, dtype, mode=QB3M_FTL, cband=None, stride=0, quanta=1, away=False, index_chunk=False):
    """qb3_create_encoder .. qb3_encode on a numpy image of shape (h, w, bands); returns the container bytes."""
    import numpy as np
    h, w, b = img.shape
    p = lib.qb3_create_encoder(w, h, b, dtype)
    if not p:
        raise ValueError("qb3_create_encoder refused the parameters")
    try:
        lib.qb3_set_encoder_mode(p, mode)
        if index_chunk:
            lib.qb3x_set_encoder_index_chunk(p, int(index_chunk))      # 1: restart table; 2: with block lengths
        if cband is not None:
            arr = (_sz * b)(*cband)
            lib.qb3_set_encoder_coreband(p, b, arr)
        if stride:
            lib.qb3_set_encoder_stride(p, stride)
        if quanta > 1:
            lib.qb3_set_encoder_quanta(p, quanta, away)
        dst = np.empty(lib.qb3_max_encoded_size(p), dtype=np.uint8)
        src = np.ascontiguousarray(img)
        n = lib.qb3_encode(p, _np_ptr(src), _np_ptr(dst))
        if n == 0:
            raise RuntimeError(f"qb3_encode failed, state {lib.qb3_get_encoder_state(p)}: {last_error()}")
        return dst[:n].copy()
    finally:
        lib.qb3_destroy_encoder(p)


def decode(stream, compat=0):
    """qb3_read_start .. qb3_read_data; returns (flat uint8 array of decoded bytes, (w, h, bands), dtype, mode)."""
    import numpy as np
    buf = np.ascontiguousarray(stream, dtype=np.uint8)
    dims = (_sz * 3)()
    p = lib.qb3_read_start(_np_ptr(buf), buf.size, dims)
    if not p:
        raise ValueError("qb3_read_start rejected the stream")
    try:
        if not lib.qb3_read_info(p):
            raise ValueError("qb3_read_info failed")
        if compat:
            lib.qb3x_set_decoder_compat(p, compat)
        out = np.empty(lib.qb3_decoded_size(p), dtype=np.uint8)
        n = lib.qb3_read_data(p, _np_ptr(out))
        if n == 0:
            raise RuntimeError(f"qb3_read_data failed: {last_error()}")
        return out[:n], tuple(dims), lib.qb3_get_type(p), lib.qb3_get_mode(p)
    finally:
        lib.qb3_destroy_decoder(p)


NP_DTYPE = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64")      # numpy / torch names of the qb3_dtype codes


def decode_window(stream, x0, y0, w, h, compat=0):
    """qb3_read_start .. qb3x_read_window: the w x h window at (x0, y0) of a container in host memory, as an array of shape
    (h, w, bands) and the raster's type."""
    import numpy as np
    buf = np.ascontiguousarray(stream, dtype=np.uint8)
    dims = (_sz * 3)()
    p = lib.qb3_read_start(_np_ptr(buf), buf.size, dims)
    if not p:
        raise ValueError("qb3_read_start rejected the stream")
    try:
        if not lib.qb3_read_info(p):
            raise ValueError("qb3_read_info failed")
        if compat:
            lib.qb3x_set_decoder_compat(p, compat)
        out = np.empty((h, w, dims[2]), dtype=NP_DTYPE[lib.qb3_get_type(p)])
        n = lib.qb3x_read_window(p, x0, y0, w, h, _np_ptr(out), 0)
        if n == 0:
            raise RuntimeError(f"qb3x_read_window failed: {last_error()}")
        return out
    finally:
        lib.qb3_destroy_decoder(p)


def band_array(bands):
    """the `sel` array of the band-selected window calls (uint8 band numbers) from a sequence of ints"""
    bands = [int(b) for b in bands]
    if any(b < 0 or b > 255 for b in bands):
        raise ValueError("band numbers are 0 .. 255")
    return (C.c_uint8 * len(bands))(*bands)


def decode_windows(stream, rects, compat=0, bands=None):
    """qb3_read_start .. qb3x_read_windows: the windows (x0, y0, w, h) of `rects` of a container in host memory -- one upload, one
    decode call -- as a list of arrays of shape (h, w, bands) and the raster's type.  bands: a sequence of band numbers (any order,
    repeats allowed, 1 to 16 of them): qb3x_read_windows_bands, arrays of shape (h, w, len(bands)) that hold those bands only."""
    import numpy as np
    buf = np.ascontiguousarray(stream, dtype=np.uint8)
    dims = (_sz * 3)()
    p = lib.qb3_read_start(_np_ptr(buf), buf.size, dims)
    if not p:
        raise ValueError("qb3_read_start rejected the stream")
    try:
        if not lib.qb3_read_info(p):
            raise ValueError("qb3_read_info failed")
        if compat:
            lib.qb3x_set_decoder_compat(p, compat)
        rects = [tuple(int(v) for v in r) for r in rects]
        outs = [np.empty((h, w, dims[2] if bands is None else len(bands)), dtype=NP_DTYPE[lib.qb3_get_type(p)]) for _, _, w, h in rects]
        wins = window_array(rects, [o.ctypes.data for o in outs])
        if bands is None:
            n = lib.qb3x_read_windows(p, wins, len(rects))
        else:
            n = lib.qb3x_read_windows_bands(p, wins, len(rects), band_array(bands), len(bands))
        if n != len(rects):
            raise RuntimeError(f"qb3x_read_windows{'' if bands is None else '_bands'} wrote {n} of {len(rects)} windows: {last_error()}")
        return outs
    finally:
        lib.qb3_destroy_decoder(p)


def reindex(stream, level):
    """qb3x_reindex: the container with its restart table dropped (level 0) or replaced by the one this library's encoder writes at
    level 1 or 2; the coded bytes are not touched.  Returns the new container as a uint8 array."""
    import numpy as np
    buf = np.ascontiguousarray(stream, dtype=np.uint8)
    dims = (_sz * 3)()
    p = lib.qb3_read_start(_np_ptr(buf), buf.size, dims)
    if not p:
        raise ValueError("qb3_read_start rejected the stream")
    try:
        cap = lib.qb3x_reindex_size(p, level) if lib.qb3_read_info(p) else 0
    finally:
        lib.qb3_destroy_decoder(p)
    if not cap:
        raise ValueError("qb3x_reindex_size refused the container or the level")
    out = np.empty(cap, dtype=np.uint8)
    n = lib.qb3x_reindex(_np_ptr(buf), buf.size, _np_ptr(out), cap, level)
    if n == 0:
        raise RuntimeError(f"qb3x_reindex failed: {last_error()}")
    return out[:n]


class RangedReader:
    """qb3x_open_ranged: windows of a container that is NOT in memory -- a file, or anything a callable reads byte ranges of --
    fetching only the table chunks and the pieces of the stream that hold the rectangles (include/qb3x.h).  `source`: a path, or a
    callable (offset, size) -> bytes-like of exactly `size` bytes (then `size` is the container's size).  last_bytes / last_reads:
    what the last call asked of the source; last_windows: the path every window of it came by.  window_kernels: set_window_kernels."""

    def __init__(self, source, size=None, window_kernels=0):
        import numpy as np
        self._file = None
        if callable(source):
            if size is None:
                raise ValueError("a callable source needs the container's size")
            read = source
        else:
            self._file = open(source, "rb")
            size = os.fstat(self._file.fileno()).st_size if size is None else size
            fd = self._file.fileno()
            read = lambda off, n: os.pread(fd, n, off)  # noqa: E731

        def rd(_ctx, off, dst, n):
            try:
                got = np.frombuffer(read(off, n), np.uint8)
                if got.size != n:
                    return 1
                C.memmove(dst, got.ctypes.data, n)
                return 0
            except Exception:       # (no exception crosses the C ABI)
                return 1
        self._rd = READ_FN(rd)      # referenced for the handle's life: the library calls it until close()
        self.size = int(size)
        dims = (_sz * 3)()
        self.p = lib.qb3x_open_ranged(self._rd, None, self.size, dims)
        if not self.p:
            self.close()
            raise ValueError("qb3x_open_ranged: not a QB3 container, or the source could not be read")
        self.width, self.height, self.bands = (int(v) for v in dims)
        self.dtype = lib.qb3_get_type(self.p)
        self.last_bytes = self.last_reads = 0
        self.last_windows = []
        if window_kernels:
            self.set_window_kernels(window_kernels)

    def set_window_kernels(self, mask):
        """qb3x_set_decoder_window_kernels on the ranged handle: QB3X_WINK_U16 -- 16-bit rasters of 1, 2, 3, 4, 6, 8 bands with a
        level-2 table are read in pieces too (else they are read whole, every call); QB3X_WINK_CF8 -- so are 8-bit rasters of 1, 3, 4
        bands in the common-factor modes whose table carries block fields; QB3X_WINK_UNIT and QB3X_WINK_CFU add no ranged shortcut (the
        container is read whole, once; its windows then take the window kernel from the uploaded copy); 0 (the default): none"""
        lib.qb3x_set_decoder_window_kernels(self.p, int(mask))

    def set_gap(self, nbytes):
        lib.qb3x_set_ranged_gap(self.p, nbytes)

    def set_cache(self, nbytes):
        lib.qb3x_set_ranged_cache(self.p, nbytes)

    def _after(self, n):
        self.last_bytes, self.last_reads = lib.qb3x_ranged_bytes(self.p), lib.qb3x_ranged_reads(self.p)
        self.last_windows = [lib.qb3x_window_path(self.p, i) for i in range(n)]

    def read_windows(self, rects):
        """qb3x_read_windows_ranged: the windows (x0, y0, w, h) as a list of arrays of shape (h, w, bands)"""
        import numpy as np
        rects = [tuple(int(v) for v in r) for r in rects]
        outs = [np.empty((h, w, self.bands), dtype=NP_DTYPE[self.dtype]) for _, _, w, h in rects]
        wins = window_array(rects, [o.ctypes.data for o in outs])
        n = lib.qb3x_read_windows_ranged(self.p, wins, len(rects))
        self._after(len(rects))
        if n != len(rects):
            raise RuntimeError(f"qb3x_read_windows_ranged wrote {n} of {len(rects)} windows: {last_error()}")
        return outs

    def close(self):
        if getattr(self, "p", None):
            lib.qb3_destroy_decoder(self.p)
        self.p = None
        if self._file is not None:
            self._file.close()
            self._file = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open_ranged(path_or_callable, size=None, window_kernels=0):
    """a RangedReader over a file or a callable (offset, size) -> bytes; window_kernels: RangedReader.set_window_kernels"""
    return RangedReader(path_or_callable, size, window_kernels)
