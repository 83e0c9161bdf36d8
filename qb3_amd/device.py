"""qb3_amd/device.py -- device-resident encode/decode through the qb3x_ C entry points, on torch tensors.

torch only supplies device memory and the stream handle; every byte of work happens inside libQB3.so.
The handles follow the reference's usage pattern (cqb3.cpp:405-493 for encode, :276-323 for decode):
create, set mode / band map, encode; read_start, read_info, read_data.
"""
import ctypes as C

import numpy as np
import torch

from . import lib, last_error, TYPESIZE, NP_DTYPE, QB3M_FTL, _sz, window_array, band_array, RangedReader

_vp = C.c_void_p


def _stream_ptr():
    return _vp(torch.cuda.current_stream().cuda_stream)


class DeviceEncoder:
    """One encoder handle bound to the current device; output and index buffers are reused across calls."""

    def __init__(self, w, h, bands, dtype, mode=QB3M_FTL, cband=None, want_index=True, index_chunk=False):
        self.w, self.h, self.bands, self.dtype = w, h, bands, dtype
        self.p = lib.qb3_create_encoder(w, h, bands, dtype)
        if not self.p:
            raise ValueError("qb3_create_encoder refused the parameters")
        self.mode = lib.qb3_set_encoder_mode(self.p, mode)
        if index_chunk:             # self-indexing container (qb3x.h): one more chunk, up to 64 KB
            lib.qb3x_set_encoder_index_chunk(self.p, int(index_chunk))   # 1: restart table; 2: with block lengths
        if cband is not None:
            arr = (_sz * bands)(*cband)
            lib.qb3_set_encoder_coreband(self.p, bands, arr)
        self.max_size = lib.qb3_max_encoded_size(self.p)
        self.raw_bytes = w * h * bands * TYPESIZE[dtype]
        self.index_bytes = lib.qb3x_index_size(self.p) if want_index else 0
        self.dst = None
        self.index = None

    def close(self):
        if self.p and lib is not None:      # `lib` may already be gone at interpreter shutdown
            lib.qb3_destroy_encoder(self.p)
            self.p = None

    __del__ = close

    def encode(self, src, dst=None, index=None):
        """src: device tensor holding the image bytes.  Returns (dst uint8 tensor, container size, index tensor)."""
        assert src.is_cuda and src.is_contiguous() and src.numel() * src.element_size() >= self.raw_bytes
        if dst is None:
            if self.dst is None:
                self.dst = torch.empty((self.max_size + 3) // 4 * 4, dtype=torch.uint8, device=src.device)
            dst = self.dst
        if index is None and self.index_bytes:
            if self.index is None:
                self.index = torch.empty(self.index_bytes, dtype=torch.uint8, device=src.device)
            index = self.index
        lib.qb3_reset_encoder(self.p)               # independent images: do not carry the band state
        lib.qb3_set_encoder_mode(self.p, self.mode)  # a STORED fallback leaves the handle's mode at 255
        n = lib.qb3x_encode_device(self.p, _vp(src.data_ptr()), _vp(dst.data_ptr()),
                                   _vp(index.data_ptr()) if index is not None else None, _stream_ptr())
        if n == 0:
            raise RuntimeError(f"qb3x_encode_device failed (state {lib.qb3_get_encoder_state(self.p)}): {last_error()}")
        return dst, n, index


class DeviceDecoder:
    """Decoder for one device-resident container.  `container` is the device tensor holding it -- the library then reads
    the few header bytes it needs itself (qb3x_read_start_device: two small copies, whatever the size of a restart table) --
    or a host array holding the container's head up to its "DT" mark (qb3x_read_start)."""

    def __init__(self, container, nbytes):
        nbytes = int(nbytes)
        dims = (_sz * 3)()
        if torch.is_tensor(container):
            self.hdr = None
            self.p = lib.qb3x_read_start_device(_vp(container.data_ptr()), nbytes, dims, _stream_ptr())
            if not self.p:
                raise ValueError("not a QB3 container (or its header does not parse)")
        else:
            self.hdr = np.ascontiguousarray(container, dtype=np.uint8)
            self.p = lib.qb3x_read_start(self.hdr.ctypes.data_as(_vp), min(self.hdr.size, nbytes), nbytes, dims)
            if not self.p:
                raise ValueError("qb3x_read_start rejected the stream")
            if not lib.qb3_read_info(self.p):
                lib.qb3_destroy_decoder(self.p)
                self.p = None
                raise ValueError("qb3_read_info failed (or the host copy ends before the container's DT mark)")
        self.w, self.h, self.bands = dims[0], dims[1], dims[2]
        self.out_bytes = lib.qb3_decoded_size(self.p)
        self.nbytes = nbytes

    def close(self):
        if self.p and lib is not None:
            lib.qb3_destroy_decoder(self.p)
            self.p = None

    __del__ = close

    def decode(self, d_stream, out=None, index=None):
        assert d_stream.is_cuda
        if out is None:
            out = torch.empty(self.out_bytes, dtype=torch.uint8, device=d_stream.device)
        n = lib.qb3x_decode_device(self.p, _vp(d_stream.data_ptr()), _vp(out.data_ptr()),
                                   _vp(index.data_ptr()) if index is not None else None, _stream_ptr())
        if n == 0:
            raise RuntimeError(f"qb3x_decode_device failed: {last_error()}")
        return out

    def decode_window(self, d_stream, x0, y0, w, h, out=None, index=None, bands=None):
        """the w x h window at (x0, y0) of the raster (qb3x_decode_window_device): a device tensor of shape (h, w, bands) and the
        raster's type.  out: a contiguous uint8 device tensor of at least the window's bytes to decode into.  bands: as
        decode_windows (a batch of one: qb3x_decode_windows_bands_device); the tensor's last dimension is len(bands)."""
        assert d_stream.is_cuda
        if bands is not None:
            return self.decode_windows(d_stream, [(x0, y0, w, h)], None if out is None else [out], index, bands)[0]
        dt = lib.qb3_get_type(self.p)
        nbytes = h * w * self.bands * TYPESIZE[dt]
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8, device=d_stream.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= nbytes
        n = lib.qb3x_decode_window_device(self.p, _vp(d_stream.data_ptr()), _vp(index.data_ptr()) if index is not None else None,
                                          x0, y0, w, h, _vp(out.data_ptr()), 0, _stream_ptr())
        if n == 0:
            raise RuntimeError(f"qb3x_decode_window_device failed: {last_error()}")
        return out.view(-1)[:nbytes].view(getattr(torch, NP_DTYPE[dt])).view(h, w, self.bands)

    def set_window_kernels(self, mask):
        """qb3x_set_decoder_window_kernels: rasters beyond the 8-bit ones whose window calls take a window kernel (path 1) --
        qb3_amd.QB3X_WINK_U16: 16-bit rasters of 1, 2, 3, 4, 6, 8 bands with a level-2 table; qb3_amd.QB3X_WINK_CF8: 8-bit rasters of
        1, 3, 4 bands in the common-factor modes; qb3_amd.QB3X_WINK_UNIT: every other FTL / BASE raster with a level-2 table (8-bit
        rasters of 2 or 5 to 16 bands, 16-bit rasters of an odd band count above 4, 32/64-bit rasters of any band count), destinations
        on a multiple of the value size; qb3_amd.QB3X_WINK_CFU: the common-factor streams of those shapes and of one-band 16-bit
        rasters, the same destinations; the bits may be or-ed; 0 (the default): none"""
        lib.qb3x_set_decoder_window_kernels(self.p, int(mask))

    def decode_windows(self, d_stream, rects, out=None, index=None, bands=None):
        """the windows (x0, y0, w, h) of `rects` in ONE call (qb3x_decode_windows_device): a list of device tensors of shape
        (h, w, bands) and the raster's type.  out: a list of contiguous uint8 device tensors, one a window, of at least the
        window's bytes each, to decode into (they may be views of one buffer; they must not overlap).  bands: a sequence of band
        numbers (any order, repeats allowed, 1 to 16 of them): qb3x_decode_windows_bands_device, tensors of shape
        (h, w, len(bands)) that hold those bands only; last_window_gathers() tells whether a window kernel wrote them itself."""
        assert d_stream.is_cuda
        dt = lib.qb3_get_type(self.p)
        rects = [tuple(int(v) for v in r) for r in rects]
        nb_px = self.bands if bands is None else len(bands)
        sizes = [h * w * nb_px * TYPESIZE[dt] for _, _, w, h in rects]
        if out is None:                 # one allocation, every window on a dword
            offs = [0]
            for nb in sizes:
                offs.append(offs[-1] + (nb + 3) // 4 * 4)
            buf = torch.empty(max(offs[-1], 4), dtype=torch.uint8, device=d_stream.device)
            out = [buf[offs[i]:offs[i] + sizes[i]] for i in range(len(rects))]
        assert len(out) == len(rects)
        for o, nb in zip(out, sizes):
            assert o.is_cuda and o.is_contiguous() and o.dtype == torch.uint8 and o.numel() >= nb
        wins = window_array(rects, [o.data_ptr() for o in out])
        d_index = _vp(index.data_ptr()) if index is not None else None
        if bands is None:
            n = lib.qb3x_decode_windows_device(self.p, _vp(d_stream.data_ptr()), d_index, wins, len(rects), _stream_ptr())
        else:
            n = lib.qb3x_decode_windows_bands_device(self.p, _vp(d_stream.data_ptr()), d_index, wins, len(rects), band_array(bands), len(bands),
                                                     _stream_ptr())
        self._nwin = len(rects)
        if n != len(rects):
            raise RuntimeError(f"qb3x_decode_windows{'' if bands is None else '_bands'}_device wrote {n} of {len(rects)} windows: {last_error()}")
        return [o.view(-1)[:nb].view(getattr(torch, NP_DTYPE[dt])).view(h, w, nb_px) for o, nb, (_, _, w, h) in zip(out, sizes, rects)]

    def last_window_gathers(self):
        """qb3x_last_window_gathers: gather launches of the last decode_windows(..., bands=...) -- 0: a window kernel wrote the selected
        bands itself (or the selection was the identity)"""
        return lib.qb3x_last_window_gathers(self.p)

    def reindex(self, d_stream, level, out=None):
        """the container with the restart table this library's encoder writes at `level` (0: none), its coded bytes untouched
        (qb3x_reindex_device).  The decoder must have been made over a host copy of the WHOLE container.  out: a contiguous uint8
        device tensor of at least qb3x_reindex_size bytes that does not overlap d_stream.  Returns (tensor, nbytes)."""
        assert d_stream.is_cuda
        cap = lib.qb3x_reindex_size(self.p, level)
        if not cap:
            raise ValueError("qb3x_reindex_size refused the handle (made over the container's head only?) or the level")
        if out is None:
            out = torch.empty((cap + 3) // 4 * 4, dtype=torch.uint8, device=d_stream.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= cap
        n = lib.qb3x_reindex_device(self.p, _vp(d_stream.data_ptr()), _vp(out.data_ptr()), out.numel(), level, _stream_ptr())
        if n == 0:
            raise RuntimeError(f"qb3x_reindex_device failed (status {lib.qb3x_last_decode_status(self.p)}): {last_error()}")
        return out, n

    @property
    def last_windows(self):
        """the paths of the last decode_windows, one a window (0: not written; 1, 2, 3 as last_window)"""
        return [lib.qb3x_window_path(self.p, i) for i in range(getattr(self, "_nwin", 0))]

    @property
    def last_window(self):
        """(path, segments) of the last decode_window: 1 the window kernel, 2 a strip of block rows + crop, 3 the whole raster + crop"""
        return lib.qb3x_last_window_path(self.p), lib.qb3x_last_window_segments(self.p)


class TileBatchCoder:
    """qb3x_encode_tiles / qb3x_decode_tiles on torch tensors: n independent tiles of one geometry per call, tile i of
    the input at i * raw_bytes, its container at i * pitch of `dst`, its out-of-band index at i * index_bytes."""

    def __init__(self, w, h, bands, dtype, n, mode=QB3M_FTL, device="cuda", want_index=True, index_chunk=False):
        """index_chunk: every tile's container carries its own restart table (include/qb3x.h), so that decode(use_index=False)
        needs nothing but the containers"""
        self.w, self.h, self.bands, self.dtype, self.n, self.mode = w, h, bands, dtype, n, mode
        self.p = lib.qb3_create_encoder(w, h, bands, dtype)
        if not self.p:
            raise ValueError("qb3_create_encoder refused the parameters")
        lib.qb3_set_encoder_mode(self.p, mode)
        lib.qb3x_set_encoder_index_chunk(self.p, int(index_chunk))
        self.raw_bytes = w * h * bands * TYPESIZE[dtype]
        self.pitch = (lib.qb3_max_encoded_size(self.p) + 3) // 4 * 4
        self.index_bytes = lib.qb3x_index_size(self.p) if want_index else 0
        self.dst = torch.empty(n * self.pitch, dtype=torch.uint8, device=device)
        self.index = torch.empty(max(1, n * self.index_bytes), dtype=torch.uint8, device=device) if want_index else None
        self.sizes = (_sz * n)()
        self.d = None

    def close(self):
        if lib is None:
            return
        if self.p:
            lib.qb3_destroy_encoder(self.p)
            self.p = None
        if self.d:
            lib.qb3_destroy_decoder(self.d)
            self.d = None

    __del__ = close

    def encode(self, imgs, first=0, count=None):
        """imgs: device tensor holding the tiles back to back; codes tiles [first, first + count) of it.  Returns their sizes."""
        count = self.n - first if count is None else count
        assert imgs.is_cuda and imgs.is_contiguous() and imgs.numel() * imgs.element_size() >= (first + count) * self.raw_bytes
        sizes = (_sz * count)()
        k = lib.qb3x_encode_tiles(self.p, _vp(imgs.data_ptr() + first * self.raw_bytes), count, self.raw_bytes,
                                  _vp(self.dst.data_ptr() + first * self.pitch), self.pitch,
                                  _vp(self.index.data_ptr() + first * self.index_bytes) if self.index is not None else None,
                                  sizes, _stream_ptr())
        if k != count:
            raise RuntimeError(f"qb3x_encode_tiles coded {k} of {count} tiles: {last_error()}")
        for i in range(count):
            self.sizes[first + i] = sizes[i]
        return list(sizes)

    def decode(self, out, use_index=True):
        """decodes the n containers made by encode() into `out` (n * raw_bytes)."""
        if self.d is None:
            dims = (_sz * 3)()
            self.d = lib.qb3x_read_start_device(_vp(self.dst.data_ptr()), int(self.sizes[0]), dims, _stream_ptr())
            if not self.d:
                raise ValueError("tile 0 does not parse")
        k = lib.qb3x_decode_tiles(self.d, _vp(self.dst.data_ptr()), self.n, self.pitch, self.sizes, _vp(out.data_ptr()), self.raw_bytes,
                                  _vp(self.index.data_ptr()) if (use_index and self.index is not None) else None, _stream_ptr())
        if k != self.n:
            raise RuntimeError(f"qb3x_decode_tiles decoded {k} of {self.n} tiles: {last_error()}")
        return out


class MosaicCoder:
    """qb3x_encode_mosaic / qb3x_decode_mosaic on torch tensors: a W x H raster on the device as a grid of independently coded
    tiles of tw x th pixels, coded from and decoded to the raster where it lies.  Tile k = j * tx + i has its container at
    k * pitch of `dst`, its size in `sizes`, its out-of-band index at k * index_bytes of `index`."""

    def __init__(self, W, H, bands, dtype, tile=(512, 512), mode=QB3M_FTL, index_chunk=False, want_index=False, device="cuda"):
        self.W, self.H, self.bands, self.dtype, self.mode = W, H, bands, dtype, mode
        self.tw, self.th = tile
        tx, ty = _sz(), _sz()
        self.n = lib.qb3x_mosaic_tiles(W, H, self.tw, self.th, C.byref(tx), C.byref(ty))
        self.tx, self.ty = tx.value, ty.value
        self.p = lib.qb3_create_encoder(self.tw, self.th, bands, dtype) if self.n else None
        if not self.p:
            raise ValueError("qb3_create_encoder refused the tile geometry")
        lib.qb3_set_encoder_mode(self.p, mode)
        lib.qb3x_set_encoder_index_chunk(self.p, int(index_chunk))
        self.pitch = (lib.qb3_max_encoded_size(self.p) + 3) // 4 * 4
        self.index_bytes = lib.qb3x_index_size(self.p) if want_index else 0
        self.dst = torch.empty(self.n * self.pitch, dtype=torch.uint8, device=device)
        self.index = torch.empty(max(1, self.n * self.index_bytes), dtype=torch.uint8, device=device) if want_index else None
        self.sizes = (_sz * self.n)()
        self.d = None

    def close(self):
        if lib is None:
            return
        if self.p:
            lib.qb3_destroy_encoder(self.p)
            self.p = None
        if self.d:
            lib.qb3_destroy_decoder(self.d)
            self.d = None

    __del__ = close

    def _raster(self, t):
        """(pointer, stride in values) of a raster tensor: contiguous, or a 2-D / 3-D view whose rows are contiguous"""
        assert t.is_cuda and TYPESIZE[self.dtype] == t.element_size()
        if t.is_contiguous():
            assert t.numel() >= self.W * self.H * self.bands
            return t.data_ptr(), 0
        rowvals = self.W * self.bands
        v = t.reshape(self.H, rowvals) if t.dim() == 3 and t.stride(1) == self.bands and t.stride(2) == 1 else t
        assert v.dim() == 2 and tuple(v.shape) == (self.H, rowvals) and v.stride(1) == 1 and v.stride(0) >= rowvals, \
            "a strided raster is a (H, W * bands) view with contiguous rows"
        return v.data_ptr(), v.stride(0)

    def encode(self, raster):
        """raster: device tensor of the raster's type, contiguous or a strided 2-D view (H, W * bands).  Returns the tile sizes."""
        ptr, stride = self._raster(raster)
        lib.qb3_reset_encoder(self.p)
        lib.qb3_set_encoder_mode(self.p, self.mode)
        k = lib.qb3x_encode_mosaic(self.p, _vp(ptr), self.W, self.H, stride, _vp(self.dst.data_ptr()), self.pitch,
                                   _vp(self.index.data_ptr()) if self.index is not None else None, self.sizes, _stream_ptr())
        if k != self.n:
            raise RuntimeError(f"qb3x_encode_mosaic coded {k} of {self.n} tiles (state {lib.qb3_get_encoder_state(self.p)}): {last_error()}")
        if self.d:                      # the containers changed: parse tile 0 again at the next decode
            lib.qb3_destroy_decoder(self.d)
            self.d = None
        return list(self.sizes)

    def container(self, k):
        """tile k's container: a view of the buffer the object owns"""
        return self.dst[k * self.pitch:k * self.pitch + self.sizes[k]]

    def decode(self, out, use_index=True, compat=None):
        """decodes the containers made by encode() into the raster tensor `out` (as encode takes it)."""
        ptr, stride = self._raster(out)
        if self.d is None:
            dims = (_sz * 3)()
            self.d = lib.qb3x_read_start_device(_vp(self.dst.data_ptr()), int(self.sizes[0]), dims, _stream_ptr())
            if not self.d:
                raise ValueError("tile 0 does not parse")
        if compat is not None:
            lib.qb3x_set_decoder_compat(self.d, int(compat))
        k = lib.qb3x_decode_mosaic(self.d, _vp(self.dst.data_ptr()), self.pitch, self.sizes, self.W, self.H, _vp(ptr), stride,
                                   _vp(self.index.data_ptr()) if (use_index and self.index is not None) else None, _stream_ptr())
        if k != self.n:
            raise RuntimeError(f"qb3x_decode_mosaic decoded {k} of {self.n} tiles: {last_error()}")
        return out

    def decode_windows(self, rects, out=None):
        """rectangles (x0, y0, w, h) of the RASTER from the containers made by encode(), in one call (qb3x_decode_mosaic_windows).
        Returns a list of (h, w, bands) tensors of the raster's type, views of one buffer; or fills `out`, a list of contiguous uint8
        device tensors of at least h * w * bands * value size bytes each.  last_windows() then tells how each went."""
        rects = [tuple(int(v) for v in r) for r in rects]
        pix = self.bands * TYPESIZE[self.dtype]
        sizes = [w * h * pix for (_, _, w, h) in rects]
        if out is None:
            offs = [0]
            for nb in sizes:
                offs.append(offs[-1] + (nb + 7) // 8 * 8)     # (every window on eight bytes: a view of any value type)
            buf = torch.empty(max(offs[-1], 8), dtype=torch.uint8, device=self.dst.device)
            out = [buf[offs[i]:offs[i] + sizes[i]] for i in range(len(rects))]
        assert len(out) == len(rects)
        for o, nb in zip(out, sizes):
            assert o.is_cuda and o.is_contiguous() and o.dtype == torch.uint8 and o.numel() >= nb
        if self.d is None:
            dims = (_sz * 3)()
            self.d = lib.qb3x_read_start_device(_vp(self.dst.data_ptr()), int(self.sizes[0]), dims, _stream_ptr())
            if not self.d:
                raise ValueError("tile 0 does not parse")
        wins = window_array(rects, [o.data_ptr() for o in out])
        n = lib.qb3x_decode_mosaic_windows(self.d, _vp(self.dst.data_ptr()), self.pitch, self.sizes, self.W, self.H, wins, len(rects), _stream_ptr())
        self._nwin = len(rects)
        if n != len(rects):
            raise RuntimeError(f"qb3x_decode_mosaic_windows wrote {n} of {len(rects)} windows: {last_error()}")
        return [o.view(-1)[:nb].view(getattr(torch, NP_DTYPE[self.dtype])).view(h, w, self.bands) for o, nb, (_, _, w, h) in zip(out, sizes, rects)]

    def last_windows(self):
        """of the last decode_windows: ([ok], [path], tiles decoded whole) -- path 1: every piece of the window came from the window
        kernel, 3: at least one from a whole-tile decode, 0: not written"""
        n = getattr(self, "_nwin", 0) if self.d else 0
        return ([bool(lib.qb3x_window_ok(self.d, i)) for i in range(n)], [lib.qb3x_window_path(self.d, i) for i in range(n)],
                lib.qb3x_last_mosaic_whole_tiles(self.d) if self.d else 0)


def profile_enable(on=True):
    """True / 1: every kernel; 2: skip the microsecond kernels (less event traffic in a timed loop); 3: the coding kernels (`*_units`) alone; False / 0: off."""
    lib.qb3x_profile_enable(int(on))


def profile_reset():
    lib.qb3x_profile_reset()


def profile_report():
    """{kernel name: (total ms, launches)} measured with HIP events on the launch stream."""
    buf = C.create_string_buffer(1024)
    lib.qb3x_profile_names(buf, 1024)
    out = {}
    for name in filter(None, buf.value.decode().split(",")):
        ms, cnt = C.c_double(), C.c_uint64()
        if lib.qb3x_profile_get(name.encode(), C.byref(ms), C.byref(cnt)):
            out[name] = (ms.value, cnt.value)
    return out


class RangedDecoder(RangedReader):
    """qb3_amd.open_ranged with device destinations: the container stays where it is (a file, a callable), the windows arrive in
    device memory (qb3x_decode_windows_ranged)."""

    def decode_windows(self, rects, out=None):
        """the windows (x0, y0, w, h) of `rects` in one call: a list of device tensors of shape (h, w, bands) and the raster's type.
        out: as DeviceDecoder.decode_windows."""
        dt = self.dtype
        rects = [tuple(int(v) for v in r) for r in rects]
        sizes = [h * w * self.bands * TYPESIZE[dt] for _, _, w, h in rects]
        if out is None:                 # one allocation, every window on a dword
            offs = [0]
            for nb in sizes:
                offs.append(offs[-1] + (nb + 3) // 4 * 4)
            buf = torch.empty(max(offs[-1], 4), dtype=torch.uint8, device="cuda")
            out = [buf[offs[i]:offs[i] + sizes[i]] for i in range(len(rects))]
        assert len(out) == len(rects)
        for o, nb in zip(out, sizes):
            assert o.is_cuda and o.is_contiguous() and o.dtype == torch.uint8 and o.numel() >= nb
        wins = window_array(rects, [o.data_ptr() for o in out])
        n = lib.qb3x_decode_windows_ranged(self.p, wins, len(rects), _stream_ptr())
        self._after(len(rects))
        if n != len(rects):
            raise RuntimeError(f"qb3x_decode_windows_ranged wrote {n} of {len(rects)} windows: {last_error()}")
        return [o.view(-1)[:nb].view(getattr(torch, NP_DTYPE[dt])).view(h, w, self.bands) for o, nb, (_, _, w, h) in zip(out, sizes, rects)]
