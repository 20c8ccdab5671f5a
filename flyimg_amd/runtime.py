"""Host-side runtime over the C-ABI: one ``Context`` per process per GPU.

Thin, allocation-light wrappers: numpy arrays in, numpy arrays out for the
host path (``fi_process_batch``), raw device pointers for device-resident
batches (``fi_process_batch_device``, used by bench.py).
"""
from __future__ import annotations

import contextlib
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib as L


@dataclass
class Op:
    """One image's operator list -- the fields of fi_image a caller sets.
    Mirrors the convert argv ImageProcessor::generateCommand builds
    (ImageProcessor.php:66-110)."""

    target_w: int = 0
    target_h: int = 0
    flags: int = L.FI_OP_THUMBNAIL
    gravity: int = L.GRAVITY["Center"]
    rotate: int = 0
    smartcrop_w: int = 0
    smartcrop_h: int = 0
    # forwarded -unsharp / -sharpen / -blur (FI_OP_UNSHARP / SHARPEN / BLUR)
    unsharp: tuple = (0.0, 1.0, 1.0, 0.05)
    sharpen: tuple = (0.0, 1.0)
    blur: tuple = (0.0, 1.0)
    # -background 0x00RRGGBB (FI_OP_BACKGROUND); -1: not given (IM's white)
    background: int = -1


def _fill(img: L.FiImage, op: Op):
    img.target_w, img.target_h = op.target_w, op.target_h
    img.flags, img.gravity, img.rotate = op.flags, op.gravity, op.rotate
    img.smartcrop_w, img.smartcrop_h = op.smartcrop_w, op.smartcrop_h
    for k in range(4):
        img.unsharp[k] = op.unsharp[k]
    for k in range(2):
        img.sharpen[k] = op.sharpen[k]
        img.blur[k] = op.blur[k]
    if op.background >= 0:
        img.background = op.background & 0xFFFFFF
        img.flags |= L.FI_OP_BACKGROUND


def plan(width: int, height: int, op: Op):
    """fi_plan for one image: (out_w, out_h, out_channels) before smart-crop apply."""
    img = L.FiImage()
    img.src_w, img.src_h, img.src_stride, img.src_channels = width, height, width * 3, 3
    _fill(img, op)
    L.check(L.lib().fi_plan(ctypes.byref(img), 1))
    return img.out_w, img.out_h, img.out_channels


def plan_bytes(sizes_ops):
    """fi_plan_bytes: SURVEY 8(e) B_img (algorithmic HBM bytes) of each
    (width, height, Op); -1 where the image does not plan."""
    n = len(sizes_ops)
    arr = (L.FiImage * max(n, 1))()
    for i, (w, h, op) in enumerate(sizes_ops):
        a = arr[i]
        a.src_w, a.src_h, a.src_stride, a.src_channels = w, h, w * 3, 3
        _fill(a, op)
    out = (ctypes.c_int64 * max(n, 1))()
    L.lib().fi_plan_bytes(arr, n, out)  # per-image -1 on failure; the caller decides
    return [int(out[i]) for i in range(n)]


def jpeg_info(blob: bytes, progressive: bool = False):
    """(width, height, channels) of a JPEG the GPU decoder handles, else None
    (fi_jpeg_info: progressive, CMYK, 4:1:1, ... decode on the host).
    ``progressive=True`` (fi_jpeg_info_ex, FI_JPEG_PROGRESSIVE) also takes
    complete Huffman progressive streams."""
    w, h, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    if progressive:
        rc = L.lib().fi_jpeg_info_ex(blob, len(blob), L.FI_JPEG_PROGRESSIVE, ctypes.byref(w), ctypes.byref(h),
                                     ctypes.byref(c), None, None)
    else:
        rc = L.lib().fi_jpeg_info(blob, len(blob), ctypes.byref(w), ctypes.byref(h), ctypes.byref(c))
    return (w.value, h.value, c.value) if rc == L.FI_OK else None


def jpeg_orientation(blob: bytes):
    """fi_jpeg_orientation (host only): the EXIF orientation 1..8 that
    ``ImageOps.exif_transpose`` would apply to this JPEG (1: none); None where
    the library cannot tell without more than an IFD0 lookup (several Exif
    segments, XMP, a malformed TIFF structure) or the input is not a JPEG."""
    o = ctypes.c_int32()
    rc = L.lib().fi_jpeg_orientation(blob, len(blob), ctypes.byref(o))
    return o.value if rc == L.FI_OK else None


def jpeg_view_dims(w: int, h: int, view):
    """(w, h) of what a (orientation 1..8, x, y, w, h) view of a w x h source
    decodes to; ``view`` None: the source's."""
    if view is None:
        return w, h
    o, _, _, vw, vh = view
    if vw or vh:
        return vw, vh
    return (h, w) if o >= 5 else (w, h)


def jpeg_scan_info(blob: bytes):
    """(width, height, channels, nscans, nlevels) of a JPEG the GPU decoder
    handles with FI_JPEG_PROGRESSIVE (fi_jpeg_info_ex: a baseline stream is one
    scan in one level; a progressive stream's scans run in ``nlevels``
    launches), else None.  ``jpeg_scan_status`` tells invalid from unsupported."""
    return jpeg_scan_status(blob)[1]


def jpeg_scan_status(blob: bytes):
    """(status, info): fi_jpeg_info_ex's return code under FI_JPEG_PROGRESSIVE
    (0, FI_EUNSUPPORTED: decode on the host, FI_EINVAL: malformed) and
    jpeg_scan_info's tuple (None unless the status is 0)."""
    v = [ctypes.c_int32() for _ in range(5)]
    rc = L.lib().fi_jpeg_info_ex(blob, len(blob), L.FI_JPEG_PROGRESSIVE, *[ctypes.byref(x) for x in v])
    return rc, (tuple(x.value for x in v) if rc == L.FI_OK else None)


def jpeg_coefs_host(blob: bytes, progressive: bool = True):
    """fi_debug_jpeg_coefs_host (test hook): a progressive stream's entropy
    decode on the CPU -- ([int16 (bh, bw, 64) zigzag blocks per component],
    [uint16 (64,) natural-order quant table per component]), or None."""
    flags = L.FI_JPEG_PROGRESSIVE if progressive else 0
    info = (ctypes.c_int32 * 7)()
    qt = np.zeros(192, np.uint16)
    fn = L.lib().fi_debug_jpeg_coefs_host
    if fn(blob, len(blob), flags, info, qt.ctypes.data, None, 0) != L.FI_OK:
        return None
    n = info[0]
    sizes = [info[1 + k] * info[4 + k] * 64 for k in range(3)]
    co = np.zeros(sum(sizes), np.int16)
    L.check(fn(blob, len(blob), flags, info, qt.ctypes.data, co.ctypes.data, co.size))
    offs = np.cumsum([0] + sizes)
    return ([co[offs[k]:offs[k + 1]].reshape(info[4 + k], info[1 + k], 64) for k in range(n)],
            [qt[64 * k:64 * k + 64] for k in range(n)])


def jpeg_encode_bound(w: int, h: int, channels: int, quality: int, subsampling: int = 0,
                      progressive: bool = False) -> int:
    """fi_jpeg_encode_bound: an upper bound of the GPU encoder's file size for
    any image of this geometry (host only); raises FiError for arguments the
    encoder turns down.  ``progressive``: the bound of the progressive encoder
    (fi_jpeg_encode_bound_ex with FI_JPEG_ENC_PROGRESSIVE)."""
    n = ctypes.c_size_t()
    if progressive:
        L.check(L.lib().fi_jpeg_encode_bound_ex(w, h, channels, quality, subsampling, L.FI_JPEG_ENC_PROGRESSIVE,
                                                ctypes.byref(n)))
    else:
        L.check(L.lib().fi_jpeg_encode_bound(w, h, channels, quality, subsampling, ctypes.byref(n)))
    return n.value


def jpeg_prog_write_host(coefs, w: int, h: int, channels: int, quality: int, subsampling: int = 0):
    """fi_debug_jpeg_prog_write_host (test hook): the progressive encoder's host
    model on quantised coefficients -- the per-component (bh, bw, 64) arrays
    of ``jpeg_coefs_host`` -- as (file bytes, correction-buffer flushes inside
    EOB runs)."""
    co = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int16).ravel() for c in coefs]))
    cap = jpeg_encode_bound(w, h, channels, quality, subsampling, progressive=True)
    out = np.empty(cap, np.uint8)
    n, fl = ctypes.c_size_t(), ctypes.c_int32()
    L.check(L.lib().fi_debug_jpeg_prog_write_host(co.ctypes.data, co.size, w, h, channels, quality, subsampling,
                                                  out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(fl)))
    return out[:n.value].tobytes(), fl.value


def png_encode_bound(w: int, h: int, channels: int) -> int:
    """fi_png_encode_bound: the true upper bound of the GPU PNG encoder's file
    size for any image of this geometry (host only); raises FiError for
    arguments the encoder turns down."""
    n = ctypes.c_size_t()
    L.check(L.lib().fi_png_encode_bound(w, h, channels, ctypes.byref(n)))
    return n.value


def webp_encode_bound(w: int, h: int, channels: int) -> int:
    """fi_webp_encode_bound: the true upper bound of the GPU lossless WebP
    encoder's file size for any image of this geometry (host only); raises
    FiError for arguments the encoder turns down."""
    n = ctypes.c_size_t()
    L.check(L.lib().fi_webp_encode_bound(w, h, channels, ctypes.byref(n)))
    return n.value


def webp_encode_host_form(image: np.ndarray, predictor: int = -1) -> bytes:
    """fi_debug_webp_encode_host (no GPU): the lossless WebP file of a host
    array (HW, or HWC with 1..4 channels) from the code the device runs --
    the device's file, byte for byte."""
    a = np.ascontiguousarray(image, dtype=np.uint8)
    h, w = a.shape[:2]
    c = a.shape[2] if a.ndim == 3 else 1
    cap = webp_encode_bound(w, h, c)
    out = np.empty(cap, np.uint8)
    n = ctypes.c_size_t()
    L.check(L.lib().fi_debug_webp_encode_host(a.ctypes.data, w, h, c, w * c, predictor, out.ctypes.data, cap,
                                              ctypes.byref(n)))
    return out[:n.value].tobytes()


def png_info(blob: bytes):
    """fi_png_info: (width, height, channels, colour type, meta) of a PNG file
    the GPU decoder reproduces exactly (8-bit, non-interlaced; channels = the
    natural count, a palette counts 3, with tRNS 4; meta: FI_PNG_META_ORIENT
    when a chunk could carry an orientation), else None: decode on the host."""
    v = [ctypes.c_int32() for _ in range(5)]
    rc = L.lib().fi_png_info(blob, len(blob), *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v) if rc == L.FI_OK else None


class Context:
    def __init__(self, device: int = 0):
        self._lib = L.lib()
        h = ctypes.c_void_p()
        L.check(self._lib.fi_create(ctypes.byref(h), device))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            for ptr in list(getattr(self, "_pinned", {})):
                self._lib.fi_host_free(self.h, ptr)
        self._pinned = {}
        if self.h:
            self._lib.fi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- host batches ----------------------------------------------------
    def pixelate_regions(self, image: np.ndarray, boxes) -> int:
        """fi_pixelate_regions: the face-blur mogrify (-region box -scale 10%
        -scale 1000%) of each (x, y, w, h) box in order, in place on an 8-bit HWC
        (or HW gray) numpy image.  Returns the C-ABI status (boxes before a
        rejected one are applied, as consecutive mogrify runs would be)."""
        assert image.dtype == np.uint8 and image.flags["C_CONTIGUOUS"]
        h, w = image.shape[:2]
        ch = image.shape[2] if image.ndim == 3 else 1
        flat = [int(v) for b in boxes for v in b]
        arr = (ctypes.c_int32 * max(len(flat), 1))(*flat)
        return self._lib.fi_pixelate_regions(self.h, image.ctypes.data, w, h, image.strides[0], ch, arr,
                                             len(flat) // 4)

    def process(self, images: list[np.ndarray], ops: list[Op]):
        """Run a batch of RGB8 HWC numpy images; returns (outputs, fi_image records)."""
        n = len(images)
        arr = (L.FiImage * n)()
        outs = []
        keep = []
        for i, (src, op) in enumerate(zip(images, ops)):
            src = np.ascontiguousarray(src, dtype=np.uint8)
            keep.append(src)
            img = arr[i]
            img.src = src.ctypes.data
            img.src_h, img.src_w = src.shape[:2]
            img.src_stride = src.strides[0]
            img.src_channels = src.shape[2] if src.ndim == 3 else 1
            _fill(img, op)
        L.lib().fi_plan(arr, n)  # per-image status decides below
        for i in range(n):
            cap = max(arr[i].out_w * arr[i].out_h * max(arr[i].out_channels, 1), 1)
            buf = np.zeros(cap, np.uint8)
            outs.append(buf)
            arr[i].dst = buf.ctypes.data
            arr[i].dst_capacity = cap
        rc = self._lib.fi_process_batch(self.h, arr, n)
        results = []
        for i in range(n):
            a = arr[i]
            if a.status == L.FI_OK:
                o = outs[i][: a.out_h * a.out_stride].reshape(a.out_h, a.out_w, a.out_channels)
                results.append(o[:, :, 0] if a.out_channels == 1 else o)
            else:
                results.append(None)
        return results, arr, rc

    # ---- pinned host buffers + asynchronous host batches ----------------------
    def host_array(self, shape, dtype=np.uint8) -> np.ndarray:
        """A numpy array over pinned host memory (fi_host_alloc): sources and
        outputs there are copied by DMA directly, overlapping earlier batches.
        Freed with the context (or ``host_free``)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = self._lib.fi_host_alloc(self.h, max(nbytes, 1))
        if not ptr:
            raise MemoryError(L.lib().fi_last_error().decode())
        buf = (ctypes.c_uint8 * max(nbytes, 1)).from_address(ptr)
        arr = np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[ptr] = arr
        return arr

    def host_free(self, arr: np.ndarray):
        ptr = arr.ctypes.data
        if ptr in getattr(self, "_pinned", {}):
            del self._pinned[ptr]
            L.check(self._lib.fi_host_free(self.h, ptr))

    def submit(self, images: list[np.ndarray], ops: list[Op], outs: list[np.ndarray] | None = None):
        """fi_submit_batch: queue a batch of host images; returns (FiImage array,
        output buffers) whose contents are final after ``wait()``.  Buffers from
        ``host_array`` go by DMA directly; others through the library's pinned
        staging.  ``images`` / ``outs`` must stay alive until then."""
        n = len(images)
        arr = (L.FiImage * n)()
        for i, (src, op) in enumerate(zip(images, ops)):
            img = arr[i]
            img.src = src.ctypes.data
            img.src_h, img.src_w = src.shape[:2]
            img.src_stride = src.strides[0]
            img.src_channels = src.shape[2] if src.ndim == 3 else 1
            _fill(img, op)
        L.lib().fi_plan(arr, n)
        if outs is None:
            outs = [np.zeros(max(arr[i].out_w * arr[i].out_h * max(arr[i].out_channels, 1), 1), np.uint8)
                    for i in range(n)]
        for i in range(n):
            arr[i].dst = outs[i].ctypes.data
            arr[i].dst_capacity = outs[i].nbytes
        L.check(self._lib.fi_submit_batch(self.h, arr, n))
        return arr, outs

    @staticmethod
    def views(arr, outs):
        """Per image: the HWC (or HW) output view of a finished batch, or None."""
        res = []
        for i in range(len(outs)):
            a = arr[i]
            if a.status != L.FI_OK:
                res.append(None)
                continue
            o = outs[i].reshape(-1)[: a.out_h * a.out_stride].reshape(a.out_h, a.out_w, a.out_channels)
            res.append(o[:, :, 0] if a.out_channels == 1 else o)
        return res

    # ---- smartcrop (smartcrop.py SmartCrop().crop) ---------------------------
    def smartcrop_ex(self, rgb: np.ndarray, width: int, height: int, params=None, options=None,
                     want_images: bool = False):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w = rgb.shape[:2]
        step, nsc = 8, 2
        if options is not None:  # crops() positions per scale x scales
            step = max(int(options.step), 1)
            nsc = int((options.max_scale - options.min_scale) / max(options.scale_step, 1e-9) + 1.5) + 1
        cap = nsc * ((w + step - 1) // step + 1) * ((h + step - 1) // step + 1) + 16
        crops = (L.FiCropScore * cap)()
        n, top = ctypes.c_int32(), ctypes.c_int32()
        awh = (ctypes.c_int32 * 2)()
        pre = ctypes.c_double()
        ocap = w * h * 3
        pbuf = np.zeros(ocap, np.uint8) if want_images else None
        mbuf = np.zeros(ocap, np.uint8) if want_images else None
        rc = self._lib.fi_smartcrop_ex(
            self.h, rgb.ctypes.data, w, h, rgb.strides[0], width, height,
            ctypes.byref(params) if params is not None else None,
            ctypes.byref(options) if options is not None else None,
            crops, cap, ctypes.byref(n), ctypes.byref(top), awh, ctypes.byref(pre),
            pbuf.ctypes.data if want_images else None, mbuf.ctypes.data if want_images else None, ocap)
        L.check(rc)
        out = {"n": n.value, "top_index": top.value, "analyse_size": (awh[0], awh[1]),
               "prescale": pre.value, "crops": [crops[k] for k in range(n.value)]}
        if want_images:
            na = awh[0] * awh[1] * 3
            out["prescaled"] = pbuf[:na].reshape(awh[1], awh[0], 3)
            out["maps"] = mbuf[:na].reshape(awh[1], awh[0], 3)
        return out

    # ---- device memory -------------------------------------------------------
    def malloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        L.check(self._lib.fi_device_malloc(self.h, ctypes.byref(p), nbytes))
        return p.value

    def free(self, ptr: int):
        L.check(self._lib.fi_device_free(self.h, ptr))

    def h2d(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        L.check(self._lib.fi_memcpy_h2d(self.h, dptr, arr.ctypes.data, arr.nbytes))

    def d2h(self, dptr: int, nbytes: int) -> np.ndarray:
        out = np.empty(nbytes, np.uint8)
        L.check(self._lib.fi_memcpy_d2h(self.h, out.ctypes.data, dptr, nbytes))
        return out

    def jpeg_decode(self, blobs: list[bytes], dptrs: list[int], strides: list[int], channels: int = 0,
                    progressive: bool = False, views=None) -> list[int]:
        """fi_jpeg_decode_device: decodes baseline JPEG byte strings (with
        ``progressive=True``, fi_jpeg_decode_device_ex: progressive ones too) into the
        device buffers ``dptrs`` (HWC rows of ``strides`` bytes; channels as
        jpeg_info says, or 3 for every image with ``channels=3``: gray
        replicated); returns the per-image status (0 = decoded,
        FI_EUNSUPPORTED = decode that one on the host).  ``views``
        (fi_jpeg_decode_device_view): per image None or (orientation, x, y, w,
        h) -- the EXIF orientation to apply (0: the file's) and a rectangle of
        the oriented image (all 0: the whole); that buffer receives h rows of w
        pixels."""
        n = len(blobs)
        bufs = [ctypes.c_char_p(b) for b in blobs]  # the bytes objects' own storage, no copy
        data = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p).value for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in blobs])
        dst = (ctypes.c_void_p * n)(*dptrs)
        st = (ctypes.c_int64 * n)(*strides)
        status = (ctypes.c_int32 * n)()
        flags = L.FI_JPEG_PROGRESSIVE if progressive else 0
        if views is not None and any(v is not None for v in views):
            va = (L.FiJpegView * n)(*[L.FiJpegView(*(v if v is not None else (1, 0, 0, 0, 0))) for v in views])
            rc = self._lib.fi_jpeg_decode_device_view(self.h, data, lens, n, dst, st, channels, flags, va, status)
        elif progressive:
            rc = self._lib.fi_jpeg_decode_device_ex(self.h, data, lens, n, dst, st, channels, flags, status)
        else:
            rc = self._lib.fi_jpeg_decode_device(self.h, data, lens, n, dst, st, channels, status)
        if rc not in (L.FI_OK, L.FI_EUNSUPPORTED, L.FI_EINVAL):
            L.check(rc)
        return list(status)

    def jpeg_decode_host(self, blobs: list[bytes], progressive: bool = False, views=None) -> list[np.ndarray | None]:
        """jpeg_decode into scratch device buffers, copied back (tests / tools):
        HWC uint8 arrays (H, W, 3) or (H, W) for gray; None where the GPU
        decoder returned a non-zero status.  With ``views`` each buffer has its
        view's size (orientation 0: the file's, read with jpeg_orientation)."""
        infos = [jpeg_info(b, progressive) for b in blobs]
        if views is not None:
            dims = []
            for b, i, v in zip(blobs, infos, views):
                if i and v is not None and v[0] == 0:
                    o = jpeg_orientation(b)
                    v = (o,) + tuple(v[1:]) if o else None
                    i = i if o else None
                dims.append(jpeg_view_dims(i[0], i[1], v) + (i[2],) if i else None)
            infos = dims
        sizes = [(i[0] * i[1] * i[2]) if i else 1 for i in infos]
        with self._scratch(sizes) as ptrs:
            status = self.jpeg_decode(blobs, ptrs, [(i[0] * i[2]) if i else 1 for i in infos], progressive=progressive,
                                      views=views)
            out = []
            for info, p, sz, s in zip(infos, ptrs, sizes, status):
                if s != 0 or not info:
                    out.append(None)
                    continue
                w, h, c = info
                a = self.d2h(p, sz)
                out.append(a.reshape(h, w, 3) if c == 3 else a.reshape(h, w))
            return out

    def png_decode(self, blobs: list[bytes], dptrs: list[int], strides: list[int], out_channels=None) -> list[int]:
        """fi_png_decode_device: decodes PNG byte strings into the device
        buffers ``dptrs`` (HWC rows of ``strides`` bytes).  ``out_channels``:
        None or 0 = the natural count png_info reports, 3 = RGB (FI_EINVAL for
        a source with alpha), 4 = RGBA; one value or a list.  Returns the
        per-image status (0 = decoded, FI_EUNSUPPORTED = decode that one on the
        host, FI_EINVAL = malformed, or channels / stride that do not fit)."""
        n = len(blobs)
        if not n:
            return []
        bufs = [ctypes.c_char_p(b) for b in blobs]  # the bytes objects' own storage, no copy
        data = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p).value for b in bufs])
        lens = (ctypes.c_size_t * n)(*[len(b) for b in blobs])
        dst = (ctypes.c_void_p * n)(*dptrs)
        st = (ctypes.c_int64 * n)(*strides)
        status = (ctypes.c_int32 * n)()
        oc = None
        if out_channels is not None:
            oc = (ctypes.c_int32 * n)(*(out_channels if isinstance(out_channels, (list, tuple)) else [out_channels] * n))
        rc = self._lib.fi_png_decode_device(self.h, data, lens, n, dst, st, oc, status)
        if rc not in (L.FI_OK, L.FI_EUNSUPPORTED, L.FI_EINVAL):
            L.check(rc)
        return list(status)

    def png_decode_host(self, blobs: list[bytes], out_channels=None) -> list[np.ndarray | None]:
        """png_decode into scratch device buffers, copied back (tests / tools):
        HWC uint8 arrays (H, W, C), (H, W) for one channel; None where the GPU
        decoder returned a non-zero status."""
        n = len(blobs)
        ocs = list(out_channels) if isinstance(out_channels, (list, tuple)) else [out_channels or 0] * n
        infos = [png_info(b) for b in blobs]
        dims = [(i[0], i[1], oc or i[2]) if i else None for i, oc in zip(infos, ocs)]
        with self._scratch([d[0] * d[1] * d[2] if d else 1 for d in dims]) as ptrs:
            status = self.png_decode(blobs, ptrs, [d[0] * d[2] if d else 1 for d in dims], ocs)
            out = []
            for d, p, s in zip(dims, ptrs, status):
                if s != 0 or not d:
                    out.append(None)
                    continue
                w, h, c = d
                a = self.d2h(p, w * h * c)
                out.append(a.reshape(h, w) if c == 1 else a.reshape(h, w, c))
            return out

    # ---- what the codec wrappers share ----------------------------------------
    @contextlib.contextmanager
    def _scratch(self, sizes):
        """Device buffers of ``sizes`` bytes (at least 1), freed on the way out."""
        ptrs = [self.malloc(max(sz, 1)) for sz in sizes]
        try:
            yield ptrs
        finally:
            for p in ptrs:
                self.free(p)

    @contextlib.contextmanager
    def _uploaded(self, images):
        """Host arrays (HW, HWC) in scratch device buffers, as (device pointer,
        w, h, stride, channels) views."""
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        with self._scratch([a.nbytes for a in arrs]) as ptrs:
            views = []
            for a, p in zip(arrs, ptrs):
                self.h2d(p, a)
                c = a.shape[2] if a.ndim == 3 else 1
                views.append((p, a.shape[1], a.shape[0], a.shape[1] * c, c))
            yield views

    @staticmethod
    def _per_image(value, n):
        return list(value) if isinstance(value, (list, tuple)) else [value] * n

    def _encode_call(self, fn, views, extras, ptrs, caps, *tail):
        """fn = a fi_*_encode_device: the argument block they share, with the
        codec's per-image int32 arrays ``extras`` (None: the NULL pointer)
        behind the strides and ``tail`` behind the status."""
        n = len(views)
        I32, I64, SZ, VP = ctypes.c_int32 * n, ctypes.c_int64 * n, ctypes.c_size_t * n, ctypes.c_void_p * n
        out_len, status = SZ(), I32()
        rc = fn(self.h, VP(*[v[0] for v in views]), I32(*[v[1] for v in views]), I32(*[v[2] for v in views]),
                I32(*[v[4] for v in views]), I64(*[v[3] for v in views]),
                *[I32(*e) if e is not None else None for e in extras], n, VP(*ptrs), SZ(*caps), out_len, status, *tail)
        return rc, list(status), list(out_len)

    @staticmethod
    def _encode_guarded(call, caps):
        """call(ptrs, caps) into fresh buffers of caps[i] + 64 bytes whose last
        128 are 0xA5: (rc, status list, length list, buffer list)."""
        offs = np.concatenate([[0], np.cumsum([c + 64 for c in caps])]).astype(np.int64)
        pool = np.empty(int(offs[-1]), np.uint8)
        bufs = [pool[int(offs[i]):int(offs[i + 1])] for i in range(len(caps))]
        for b, c in zip(bufs, caps):
            b[max(0, c - 64):] = 0xA5
        rc, status, lens = call([b.ctypes.data for b in bufs], caps)
        return rc, status, lens, bufs

    def _encode_pooled(self, call, caps, short_is_status=False):
        """call(ptrs, caps) into the output pool all the encoders keep: (status
        list, length list, files -- None where the status is not 0).  A
        failure of the call, not of an image, raises (``short_is_status``:
        FI_ENOMEM that an image reports is the image's)."""
        offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        pool = getattr(self, "_enc_out", None)
        if pool is None or pool.size < int(offs[-1]):  # kept: fresh pages are the cost of a large buffer
            pool = self._enc_out = np.empty(int(offs[-1]) + int(offs[-1]) // 4, np.uint8)
        base = pool.ctypes.data
        rc, status, lens = call([base + int(o) for o in offs[:-1]], caps)
        if rc not in (L.FI_OK, L.FI_EUNSUPPORTED, L.FI_EINVAL) and not (
                short_is_status and rc == L.FI_ENOMEM and rc in status):
            L.check(rc)
        files = [pool[int(offs[i]):int(offs[i]) + lens[i]].tobytes() if status[i] == L.FI_OK else None
                 for i in range(len(caps))]
        return status, lens, files

    def _jpeg_encode_call(self, views, qs, ss, ptrs, caps, progressive=False):
        if progressive:
            return self._encode_call(self._lib.fi_jpeg_encode_device_ex, views, [qs, ss], ptrs, caps,
                                     L.FI_JPEG_ENC_PROGRESSIVE)
        return self._encode_call(self._lib.fi_jpeg_encode_device, views, [qs, ss], ptrs, caps)

    def _jpeg_bound(self, view, q, s, progressive=False):
        b = ctypes.c_size_t()
        rc = self._lib.fi_jpeg_encode_bound_ex(view[1], view[2], view[4], q, s,
                                               L.FI_JPEG_ENC_PROGRESSIVE if progressive else 0, ctypes.byref(b))
        return b.value if rc == L.FI_OK else 1

    def jpeg_encode_raw(self, views, quality, subsampling, caps=None, progressive=False):
        """fi_jpeg_encode_device on (device pointer, w, h, stride, channels)
        views; ``quality`` / ``subsampling`` per image or one value for all;
        ``caps``: output capacities (default: fi_jpeg_encode_bound, 1 where the
        bound turns the image down).  Returns (rc, status list, length list,
        output buffer list): buffer i is a uint8 array of caps[i] + 64 bytes
        whose last 128 are set to 0xA5 beforehand, so a caller can see what
        was written behind the file and behind the capacity.
        ``progressive``: fi_jpeg_encode_device_ex with FI_JPEG_ENC_PROGRESSIVE
        and its bound."""
        n = len(views)
        qs, ss = self._per_image(quality, n), self._per_image(subsampling, n)
        if caps is None:
            caps = [self._jpeg_bound(v, q, s, progressive) for v, q, s in zip(views, qs, ss)]
        return self._encode_guarded(lambda ptrs, caps: self._jpeg_encode_call(views, qs, ss, ptrs, caps, progressive),
                                    caps)

    def jpeg_encode(self, views, quality, subsampling, progressive=False) -> list[bytes | None]:
        """fi_jpeg_encode_device: baseline JPEG files of device-resident images
        given as (device pointer, w, h, stride, channels) views -- byte for
        byte what Pillow writes with quality / subsampling (0 = 4:4:4, 2 =
        4:2:0; per image or one value) and restart_marker_rows=1.  None where
        the encoder turned the image down (alpha channels, other samplings,
        bad quality).  The output buffers are sized to the pixels (the worst
        case of fi_jpeg_encode_bound is many times a real file); the rare file
        larger than its pixels -- noise at the top qualities -- is encoded
        again into a buffer of the size the first call reported.
        ``progressive``: progressive files with per-scan optimal Huffman
        tables instead (FI_JPEG_ENC_PROGRESSIVE) -- byte for byte what Pillow
        writes with progressive=True added."""
        n = len(views)
        if not n:
            return []
        qs, ss = self._per_image(quality, n), self._per_image(subsampling, n)
        caps = [min(self._jpeg_bound(v, q, s, progressive), v[1] * v[2] * v[4] + 1024)
                for v, q, s in zip(views, qs, ss)]
        status, lens, files = self._encode_pooled(
            lambda ptrs, caps: self._jpeg_encode_call(views, qs, ss, ptrs, caps, progressive), caps, short_is_status=True)
        again = [i for i in range(n) if status[i] == L.FI_ENOMEM and lens[i] > caps[i]]
        if again:
            big = [np.empty(lens[i], np.uint8) for i in again]
            rc, st2, len2 = self._jpeg_encode_call([views[i] for i in again], [qs[i] for i in again],
                                                   [ss[i] for i in again], [b.ctypes.data for b in big],
                                                   [lens[i] for i in again], progressive)
            L.check(rc)
            for k, i in enumerate(again):
                files[i] = big[k][:len2[k]].tobytes()
        return files

    def jpeg_encode_host(self, images: list[np.ndarray], quality, subsampling, progressive=False) -> list[bytes | None]:
        """jpeg_encode of host arrays (HW, HWC with 1..4 channels), uploaded to
        scratch device buffers first (tests / tools): the counterpart of
        jpeg_decode_host."""
        with self._uploaded(images) as views:
            return self.jpeg_encode(views, quality, subsampling, progressive)

    def _png_encode_call(self, views, fs, ptrs, caps):
        return self._encode_call(self._lib.fi_png_encode_device, views, [fs], ptrs, caps)

    def _png_bound(self, view):
        b = ctypes.c_size_t()
        return b.value if self._lib.fi_png_encode_bound(view[1], view[2], view[4], ctypes.byref(b)) == L.FI_OK else 1

    def png_encode_raw(self, views, filter=-1, caps=None):
        """fi_png_encode_device on (device pointer, w, h, stride, channels)
        views; ``filter`` per image, one value for all, or None (the NULL
        pointer: adaptive); ``caps``: output capacities (default:
        fi_png_encode_bound, 1 where the bound turns the image down).  Returns
        (rc, status list, length list, output buffer list) with the 0xA5
        guards of jpeg_encode_raw."""
        fs = None if filter is None else self._per_image(filter, len(views))
        if caps is None:
            caps = [self._png_bound(v) for v in views]
        return self._encode_guarded(lambda ptrs, caps: self._png_encode_call(views, fs, ptrs, caps), caps)

    def png_encode(self, views, filter=-1) -> list[bytes | None]:
        """fi_png_encode_device: PNG files of device-resident images given as
        (device pointer, w, h, stride, channels) views, 1..4 channels; any
        PNG decoder returns the pixels bit for bit.  ``filter``: -1 adaptive,
        0..4 fixed (per image or one value).  None where the encoder turned the
        image down.  The output buffers are sized to fi_png_encode_bound (a
        few hundred bytes above the pixels), so one call always suffices."""
        if not len(views):
            return []
        fs = self._per_image(filter, len(views))
        return self._encode_pooled(lambda ptrs, caps: self._png_encode_call(views, fs, ptrs, caps),
                                   [self._png_bound(v) for v in views])[2]

    def png_encode_host(self, images: list[np.ndarray], filter=-1) -> list[bytes | None]:
        """png_encode of host arrays (HW, HWC with 1..4 channels), uploaded to
        scratch device buffers first (tests / tools)."""
        with self._uploaded(images) as views:
            return self.png_encode(views, filter)

    def _webp_encode_call(self, views, ps, ptrs, caps):
        return self._encode_call(self._lib.fi_webp_encode_device, views, [ps], ptrs, caps)

    def _webp_bound(self, view):
        b = ctypes.c_size_t()
        return b.value if self._lib.fi_webp_encode_bound(view[1], view[2], view[4], ctypes.byref(b)) == L.FI_OK else 1

    def webp_encode_raw(self, views, predictor=-1, caps=None):
        """fi_webp_encode_device on (device pointer, w, h, stride, channels)
        views; ``predictor`` per image, one value for all, or None (the NULL
        pointer: adaptive); ``caps``: output capacities (default:
        fi_webp_encode_bound, 1 where the bound turns the image down).
        Returns (rc, status list, length list, output buffer list) with the
        0xA5 guards of jpeg_encode_raw."""
        ps = None if predictor is None else self._per_image(predictor, len(views))
        if caps is None:
            caps = [self._webp_bound(v) for v in views]
        return self._encode_guarded(lambda ptrs, caps: self._webp_encode_call(views, ps, ptrs, caps), caps)

    def webp_encode(self, views, predictor=-1) -> list[bytes | None]:
        """fi_webp_encode_device: lossless WebP files of device-resident
        images given as (device pointer, w, h, stride, channels) views, 1..4
        channels; any WebP decoder returns the pixels bit for bit.
        ``predictor``: -1 adaptive, 0..13 fixed (per image or one value).  None
        where the encoder turned the image down.  The output buffers are sized
        to fi_webp_encode_bound (below 1 KiB above the pixels), so one call
        always suffices."""
        if not len(views):
            return []
        ps = self._per_image(predictor, len(views))
        return self._encode_pooled(lambda ptrs, caps: self._webp_encode_call(views, ps, ptrs, caps),
                                   [self._webp_bound(v) for v in views])[2]

    def webp_encode_host(self, images: list[np.ndarray], predictor=-1) -> list[bytes | None]:
        """webp_encode of host arrays (HW, HWC with 1..4 channels), uploaded to
        scratch device buffers first (tests / tools)."""
        with self._uploaded(images) as views:
            return self.webp_encode(views, predictor)

    def process_device_resident(self, views, ops: list[Op]):
        """fi_process_batch_device on device-resident sources given as (device
        pointer, width, height, stride) views of RGB8 pixels (e.g. fi_jpeg_decode_device
        targets, extract offsets applied) or (device pointer, width, height,
        stride, channels) views (3, or 4: RGBA, e.g. fi_png_decode_device
        targets), the outputs left on the device (for
        jpeg_encode): (base, out_views, fi_image records, rc); out_views[i] is
        the (device pointer, w, h, stride, channels) view of output i or None,
        inside the allocation ``base``, which the caller frees."""
        n = len(views)
        arr = (L.FiImage * max(n, 1))()
        for i, (v, op) in enumerate(zip(views, ops)):
            a = arr[i]
            p, w, h, st = v[:4]
            a.src, a.src_w, a.src_h, a.src_stride, a.src_channels = p, w, h, st, v[4] if len(v) > 4 else 3
            _fill(a, op)
        L.lib().fi_plan(arr, n)
        caps = [max(arr[i].out_w * arr[i].out_h * max(arr[i].out_channels, 1), 1) for i in range(n)]
        offs = np.concatenate([[0], np.cumsum([(c + 255) // 256 * 256 for c in caps])]).astype(np.int64)
        base = self.malloc(int(offs[-1]) if n else 256)
        try:
            for i in range(n):
                arr[i].dst, arr[i].dst_capacity = base + int(offs[i]), caps[i]
            rc = self._lib.fi_process_batch_device(self.h, arr, n)
        except BaseException:
            self.free(base)
            raise
        out_views = [(base + int(offs[i]), arr[i].out_w, arr[i].out_h, arr[i].out_stride, arr[i].out_channels)
                     if arr[i].status == L.FI_OK else None for i in range(n)]
        return base, out_views, [arr[i] for i in range(n)], rc

    def process_device_views(self, views, ops: list[Op]):
        """process_device_resident with the outputs copied back as host
        arrays: (outputs, fi_image records, rc) like ``process``."""
        base, out_views, recs, rc = self.process_device_resident(views, ops)
        try:
            results = []
            for v in out_views:
                if v is None:
                    results.append(None)
                    continue
                p, w, h, st, c = v
                o = self.d2h(p, h * st).reshape(h, st)[:, : w * c].reshape(h, w, c)
                results.append(o[:, :, 0] if c == 1 else o)
        finally:
            self.free(base)
        return results, recs, rc

    def fill_synthetic(self, dptr: int, w: int, h: int, stride: int, seed: int):
        L.check(self._lib.fi_fill_synthetic(self.h, dptr, w, h, stride, seed & 0xFFFFFFFF))

    def process_device(self, arr, n: int) -> int:
        """fi_process_batch_device on a prepared FiImage array (device pointers)."""
        return self._lib.fi_process_batch_device(self.h, arr, n)

    def submit_device(self, arr, n: int) -> int:
        """fi_submit_batch_device: plan + upload + launch, returns before the GPU
        finishes; ``arr`` must stay alive until ``wait()``."""
        return self._lib.fi_submit_batch_device(self.h, arr, n)

    def wait(self, keep: int = 0) -> int:
        """fi_wait: finalize submitted batches (oldest first) until at most
        ``keep`` remain in flight, filling their records."""
        return self._lib.fi_wait(self.h, keep)

    def query(self) -> int:
        """fi_query: how many submitted batches are still running on the GPU
        (does not block)."""
        n = ctypes.c_int32()
        L.check(self._lib.fi_query(self.h, ctypes.byref(n)))
        return n.value

    # ---- timing ----------------------------------------------------------------
    def set_timing(self, on):
        """True / 1: every stage timed; 2: the resample stage only; False / 0: off."""
        L.check(self._lib.fi_set_timing(self.h, int(on)))

    def reset_stats(self):
        L.check(self._lib.fi_reset_stats(self.h))

    def stats(self, name: str):
        ms, n, b = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        L.check(self._lib.fi_kernel_stats(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(b)))
        return ms.value, n.value, b.value

    def monochrome_q16(self, gray: np.ndarray, rot: int = 0) -> np.ndarray:
        """Test hook: the -monochrome kernels on a Q16 gray image (fi_debug_monochrome)."""
        g = np.ascontiguousarray(gray, dtype=np.uint16)
        h, w = g.shape
        oh, ow = (w, h) if rot in (90, 270) else (h, w)
        out = np.zeros((oh, ow), np.uint8)
        L.check(self._lib.fi_debug_monochrome(self.h, g.ctypes.data, w, h, rot, out.ctypes.data, ow))
        return out

    def rotate_q16(self, q16: np.ndarray, degrees: int, background: int = 0xFFFFFF):
        """Test hook: the rotation stage on a Q16 HWC (or HW gray) image
        (fi_debug_rotate): ``-background`` 0x00RRGGBB, ``-rotate degrees``.
        Returns (Q16 result, its 8-bit form)."""
        q = np.ascontiguousarray(q16, dtype=np.uint16)
        h, w = q.shape[:2]
        ch = q.shape[2] if q.ndim == 3 else 1
        size = rotated_size(w, h, degrees)
        if size is None:
            raise L.FiError(L.FI_EUNSUPPORTED, "-rotate: shear leaves IM's canvas")
        ow, oh = size
        shape = (oh, ow, ch) if q.ndim == 3 else (oh, ow)
        o16, o8 = np.zeros(shape, np.uint16), np.zeros(shape, np.uint8)
        rw, rh = ctypes.c_int32(), ctypes.c_int32()
        L.check(self._lib.fi_debug_rotate(self.h, q.ctypes.data, w, h, ch, degrees, background & 0xFFFFFF,
                                          o16.ctypes.data, o8.ctypes.data, ctypes.byref(rw), ctypes.byref(rh)))
        assert (rw.value, rh.value) == (ow, oh)
        return o16, o8

    def convolve_q16(self, q16: np.ndarray, conv, ops: int) -> np.ndarray:
        """Test hook: the forwarded convolution kernels on a Q16 HWC image
        (fi_debug_convolve); conv = unsharp[4] + sharpen[2] + blur[2]."""
        q = np.ascontiguousarray(q16, dtype=np.uint16)
        h, w = q.shape[:2]
        ch = q.shape[2] if q.ndim == 3 else 1
        cv = (ctypes.c_double * 8)(*conv)
        out = np.zeros(q.shape, np.uint8)
        L.check(self._lib.fi_debug_convolve(self.h, q.ctypes.data, w, h, ch, cv, ops, out.ctypes.data))
        return out


def rotated_size(w: int, h: int, degrees: int):
    """fi_debug_rotate's planner half (no GPU): (out_w, out_h) of a w x h image
    after ``-rotate degrees``, or None where a shear would leave IM's canvas
    (FI_EUNSUPPORTED: tall, narrow images)."""
    ow, oh = ctypes.c_int32(), ctypes.c_int32()
    rc = L.lib().fi_debug_rotate(None, None, w, h, 3, degrees, 0xFFFFFF, None, None, ctypes.byref(ow),
                                 ctypes.byref(oh))
    if rc == L.FI_EUNSUPPORTED:
        return None
    L.check(rc)
    return ow.value, oh.value


def rotate_q16_host(q16: np.ndarray, degrees: int, background: int = 0xFFFFFF):
    """fi_debug_rotate_host (test hook, no GPU): the rotation kernel's
    per-pixel procedure run on the CPU -- what ``Context.rotate_q16`` returns."""
    q = np.ascontiguousarray(q16, dtype=np.uint16)
    h, w = q.shape[:2]
    ch = q.shape[2] if q.ndim == 3 else 1
    size = rotated_size(w, h, degrees)
    if size is None:
        raise L.FiError(L.FI_EUNSUPPORTED, "-rotate: shear leaves IM's canvas")
    ow, oh = size
    shape = (oh, ow, ch) if q.ndim == 3 else (oh, ow)
    o16, o8 = np.zeros(shape, np.uint16), np.zeros(shape, np.uint8)
    rw, rh = ctypes.c_int32(), ctypes.c_int32()
    L.check(L.lib().fi_debug_rotate_host(q.ctypes.data, w, h, ch, degrees, background & 0xFFFFFF, o16.ctypes.data,
                                         o8.ctypes.data, ctypes.byref(rw), ctypes.byref(rh)))
    return o16, o8


def device_count() -> int:
    n = ctypes.c_int32()
    L.check(L.lib().fi_device_count(ctypes.byref(n)))
    return n.value
