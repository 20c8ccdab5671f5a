"""Host codec pipeline around the GPU path:
ImageHandler::processNewImage end to end for a batch of encoded images.

  decode   Pillow (libjpeg-turbo / libpng) on a thread pool -- the decoders
           release the GIL -- with ``-auto-orient`` (ImageProcessor.php:78)
           applied from the EXIF orientation, then ExtractProcessor's view;
  process  ONE fi_process_batch for the whole batch (ImageProcessor +
           SmartCropProcessor on the MI355X);
  encode   on the thread pool: JPEG at ``q_`` (default 90) -- flyimg pipes
           TGA into MozJPEG's cjpeg when it is executable and otherwise lets
           ImageMagick write the JPEG with ``-quality`` (calculateQuality,
           ImageProcessor.php:195-217); neither ``cjpeg`` nor ``convert`` is
           in this image, so the encoder is libjpeg-turbo at the same quality
           (IM's own JPEG coder is libjpeg as well).  Images with alpha are
           written as PNG.  With ``gpu_encode`` the JPEGs are written on the
           MI355X instead (fi_jpeg_encode_device): the outputs stay in device
           memory and leave it compressed -- the same baseline coding with
           one restart interval per MCU row, byte for byte what
           libjpeg-turbo writes with ``restart_marker_rows=1``.  With
           ``gpu_png`` on top the alpha outputs are written there as well
           (fi_png_encode_device): PNG files of the same pixels, deflated
           per 32 KiB band on the device.  With ``gpu_webp`` on top the
           ``o_webp,webpl_1`` outputs leave as lossless WebP
           (fi_webp_encode_device); otherwise the option is ignored.

Gray (L), bilevel and palette sources are expanded to RGB / RGBA before the
GPU (IM would keep a gray JPEG gray: the channels are equal either way), and
flagged FI_SRC_PSEUDOCLASS: IM's readers give them a colormap (1-component
JPEG, palette / 8-bit gray PNG, GIF), so ResizeImage filters them with
Mitchell instead of Lanczos (resize.c).
"""
from __future__ import annotations

import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib as L
from .processor import ExecFailedException, ExtractProcessor, ImageProcessor, OptionsBag, _empty


# Pillow modes whose IM reading is a PseudoClass image: bilevel, 8-bit gray and
# palette (16-bit gray "I;16" / "I" stays DirectClass, depth > 8)
PSEUDOCLASS_MODES = ("1", "L", "P")


def decode_ex(blob: bytes):
    """Encoded bytes -> (HWC uint8 RGB, or RGBA when the file has alpha, EXIF
    orientation applied (-auto-orient); True when IM would read a PseudoClass
    image)."""
    from PIL import Image, ImageOps

    im = Image.open(io.BytesIO(blob))
    im = ImageOps.exif_transpose(im)
    pseudo = im.mode in PSEUDOCLASS_MODES
    alpha = im.mode in ("RGBA", "LA", "PA") or (im.mode == "P" and "transparency" in im.info)
    im = im.convert("RGBA" if alpha else "RGB")
    return np.asarray(im), pseudo


def decode(blob: bytes) -> np.ndarray:
    """decode_ex without the class flag."""
    return decode_ex(blob)[0]


def encode(pixels: np.ndarray, quality: int = 90) -> bytes:
    from PIL import Image

    buf = io.BytesIO()
    ch = pixels.shape[2] if pixels.ndim == 3 else 1
    if ch in (2, 4):  # alpha survives: PNG
        Image.fromarray(pixels, "LA" if ch == 2 else "RGBA").save(buf, "PNG")
    else:
        # IM 6 coders/jpeg.c: without -sampling-factor, quality >= 90 writes 1x1
        # (4:4:4) chroma and lower qualities 2x2 (4:2:0).  (MozJPEG's cjpeg, the
        # reference's path when it is installed, always uses 2x2.)
        Image.fromarray(pixels, "L" if ch == 1 else "RGB").save(
            buf, "JPEG", quality=int(quality), subsampling=0 if int(quality) >= 90 else 2)
    return buf.getvalue()


class _PinnedSlot:
    """One in-flight batch's pinned host memory (fi_host_alloc): the decoded
    sources and the GPU outputs, sliced per image (256-B aligned), grown on
    demand.  Two slots: batch k+1 decodes into one while batch k's DMA and
    kernels use the other."""

    def __init__(self, ctx):
        self.ctx, self.src, self.dst = ctx, None, None

    def _grow(self, which, nbytes):
        cur = getattr(self, which)
        if cur is None or cur.nbytes < nbytes:
            if cur is not None:
                self.ctx.host_free(cur)
            setattr(self, which, self.ctx.host_array((max(nbytes, 1 << 20),)))
        return getattr(self, which)

    @staticmethod
    def _slices(buf, sizes):
        out, off = [], 0
        for n in sizes:
            out.append(buf[off:off + n])
            off += (n + 255) // 256 * 256
        return out

    def sources(self, shapes):
        sizes = [int(np.prod(s)) for s in shapes]
        buf = self._grow("src", sum((n + 255) // 256 * 256 for n in sizes))
        return [v.reshape(s) for v, s in zip(self._slices(buf, sizes), shapes)]

    def outputs(self, sizes):
        buf = self._grow("dst", sum((n + 255) // 256 * 256 for n in sizes))
        return self._slices(buf, sizes)


def gpu_decodable(blob: bytes, progressive: bool = False, orient: bool = False):
    """(width, height, source channels) when the GPU decoder
    (fi_jpeg_decode_device, RGB output) produces exactly what decode_ex would:
    a baseline gray or YCbCr JPEG (fi_jpeg_info) with no EXIF rotation to
    apply; None otherwise (progressive, CMYK, PNG, ...).  A gray (1-component)
    JPEG is an IM PseudoClass source, as decode_ex flags it.  With
    ``progressive`` complete Huffman progressive JPEGs qualify as well
    (fi_jpeg_info_ex / fi_jpeg_decode_device_ex, FI_JPEG_PROGRESSIVE).  With
    ``orient`` EXIF-rotated files qualify too, for a decode through a view
    (fi_jpeg_decode_device_view, orientation 0): the ORIENTED (width, height,
    channels) of every file whose orientation the library determines
    (fi_jpeg_orientation), None for the others."""
    from .runtime import jpeg_info, jpeg_orientation, jpeg_view_dims

    info = jpeg_info(blob, progressive)
    if not info:
        return None
    if orient:
        o = jpeg_orientation(blob)
        return jpeg_view_dims(info[0], info[1], (o, 0, 0, 0, 0)) + (info[2],) if o else None
    from PIL import Image

    try:
        orientation = Image.open(io.BytesIO(blob)).getexif().get(0x0112, 1)  # headers only
    except Exception:  # noqa: BLE001 - unreadable EXIF: let the host path decide
        return None
    return info if orientation in (0, 1) else None


def png_gpu_decodable(blob: bytes, bag):
    """(width, height, natural channels, colour type) when the GPU PNG decoder
    (fi_png_decode_device) produces exactly what decode_ex and
    ExtractProcessor would: fi_png_info accepts the file, no chunk could carry
    an orientation (meta 0: exif_transpose has nothing to apply) and the
    request has no ``e_1`` extract; None otherwise (JPEGs among them)."""
    from .runtime import png_info

    if not _empty(bag.get("extract")):
        return None
    info = png_info(blob)
    if not info or info[4] != 0:
        return None
    return info[:4]


class CodecPipeline:
    """Batches of encoded images through decode -> GPU -> encode.  With
    ``gpu_decode`` (default) baseline gray / YCbCr JPEGs are decoded on the MI355X
    straight into device memory (bit-exact with the host decoder) and only
    the other sources take the host decoder.  With ``gpu_encode`` (off by
    default: the files carry restart markers, so their bytes differ from the
    host encoder's, the decoded pixels do not) ``process`` keeps the outputs
    on the device and writes every JPEG there with one fi_jpeg_encode_device
    call; outputs with alpha still go through the host PNG writer unless
    ``gpu_png`` (off by default, needs ``gpu_encode``) sends them through one
    fi_png_encode_device call per batch: other bytes than the host writer's
    file, the same decoded pixels.  With ``gpu_progressive_encode`` (off by
    default, needs ``gpu_encode``) the JPEGs are the file class flyimg ships:
    progressive, with Huffman tables fitted to every scan
    (FI_JPEG_ENC_PROGRESSIVE) -- smaller files, the same decoded pixels,
    more device time; DESIGN.md 3.6b.  With ``gpu_webp`` (off by default, needs
    ``gpu_encode``) the outputs whose options resolve to lossless WebP
    (``o_webp,webpl_1``), opaque or with alpha, are written by one
    fi_webp_encode_device call per batch (VP8L; any decoder returns the
    pixels); without it the option stays ignored.  With
    ``gpu_progressive`` (off by default) progressive JPEG sources join the GPU
    decode batch instead of the host threads (same pixels).  A progressive
    scan is one serial chain on the GPU: measured on 1080p sources the GPU
    path loses to 16 host threads below about 220 images per batch (172
    against 403 img/s at batches of 64) and wins above (1956 against 652
    img/s at 1024 images); DESIGN.md 3.5.  With ``gpu_orient`` (off by
    default) EXIF-rotated JPEGs and ``e_1`` extracts join the GPU decode batch
    as well: the decoder's colour stage applies ``-auto-orient`` and
    ExtractProcessor's rectangle (fi_jpeg_decode_device_view), so each device
    buffer holds the oriented, extracted source (same pixels as the host
    path's).  With ``gpu_png_decode`` (off by default) PNG sources -- 8-bit,
    non-interlaced, without orientation metadata or an extract -- are inflated
    and unfiltered on the MI355X as well (fi_png_decode_device) and, with
    ``gpu_encode`` and ``gpu_png``, an RGBA batch stays on the device from file
    to file.  An image's deflate stream is one serial chain on one wave (0.67 s
    for a 1000x750 RGBA file), so the batch supplies the parallelism: measured
    on such sources, device-resident, 80 against 553 img/s of the host-decode
    arm at batches of 64, 230 against 397 at 256, and 429 against 379 at 1024
    images, where the host arm's spread still reaches past it; DESIGN.md 3.8.  ``decode_stats`` counts the images ``process`` decoded
    on each side.  With ``shear_rotate`` (off by default) ``r_`` by any
    integer angle and ``bg_`` run on the GPU instead of being
    rejected."""

    def __init__(self, ctx, threads: int = 16, gpu_decode: bool = True, gpu_encode: bool = False,
                 gpu_progressive: bool = False, gpu_orient: bool = False, gpu_png: bool = False,
                 gpu_png_decode: bool = False, gpu_progressive_encode: bool = False, shear_rotate: bool = False,
                 gpu_webp: bool = False):
        if gpu_webp and not gpu_encode:
            raise ValueError("gpu_webp needs gpu_encode=True: the WebP outputs are written by the GPU encode stage")
        if gpu_progressive_encode and not gpu_encode:
            raise ValueError("gpu_progressive_encode needs gpu_encode=True: it selects the GPU encoder's file class")
        if gpu_png and not gpu_encode:
            raise ValueError("gpu_png needs gpu_encode=True: the PNG outputs are written by the GPU encode stage")
        self.ctx = ctx
        self.pool = ThreadPoolExecutor(max_workers=max(1, threads))
        self.gpu_decode = gpu_decode
        self.gpu_encode = gpu_encode
        self.gpu_progressive = gpu_progressive
        self.gpu_orient = gpu_orient
        self.gpu_png = gpu_png
        self.gpu_png_decode = gpu_png_decode
        self.gpu_webp = gpu_webp
        self.gpu_progressive_encode = gpu_progressive_encode
        self.shear_rotate = shear_rotate  # ImageProcessor's opt-in: r_ by any integer angle, bg_
        self.decode_stats = {"gpu": 0, "host": 0}  # images ``process`` decoded on the GPU / on the host
        # ``process``: host seconds in the encode stage, the bytes its outputs
        # were as pixels and are as files (with gpu_encode, what crosses PCIe)
        self.process_stats = {"s_encode": 0.0, "raw_bytes": 0, "encoded_bytes": 0}

    def close(self):
        self.pool.shutdown()

    @staticmethod
    def _quality(bag):
        q = bag.get_option("quality")
        return int(q) if not _empty(q) else 90

    def _host_batch(self, blobs, bags):
        decoded = list(self.pool.map(decode_ex, blobs))
        srcs, ops = [], []
        for (img, pseudo), bag in zip(decoded, bags):
            img = ExtractProcessor.extract(bag, img)
            h, w = img.shape[:2]
            op = ImageProcessor(bag, w, h, shear_rotate=self.shear_rotate).to_op()
            if pseudo:
                op.flags |= L.FI_SRC_PSEUDOCLASS
            ops.append(op)
            srcs.append(np.ascontiguousarray(img))
        outs, recs, _ = self.ctx.process(srcs, ops)
        return outs, list(recs)

    def _gpu_batch(self, blobs, bags, dims, held=None, views=None):
        """GPU decode into one device pool (16-B aligned rows for the streaming
        resample kernels), one device batch.  ``views`` (gpu_orient): the
        decode view of each image, ``dims`` then being what it decodes to.
        Returns (outputs, records, indices the GPU decoder turned down).  With
        ``held`` (a list) the outputs stay on the device: they come back as
        (device pointer, w, h, stride, channels) views and their allocation is
        appended to ``held`` for the caller to free."""
        # a PNG source's dims are (w, h, natural channels, colour type): alpha decodes to 4 channels
        png = [len(d) == 4 for d in dims]
        chans = [4 if p and d[2] in (2, 4) else 3 for p, d in zip(png, dims)]
        strides = [(d[0] * c + 15) // 16 * 16 for d, c in zip(dims, chans)]
        offs = np.concatenate([[0], np.cumsum([(s * d[1] + 255) // 256 * 256 for s, d in zip(strides, dims)])])
        base = self.ctx.malloc(int(offs[-1]))
        try:
            ptrs = [base + int(o) for o in offs[:-1]]
            status = [L.FI_OK] * len(blobs)
            ji = [i for i in range(len(blobs)) if not png[i]]
            pi = [i for i in range(len(blobs)) if png[i]]
            if ji:
                st_j = self.ctx.jpeg_decode([blobs[i] for i in ji], [ptrs[i] for i in ji], [strides[i] for i in ji],
                                            channels=3, progressive=self.gpu_progressive,
                                            views=[views[i] for i in ji] if views else None)
                for i, s in zip(ji, st_j):
                    status[i] = s
            if pi:
                st_p = self.ctx.png_decode([blobs[i] for i in pi], [ptrs[i] for i in pi], [strides[i] for i in pi],
                                           [chans[i] for i in pi])
                for i, s in zip(pi, st_p):
                    status[i] = s
            views, ops, keep = [], [], []
            for i, (bag, d, p, st) in enumerate(zip(bags, dims, ptrs, strides)):
                if status[i] != L.FI_OK:
                    continue
                w, h = d[0], d[1]
                views.append((p, w, h, st, chans[i]))
                op = ImageProcessor(bag, w, h, shear_rotate=self.shear_rotate).to_op()
                # 1-component JPEG, gray or palette PNG (Pillow's "L" / "P"): IM PseudoClass (Mitchell), as
                # decode_ex flags it
                if (d[3] in (0, 3)) if png[i] else (d[2] == 1):
                    op.flags |= L.FI_SRC_PSEUDOCLASS
                ops.append(op)
                keep.append(i)
            if held is None:
                outs, recs, _ = self.ctx.process_device_views(views, ops)
            else:
                obase, outs, recs, _ = self.ctx.process_device_resident(views, ops)
                held.append(obase)
        finally:
            self.ctx.free(base)
        full_o, full_r = [None] * len(blobs), [None] * len(blobs)
        for k, i in enumerate(keep):
            full_o[i], full_r[i] = outs[k], recs[k]
        return full_o, full_r, [i for i in range(len(blobs)) if status[i] != L.FI_OK]

    def _gpu_encode(self, outs, quality, held, webp=None):
        """Every JPEG output in one fi_jpeg_encode_device call: device views
        as they are, host arrays (host-decoded sources) uploaded first; chroma
        as ``encode``: q >= 90 -> 4:4:4, else 4:2:0.  Alpha outputs: host PNG,
        or with ``gpu_png`` one fi_png_encode_device call for all of them.
        ``webp`` (gpu_webp): the outputs that leave as lossless WebP instead,
        opaque or not, through one fi_webp_encode_device call."""
        encoded = [None] * len(outs)
        views, idx = [], []
        png_views, png_idx = [], []
        webp_views, webp_idx = [], []
        for i, o in enumerate(outs):
            if webp and webp[i]:
                if isinstance(o, tuple):
                    view = o
                else:
                    ch = o.shape[2] if o.ndim == 3 else 1
                    o = np.ascontiguousarray(o)
                    p = self.ctx.malloc(max(o.nbytes, 1))
                    held.append(p)
                    self.ctx.h2d(p, o)
                    view = (p, o.shape[1], o.shape[0], o.shape[1] * ch, ch)
                webp_views.append(view)
                webp_idx.append(i)
                continue
            if isinstance(o, tuple):  # a device batch's output; 2 or 4 channels (alpha) from GPU-decoded PNGs
                view = o
                if view[4] in (2, 4):
                    if self.gpu_png:
                        png_views.append(view)
                        png_idx.append(i)
                    else:  # the host PNG writer takes pixels
                        p, w, h, st, c = view
                        px = self.ctx.d2h(p, h * st).reshape(h, st)[:, : w * c].reshape(h, w, c)
                        encoded[i] = encode(np.ascontiguousarray(px), quality[i])
                    continue
            else:
                ch = o.shape[2] if o.ndim == 3 else 1
                if ch in (2, 4) and not self.gpu_png:
                    encoded[i] = encode(o, quality[i])
                    continue
                o = np.ascontiguousarray(o)
                p = self.ctx.malloc(max(o.nbytes, 1))
                held.append(p)
                self.ctx.h2d(p, o)
                view = (p, o.shape[1], o.shape[0], o.shape[1] * ch, ch)
                if ch in (2, 4):
                    png_views.append(view)
                    png_idx.append(i)
                    continue
            views.append(view)
            idx.append(i)
        for i, f in zip(png_idx, self.ctx.png_encode(png_views)):
            if f is None:
                msg = L.lib().fi_last_error()
                raise ExecFailedException("Command failed.\nThe exit code: %d\n%s" % (
                    L.FI_EINVAL, msg.decode() if msg else f"image {i}: PNG encode"))
            encoded[i] = f
        for i, f in zip(webp_idx, self.ctx.webp_encode(webp_views)):
            if f is None:
                msg = L.lib().fi_last_error()
                raise ExecFailedException("Command failed.\nThe exit code: %d\n%s" % (
                    L.FI_EINVAL, msg.decode() if msg else f"image {i}: WebP encode"))
            encoded[i] = f
        qs = [int(quality[i]) for i in idx]
        files = self.ctx.jpeg_encode(views, qs, [0 if q >= 90 else 2 for q in qs],
                                     progressive=self.gpu_progressive_encode)
        for i, f in zip(idx, files):
            if f is None:
                msg = L.lib().fi_last_error()
                raise ExecFailedException("Command failed.\nThe exit code: %d\n%s" % (
                    L.FI_EINVAL, msg.decode() if msg else f"image {i}: JPEG encode"))
            encoded[i] = f
        return encoded

    def process(self, blobs: list[bytes], options: list[str]):
        """Returns (encoded outputs, fi_image records); a failed image raises
        ExecFailedException as Processor::execute does."""
        held = []  # device allocations that live until the GPU encode
        try:
            return self._process(blobs, options, held)
        finally:
            for p in held:
                self.ctx.free(p)

    def _process(self, blobs, options, held):
        bags = [OptionsBag(o) for o in options]
        n = len(blobs)
        outs, recs = [None] * n, [None] * n
        # extract (e_1) views start at any byte: the host path copies them to an
        # aligned array, so they decode there and take the same kernels
        # (bag.get: extract_key would consume the option, as InputImage::extractKey does)
        views = None
        if self.gpu_decode and self.gpu_orient:
            # ... unless the decoder applies the view itself: orientation from the
            # file, ExtractProcessor's rectangle of the oriented image
            dims, views = [None] * n, [None] * n
            for i, (b, bag) in enumerate(zip(blobs, bags)):
                d = gpu_decodable(b, self.gpu_progressive, orient=True)
                if d is None:
                    continue
                rect = (0, 0, 0, 0)
                if not _empty(bag.extract_key("extract")):  # (as ExtractProcessor.extract)
                    rect = ExtractProcessor.rectangle(bag, d[0], d[1])
                    d = (rect[2], rect[3], d[2])
                dims[i], views[i] = d, (0,) + rect
        else:
            dims = [gpu_decodable(b, self.gpu_progressive) if self.gpu_decode and _empty(bag.get("extract")) else None
                    for b, bag in zip(blobs, bags)]
        if self.gpu_png_decode:
            for i, (b, bag) in enumerate(zip(blobs, bags)):
                if dims[i] is None:
                    dims[i] = png_gpu_decodable(b, bag)
                    if views and dims[i] is not None:
                        views[i] = None
        host = [i for i in range(n) if dims[i] is None]
        gpu = [i for i in range(n) if dims[i] is not None]
        if gpu:
            o, r, back = self._gpu_batch([blobs[i] for i in gpu], [bags[i] for i in gpu], [dims[i] for i in gpu],
                                         held if self.gpu_encode else None,
                                         [views[i] for i in gpu] if views else None)
            for k, i in enumerate(gpu):
                outs[i], recs[i] = o[k], r[k]
            host += [gpu[k] for k in back]
            if views:  # (the view consumed their extract keys: the host path extracts from a fresh bag)
                for k in back:
                    bags[gpu[k]] = OptionsBag(options[gpu[k]])
        self.decode_stats["gpu"] += n - len(host)
        self.decode_stats["host"] += len(host)
        if host:
            o, r = self._host_batch([blobs[i] for i in host], [bags[i] for i in host])
            for k, i in enumerate(host):
                outs[i], recs[i] = o[k], r[k]
        for i, r in enumerate(recs):
            if r.status != L.FI_OK:
                msg = L.lib().fi_last_error()
                raise ExecFailedException("Command failed.\nThe exit code: %d\n%s" % (
                    r.status, msg.decode() if msg else f"image {i}"))
        import time

        quality = [self._quality(b) for b in bags]
        t0 = time.perf_counter()
        if self.gpu_encode:
            webp = None
            if self.gpu_webp:  # o_webp,webpl_1: ImageProcessor.php:199-203 (-define webp:lossless=true)
                webp = [b.get("output") == "webp" and not _empty(b.get("webp-lossless")) for b in bags]
            encoded = self._gpu_encode(outs, quality, held, webp)
        else:
            encoded = list(self.pool.map(lambda a: encode(a[0], a[1]), zip(outs, quality)))
        self.process_stats["s_encode"] += time.perf_counter() - t0
        self.process_stats["raw_bytes"] += sum(r.out_w * r.out_h * r.out_channels for r in recs)
        self.process_stats["encoded_bytes"] += sum(len(e) for e in encoded)
        return encoded, recs

    def _prepare(self, slot, blobs, options):
        """Decode (thread pool) straight into the slot's pinned sources; ops."""
        decoded = list(self.pool.map(decode_ex, blobs))
        views, ops, quality = [], [], []
        for (img, pseudo), opts in zip(decoded, options):
            bag = OptionsBag(opts)
            img = ExtractProcessor.extract(bag, img)
            h, w = img.shape[:2]
            q = bag.get_option("quality")
            quality.append(int(q) if not _empty(q) else 90)
            op = ImageProcessor(bag, w, h, shear_rotate=self.shear_rotate).to_op()
            if pseudo:
                op.flags |= L.FI_SRC_PSEUDOCLASS
            ops.append(op)
            views.append(img)
        pins = slot.sources([v.shape for v in views])
        list(self.pool.map(lambda a: np.copyto(a[0], a[1]), zip(pins, views)))
        return pins, ops, quality

    def process_batches(self, batches):
        """Pipelined form of ``process`` over an iterable of (blobs, options)
        batches: batch k+1 is decoded into pinned memory and submitted
        (fi_submit_batch) while batch k's DMA and kernels run, and batch k is
        encoded while batch k+1 runs (on the host encoder: ``gpu_encode``
        applies to ``process`` only -- this form's outputs are already in pinned
        host memory when the batch ends).  Yields (encoded outputs, records) per
        batch, in order; the ``stats`` attribute holds the host time spent
        decoding, blocked on the GPU, and encoding."""
        from .runtime import plan as fi_plan

        slots = [_PinnedSlot(self.ctx), _PinnedSlot(self.ctx)]
        self.stats = {"s_decode": 0.0, "s_gpu_wait": 0.0, "s_encode": 0.0}
        import time

        prev = None
        for k, (blobs, options) in enumerate(batches):
            t0 = time.perf_counter()
            slot = slots[k % 2]
            srcs, ops, quality = self._prepare(slot, blobs, options)
            sizes = []
            for src, op in zip(srcs, ops):
                ow, oh, oc = fi_plan(src.shape[1], src.shape[0], op)
                sizes.append(max(ow * oh * oc, 1))
            outs = slot.outputs(sizes)
            arr, outs = self.ctx.submit(srcs, ops, outs)
            t1 = time.perf_counter()
            self.stats["s_decode"] += t1 - t0
            if prev is not None:
                yield self._finish(prev, keep=1)
            prev = (arr, outs, quality, srcs)
        if prev is not None:
            yield self._finish(prev, keep=0)

    def _finish(self, batch, keep):
        import time

        arr, outs, quality, _ = batch
        t0 = time.perf_counter()
        self.ctx.wait(keep)  # that batch is final (its failures are in its records)
        t1 = time.perf_counter()
        for i in range(len(outs)):
            if arr[i].status != L.FI_OK:
                msg = L.lib().fi_last_error()
                raise ExecFailedException("Command failed.\nThe exit code: %d\n%s" % (
                    arr[i].status, msg.decode() if msg else f"image {i}"))
        views = self.ctx.views(arr, outs)
        encoded = list(self.pool.map(lambda a: encode(np.ascontiguousarray(a[0]), a[1]), zip(views, quality)))
        self.stats["s_gpu_wait"] += t1 - t0
        self.stats["s_encode"] += time.perf_counter() - t1
        return encoded, arr
