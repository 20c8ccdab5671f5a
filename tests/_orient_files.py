"""JPEG files with hand-built EXIF / XMP APP1 segments, shared by
tests/test_jpeg_orient_cpu.py and tests/test_gpu_jpeg_view.py."""
import io
import struct

import numpy as np
from PIL import Image, ImageOps

XMP_ID = b"http://ns.adobe.com/xap/1.0/\x00"


def photo(w, h, seed=7, gray=False):
    """A smooth picture with some noise (every block has AC energy), HWC uint8."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [128 + 90 * np.sin(x / (3.0 + k) + k) * np.cos(y / (4.0 + k)) + 12 * rng.standard_normal((h, w))
          for k in range(1 if gray else 3)]
    px = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    return px[..., 0] if gray else px


def jpeg(px, **kw):
    buf = io.BytesIO()
    kw.setdefault("quality", 85)
    Image.fromarray(px).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_oriented(px, k, **kw):
    """Written by Pillow itself with exif[0x0112] = k."""
    exif = Image.Exif()
    exif[0x0112] = k
    return jpeg(px, exif=exif, **kw)


def segment(marker, payload):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload


def tiff(orientation=6, le=True, typ=3, count=1, ifd_off=8, entries=None, pad=b""):
    """A TIFF structure whose IFD0 holds ``entries`` (default: ImageWidth, the
    orientation tag and ResolutionUnit); (tag, type, count, 4 value bytes)."""
    e = "<" if le else ">"
    if entries is None:
        val = struct.pack(e + "HH", orientation, 0) if typ == 3 else struct.pack(e + "L", orientation)
        entries = [(0x0100, 4, 1, struct.pack(e + "L", 640)), (0x0112, typ, count, val),
                   (0x0128, 3, 1, struct.pack(e + "HH", 2, 0))]
    ifd = struct.pack(e + "H", len(entries))
    for tag, ty, cnt, val in entries:
        ifd += struct.pack(e + "HHL", tag, ty, cnt) + val
    ifd += struct.pack(e + "L", 0)
    head = (b"II*\x00" if le else b"MM\x00*") + struct.pack(e + "L", ifd_off)
    return head + b"\x00" * max(0, ifd_off - 8) + ifd + pad


def exif_app1(*a, **kw):
    return segment(0xE1, b"Exif\x00\x00" + tiff(*a, **kw))


def xmp_app1(orientation):
    body = ('<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#">'
            '<rdf:Description xmlns:tiff="http://ns.adobe.com/tiff/1.0/" tiff:Orientation="%d"/></rdf:RDF></x:xmpmeta>'
            % orientation)
    return segment(0xE1, XMP_ID + body.encode())


def splice(blob, segs, before_jfif=False):
    """``segs`` (bytes) after the JFIF APP0 of a Pillow-written file, or before it."""
    assert blob[:4] == b"\xff\xd8\xff\xe0"
    p = 2 if before_jfif else 4 + struct.unpack(">H", blob[4:6])[0]
    return blob[:p] + segs + blob[p:]


def host_orientation(blob):
    """The orientation the host decode path applies (codec.decode_ex)."""
    o = Image.open(io.BytesIO(blob)).getexif().get(0x0112, 1)
    return o if o in range(2, 9) else 1


def reference(blob, rect=None, mode="RGB"):
    im = ImageOps.exif_transpose(Image.open(io.BytesIO(blob))).convert(mode)
    a = np.asarray(im)
    if rect:
        x, y, w, h = rect
        a = a[y:y + h, x:x + w]
    return a
