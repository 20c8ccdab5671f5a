"""Literal scalar restatement of ImageMagick 6.9's RotateImage (magick/shear.c,
Q16, non-HDRI) for SMALL opaque images -- test infrastructure only: the
reference the GPU rotation stage (flyimg_amd/csrc/fi_rotate.hip) and the host
planner (fi_plan.cpp plan_shear) are checked against.

Follows shear.c statement by statement:
  * RotateImage: the angle reduction, IntegralRotateImage, shear.x / shear.y,
    the bounds, BorderImage, the three shears, CropToFitImage;
  * XShearImage / YShearImage: the in-place scans with their running `pixel`,
    LEFT / RIGHT (UP / DOWN) directions, trailers and background runs;
  * MagickPixelCompositeAreaBlend (composite-private.h) for opaque pixels, the
    pixel cache's ClampToQuantum after every shear.
Every float is a Python float (IEEE f64), every expression in IM's order.

Where a line's step is too large for the canvas IM's scans clip by themselves
(a LEFT row with step > x_offset is skipped, which leaves the `x_offset + i <
step` prefix dead; RIGHT's guard against image->columns drops iterations): the
scans below keep those branches, and the library reproduces them -- the outer
rows of the third shear of a square image at 45 degrees take both.  What IM
does not guard is the RIGHT trailer at x_offset + step - 1, or offsets that
wrap in size_t: there it indexes outside the row.  ``contained`` is False
then, and the library rejects the image instead.
Parity with ImageMagick itself is unpinned (IM is absent here).
"""
from __future__ import annotations

import math

import numpy as np

QR = 65535.0
QSCALE = 1.0 / 65535.0
MAGICK_PI = 3.14159265358979323846264338327950288419716939937510
MAGICK_EPSILON = 1.0e-12


def q2c(q):
    """ScaleQuantumToChar, on ints or arrays."""
    q = np.asarray(q).astype(np.int64)
    return (((q + 128) - ((q + 128) >> 8)) >> 8).astype(np.uint8)


def clamp_to_quantum(v: float) -> int:
    if v <= 0.0:
        return 0
    if v >= QR:
        return 65535
    return int(v + 0.5)


def perceptible_reciprocal(x: float) -> float:
    sign = -1.0 if x < 0.0 else 1.0
    if sign * x >= MAGICK_EPSILON:
        return 1.0 / x
    return sign / MAGICK_EPSILON


def area_blend(p, q, area: float):
    """MagickPixelCompositeAreaBlend(p, OpaqueOpacity, q, OpaqueOpacity, area)
    -> MagickPixelCompositePlus, per channel, stored through ClampToQuantum."""
    alpha = QR - (1.0 - area) * (QR - 0.0)
    beta = QR - area * (QR - 0.0)
    Sa = 1.0 - QSCALE * alpha
    Da = 1.0 - QSCALE * beta
    gamma = Sa + Da
    if gamma > 1.0:  # RoundToUnity
        gamma = 1.0
    gamma = perceptible_reciprocal(gamma)
    return [clamp_to_quantum(gamma * (Sa * float(pc) + Da * float(qc))) for pc, qc in zip(p, q)]


def reduce_angle(degrees):
    """RotateImage's head: (rotations, shear.x, shear.y)."""
    angle = math.fmod(float(degrees), 360.0)
    if angle < -45.0:
        angle += 360.0
    rotations = 0
    while angle > 45.0:
        angle -= 90.0
        rotations += 1
    rotations %= 4
    rad = MAGICK_PI * angle / 180.0  # DegreesToRadians
    return rotations, -math.tan(rad / 2.0), math.sin(rad)


def integral_rotate(img: np.ndarray, rotations: int) -> np.ndarray:
    """IntegralRotateImage: clockwise quarter turns."""
    return np.ascontiguousarray(np.rot90(img, -rotations))


class _Flags:
    def __init__(self):
        self.contained = True


def _shear_line(line: list, s: float, k: int, nlines: int, ext: int, off: int, background, fl: _Flags):
    """One row of XShearImage (or one column of YShearImage): `line` is the
    whole canvas row (column), a list of channel lists, sheared in place."""
    n = len(line)  # image->columns (rows)
    displacement = s * (k - nlines / 2.0)
    if displacement == 0.0:
        return
    if displacement > 0.0:
        right = True
    else:
        displacement *= -1.0
        right = False
    step = int(math.floor(displacement))
    area = displacement - step
    step += 1
    pixel = list(background)
    if not right:
        # LEFT / UP: transfer pixels left-to-right
        if step > off:
            return
        p = off
        q = p - step
        for i in range(ext):
            if off + i < step:
                p += 1
                pixel = list(line[p])
                q += 1
                continue
            source = list(line[p])
            line[q] = area_blend(pixel, source, area)
            q += 1
            pixel = source
            p += 1
        line[q] = area_blend(pixel, background, area)
        q += 1
        for _ in range(step - 1):
            line[q] = list(background)
            q += 1
    else:
        # RIGHT / DOWN: transfer pixels right-to-left
        p = off + ext
        q = p + step
        if off + step > n:
            fl.contained = False  # the trailer below would index past the row
        for i in range(ext):
            p -= 1
            q -= 1
            if off + ext + step - i > n:
                continue
            source = list(line[p])
            line[q] = area_blend(pixel, source, area)
            pixel = source
        q -= 1
        if 0 <= q < n:
            line[q] = area_blend(pixel, background, area)
        for _ in range(step - 1):
            q -= 1
            if 0 <= q < n:
                line[q] = list(background)


def x_shear(R: list, s: float, width: int, height: int, x_off: int, y_off: int, background, fl: _Flags):
    if x_off < 0 or y_off < 0 or y_off + height > len(R) or x_off + width > len(R[0]):
        fl.contained = False
        return
    for y in range(height):
        _shear_line(R[y_off + y], s, y, height, width, x_off, background, fl)


def y_shear(R: list, s: float, width: int, height: int, x_off: int, y_off: int, background, fl: _Flags):
    if x_off < 0 or y_off < 0 or x_off + width > len(R[0]) or y_off + height > len(R):
        fl.contained = False
        return
    for x in range(width):
        col = [R[y][x_off + x] for y in range(len(R))]
        _shear_line(col, s, x, width, height, y_off, background, fl)
        for y in range(len(R)):
            R[y][x_off + x] = col[y]


def geometry(w: int, h: int, sx: float, sy: float):
    """RotateImage's bounds and CropToFitImage's rectangle for the w x h
    integral image: dict(bw, bh, bx, by, cols, rows, crop=(x, y, w, h))."""
    bw = int(abs(float(h) * sx) + w + 0.5)
    bh = int(abs(float(bw) * sy) + h + 0.5)
    sw = int(abs(float(bh) * sx) + bw + 0.5)
    bx = int(math.floor(float(w if sw > bw else bw - sw + 2) / 2.0 + 0.5))
    by = int(math.floor((float(bh) - h + 2) / 2.0 + 0.5))
    cols, rows = w + 2 * bx, h + 2 * by
    ext = [(-w / 2.0, -h / 2.0), (w / 2.0, -h / 2.0), (-w / 2.0, h / 2.0), (w / 2.0, h / 2.0)]
    pts = []
    for x, y in ext:
        x += sx * y
        y += sy * x
        x += sx * y
        x += cols / 2.0
        y += rows / 2.0
        pts.append((x, y))
    minx, maxx = min(p[0] for p in pts), max(p[0] for p in pts)
    miny, maxy = min(p[1] for p in pts), max(p[1] for p in pts)
    gx, gy = int(math.ceil(minx - 0.5)), int(math.ceil(miny - 0.5))
    gw, gh = int(math.floor(maxx - minx + 0.5)), int(math.floor(maxy - miny + 0.5))
    # CropImage: the rectangle intersected with the canvas
    if gx < 0:
        gw += gx
        gx = 0
    if gy < 0:
        gh += gy
        gy = 0
    if gx + gw > cols:
        gw = cols - gx
    if gy + gh > rows:
        gh = rows - gy
    return dict(bw=bw, bh=bh, bx=bx, by=by, cols=cols, rows=rows, crop=(gx, gy, gw, gh))


def rotate(img: np.ndarray, degrees: int, background=(65535, 65535, 65535)):
    """RotateImage(img, degrees) with image->background_color = background on a
    Q16 image (H, W) or (H, W, C): (rotated Q16 array, contained)."""
    a = np.asarray(img)
    gray = a.ndim == 2
    if gray:
        a = a[:, :, None]
    C = a.shape[2]
    background = [int(v) for v in background][:C]
    rotations, sx, sy = reduce_angle(degrees)
    I = integral_rotate(a, rotations)
    if sx == 0.0 and sy == 0.0:
        return (I[:, :, 0] if gray else I).astype(np.uint16), True
    h, w = I.shape[:2]
    g = geometry(w, h, sx, sy)
    bw, bh, bx, by, cols, rows = (g[k] for k in ("bw", "bh", "bx", "by", "cols", "rows"))
    # BorderImage
    R = [[list(background) for _ in range(cols)] for _ in range(rows)]
    for y in range(h):
        for x in range(w):
            R[by + y][bx + x] = [int(v) for v in I[y, x]]
    fl = _Flags()
    if cols < bw or rows < bh:  # IM's size_t offsets wrap here
        return None, False
    x_shear(R, sx, w, h, bx, (rows - h) // 2, background, fl)
    y_shear(R, sy, bw, h, (cols - bw) // 2, by, background, fl)
    x_shear(R, sx, bw, bh, (cols - bw) // 2, (rows - bh) // 2, background, fl)
    gx, gy, gw, gh = g["crop"]
    if gw <= 0 or gh <= 0:
        return None, False
    out = np.array([[R[gy + y][gx + x] for x in range(gw)] for y in range(gh)], dtype=np.uint16).reshape(gh, gw, C)
    return (out[:, :, 0] if gray else out), fl.contained


def rotated_size(w: int, h: int, degrees: int):
    """(out_w, out_h, contained) without touching pixels: the scans' containment
    conditions evaluated line by line."""
    rotations, sx, sy = reduce_angle(degrees)
    if rotations % 2:
        w, h = h, w
    if sx == 0.0 and sy == 0.0:
        return w, h, True
    g = geometry(w, h, sx, sy)
    bw, bh, bx, by, cols, rows = (g[k] for k in ("bw", "bh", "bx", "by", "cols", "rows"))
    ok = cols >= bw and rows >= bh

    def lines(s, nlines, ext, off, canvas):
        if off < 0 or off + ext > canvas:
            return False
        for k in range(nlines):
            d = s * (k - nlines / 2.0)
            if d == 0.0:
                continue
            step = int(math.floor(abs(d))) + 1
            if d > 0.0 and off + step > canvas:
                return False
        return True

    if ok:
        xo = (cols - bw) // 2
        ok = (lines(sx, h, w, bx, cols) and xo + bw <= cols and lines(sy, bw, h, by, rows)
              and (rows - bh) // 2 + bh <= rows and lines(sx, bh, bw, xo, cols))
    gx, gy, gw, gh = g["crop"]
    return gw, gh, ok
