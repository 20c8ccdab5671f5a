// fi_rotate.hip -- -rotate by an angle that is no multiple of 90, with
// -background (forwarded options, src/Core/Processor/ImageProcessor.php:303-315):
// IM 6.9 RotateImage (magick/shear.c, Q16, non-HDRI) past IntegralRotateImage,
// on the integrally rotated Q16 image the resample epilogue leaves in the
// workspace (ResizeDesc::q16out).
//
// IM borders the image with the background (BorderImage), shears the canvas in
// place three times (XShearImage, YShearImage, XShearImage: every written
// pixel is MagickPixelCompositeAreaBlend of two neighbours of the line, rounded
// to Q16 by the pixel cache) and crops (CropToFitImage).  Here no canvas
// exists: a shear's output pixel is a function of at most two pixels of the
// same line of the stage before it, so each output pixel is pulled backwards
//   crop -> canvas -> third shear's two taps -> each one's two taps of the
//   second -> each one's two taps of the first -> the image or the background
// which is at most 8 Q16 reads and 7 blends per channel, every stage's
// ClampToQuantum included.  shear_tap maps a canvas coordinate to what
// XShearImage / YShearImage left there, the scans' own clipping included: a
// LEFT row whose step exceeds x_offset is skipped (which leaves its `x_offset
// + i < step` prefix dead), and a RIGHT row drops the iterations IM's guard
// `x_offset + width + step - i > columns` drops -- the outer rows of the third
// shear of a square image at 45 degrees take both.  The planner (fi_plan.cpp
// plan_shear) rejects the images for which IM itself would index outside the
// row (a RIGHT trailer at x_offset + step - 1 >= columns) or whose offsets
// wrap, so every coordinate here lies on the canvas.
//
// Built with -ffp-contract=off: the f64 expressions are IM's, operation by
// operation, so the pixels are tests/rotate_literal.py's bit for bit.
//
// Work item: a tile of kRotTileH output rows x kRotTileW pixels, one wave per
// row, 4 pixels per lane (8-bit rows that are dword aligned are stored as
// whole dwords).  No LDS.  HBM traffic: the Q16 image once (its re-reads hit
// L2) and the output once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fi_internal.h"

namespace fi {

__device__ __forceinline__ int rt_find(const int32_t *prefix, int n, int t) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// What a shear left at position u of one line: the stage before it at a
// (kPass), the background (kBg), or blend(a, b) where a negative coordinate
// stands for the background
enum { kPass = 0, kBg = 1, kBlend = 2 };
struct Tap {
  int mode, a, b;
  double sa, da, g;  // MagickPixelCompositeAreaBlend's Sa, Da and 1 / gamma for the line's area
};

// XShearImage: line = row, u = column, nlines = height, ext = width, canvas = columns.
// YShearImage: line = column, u = row, nlines = width, ext = height, canvas = rows.
__host__ __device__ __forceinline__ Tap shear_tap(double s, int nlines, int line_off, int ext, int ext_off, int canvas,
                                         int line, int u) {
  Tap t;
  t.mode = kPass;
  t.a = u;
  t.b = -1;
  t.sa = t.da = t.g = 0.0;
  const int k = line - line_off;
  if (k < 0 || k >= nlines) return t;
  double d = s * ((double)k - (double)nlines / 2.0);
  if (d == 0.0) return t;
  const bool right = d > 0.0;
  if (!right) d *= -1.0;
  const double fl = floor(d);
  const double area = d - fl;
  const int step = (int)fl + 1;
  if (!right) {  // LEFT / UP: q = p - step, written left to right
    if (step > ext_off) return t;  // IM skips the line
    const int i = u - (ext_off - step);
    if (i < 0 || i >= ext + step) return t;
    if (i < ext) {
      t.mode = kBlend;
      t.a = i == 0 ? -1 : ext_off + i - 1;
      t.b = ext_off + i;
    } else if (i == ext) {
      t.mode = kBlend;
      t.a = ext_off + ext - 1;
      t.b = -1;
    } else {
      t.mode = kBg;
    }
  } else {  // RIGHT / DOWN: q = p + step, written right to left
    // the first i0 iterations would write at or past `canvas`: IM's guard
    // skips them and `pixel` is still the background at the first one kept
    const int over = ext_off + ext + step - canvas, i0 = over > 0 ? over : 0;
    const int j = u - ext_off;
    if (j < 0 || j >= ext + step - i0) return t;
    if (j >= step) {
      const int p = u - step;
      t.mode = kBlend;
      t.a = p == ext_off + ext - 1 - i0 ? -1 : p + 1;
      t.b = p;
    } else if (j == step - 1) {
      t.mode = kBlend;
      t.a = ext_off;
      t.b = -1;
    } else {
      t.mode = kBg;
    }
  }
  if (t.mode == kBlend) {
    // MagickPixelCompositeAreaBlend of two opaque pixels (composite-private.h)
    const double alpha = 65535.0 - (1.0 - area) * (65535.0 - 0.0);
    const double beta = 65535.0 - area * (65535.0 - 0.0);
    const double qs = 1.0 / 65535.0;  // QuantumScale
    t.sa = 1.0 - qs * alpha;
    t.da = 1.0 - qs * beta;
    double g = t.sa + t.da;
    if (g > 1.0) g = 1.0;
    t.g = g >= 1.0e-12 ? 1.0 / g : 1.0 / 1.0e-12;  // PerceptibleReciprocal (g >= 0)
  }
  return t;
}

__host__ __device__ __forceinline__ double rt_blend(const Tap &t, double p, double q) {
  const double v = t.g * (t.sa * p + t.da * q);
  // ClampToQuantum
  if (!(v > 0.0)) return 0.0;
  if (v >= 65535.0) return 65535.0;
  return (double)(uint32_t)(v + 0.5);
}

// the canvas before the first shear: the image at (bx, by) on the background
__host__ __device__ __forceinline__ double rt_canvas(const RotDesc &D, int x, int y, int c, double bg) {
  const int ix = x - D.bx, iy = y - D.by;
  if (ix < 0 || ix >= D.w || iy < 0 || iy >= D.h) return bg;
  return (double)D.src[((int64_t)iy * D.w + ix) * D.C + c];
}

// Output pixel at canvas (X, Y) after the three shears: q[c] for c < D.C.
// The taps are the same for every channel and are found once.
__host__ __device__ __forceinline__ void rt_pixel(const RotDesc &D, int X, int Y, uint32_t q[3]) {
  const RotShear S1 = D.sh[0], S2 = D.sh[1], S3 = D.sh[2];
  // third shear (X): row Y
  const Tap t3 = shear_tap(S3.s, S3.height, S3.y_off, S3.width, S3.x_off, D.cols, Y, X);
  const int x2[2] = {t3.a, t3.mode == kBlend ? t3.b : -1};
  Tap t2[2], t1[2][2];
  int y1[2][2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    // second shear (Y): column x2[k]
    t2[k] = shear_tap(S2.s, S2.width, S2.x_off, S2.height, S2.y_off, D.rows, x2[k], Y);
    y1[k][0] = t2[k].a;
    y1[k][1] = t2[k].mode == kBlend ? t2[k].b : -1;
#pragma unroll
    for (int m = 0; m < 2; m++)  // first shear (X): row y1[k][m]
      t1[k][m] = shear_tap(S1.s, S1.height, S1.y_off, S1.width, S1.x_off, D.cols, y1[k][m], x2[k]);
  }
  for (int c = 0; c < D.C; c++) {
    const double bg = (double)D.bg[c];
    double v2[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      v2[k] = bg;
      if (x2[k] < 0 || t3.mode == kBg || t2[k].mode == kBg) continue;
      double v1[2];
#pragma unroll
      for (int m = 0; m < 2; m++) {
        v1[m] = bg;
        const Tap &t = t1[k][m];
        const int y = y1[k][m];
        if (y < 0 || t.mode == kBg) continue;
        const double va = t.a >= 0 ? rt_canvas(D, t.a, y, c, bg) : bg;
        if (t.mode == kPass) {
          v1[m] = va;
        } else {
          const double vb = t.b >= 0 ? rt_canvas(D, t.b, y, c, bg) : bg;
          v1[m] = rt_blend(t, va, vb);
        }
      }
      v2[k] = t2[k].mode == kPass ? v1[0] : rt_blend(t2[k], v1[0], v1[1]);
    }
    const double v = t3.mode == kBg ? bg : t3.mode == kPass ? v2[0] : rt_blend(t3, v2[0], v2[1]);
    q[c] = (uint32_t)v;
  }
}
__host__ __device__ __forceinline__ uint32_t rt_q2c(uint32_t q) {  // ScaleQuantumToChar
  return ((q + 128u) - ((q + 128u) >> 8)) >> 8;
}

__global__ __launch_bounds__(256) void k_rotate(const RotDesc *__restrict__ descs, const int32_t *__restrict__ prefix,
                                                int n) {
  const int tile = blockIdx.x;
  const int img = rt_find(prefix, n, tile);
  const RotDesc &D = descs[img];
  const int lt = tile - prefix[img];
  const int tx = (D.cw + kRotTileW - 1) / kRotTileW;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int oy = (lt / tx) * kRotTileH + wave;
  const int ox0 = (lt % tx) * kRotTileW + lane * 4;
  if (oy >= D.ch || ox0 >= D.cw) return;
  const int C = D.C;
  const int Y = D.cy + oy;
  uint64_t lo = 0, hi = 0;  // the lane's 8-bit output bytes, first byte lowest
  const int npx = min(4, D.cw - ox0);
#pragma unroll 1
  for (int p = 0; p < npx; p++) {
    uint32_t q[3];
    rt_pixel(D, D.cx + ox0 + p, Y, q);
    for (int c = 0; c < C; c++) {
      if (D.dst16) D.dst16[(int64_t)oy * D.stride16 + (int64_t)(ox0 + p) * C + c] = (uint16_t)q[c];
      const uint64_t b8 = rt_q2c(q[c]);
      const int bi = p * C + c;
      if (bi < 8)
        lo |= b8 << (8 * bi);
      else
        hi |= b8 << (8 * (bi - 8));
    }
  }
  if (!D.dst8) return;
  uint8_t *o = D.dst8 + (int64_t)oy * D.stride8 + (int64_t)ox0 * C;
  const int nb = npx * C;
  if (npx == 4 && (((uintptr_t)o) & 3) == 0) {
    uint32_t *o4 = reinterpret_cast<uint32_t *>(o);
    o4[0] = (uint32_t)lo;
    if (C == 3) {
      o4[1] = (uint32_t)(lo >> 32);
      o4[2] = (uint32_t)hi;
    }
  } else {
    for (int b = 0; b < nb; b++) o[b] = (uint8_t)(b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8)));
  }
}

// The kernel's per-pixel procedure on the host, over host buffers (test hook
// fi_debug_rotate_host: the CPU suite checks it against the literal).
void rot_host(const RotDesc &D) {
  for (int oy = 0; oy < D.ch; oy++)
    for (int ox = 0; ox < D.cw; ox++) {
      uint32_t q[3];
      rt_pixel(D, D.cx + ox, D.cy + oy, q);
      for (int c = 0; c < D.C; c++) {
        if (D.dst16) D.dst16[(int64_t)oy * D.stride16 + (int64_t)ox * D.C + c] = (uint16_t)q[c];
        if (D.dst8) D.dst8[(int64_t)oy * D.stride8 + (int64_t)ox * D.C + c] = (uint8_t)rt_q2c(q[c]);
      }
    }
}

int launch_rot(hipStream_t s, const RotDesc *descs, const int32_t *prefix, int n, int tiles) {
  if (n <= 0 || tiles <= 0) return 0;
  hipLaunchKernelGGL(k_rotate, dim3(tiles), dim3(256), 0, s, descs, prefix, n);
  return 0;
}

}  // namespace fi
