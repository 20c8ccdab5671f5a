// fi_plan.cpp -- host planner: ImageMagick geometry and tap tables.  Every
// floating-point expression mirrors the reference's evaluation order (built
// with -ffp-contract=off): ImageMagick 6.9 geometry.c ParseMetaGeometry /
// GravityAdjustGeometry, shear.c RotateImage, resize.c ThumbnailImage /
// SampleImage / ResizeImage contribution lists and ScaleImage (flyimg emits
// them from ImageProcessor.php:66-110).  The MFMA tables built from the tap
// tables are in fi_plan_mfma.cpp, Pillow's and smartcrop.py's side in
// fi_plan_sc.cpp.
#include "fi_plan.h"

#include <math.h>

#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace fi {

static constexpr double kImEpsilon = 1.0e-12;  // MagickEpsilon

// ---------------------------------------------------------------------------
// ImageMagick geometry
// ---------------------------------------------------------------------------
static void meta_geometry(int W, int H, int tw, int th, bool fill, bool shrink, int *ow, int *oh) {
  double scale;
  const bool has_w = tw > 0, has_h = th > 0;
  if (has_w && has_h) {
    scale = (double)tw / (double)W;
    if (!fill) {
      if (scale > ((double)th / (double)H)) scale = (double)th / (double)H;
    } else if (scale < ((double)th / (double)H)) {
      scale = (double)th / (double)H;
    }
  } else if (has_w) {
    scale = (double)tw / (double)W;
    if (fill && scale < ((double)tw / (double)H)) scale = (double)tw / (double)H;
  } else {
    scale = (double)th / (double)H;
    if (fill && scale < ((double)th / (double)W)) scale = (double)th / (double)W;
  }
  long w = (long)floor(scale * W + 0.5), h = (long)floor(scale * H + 0.5);
  if (w < 1) w = 1;
  if (h < 1) h = 1;
  if (shrink) {
    if (W < w) w = W;
    if (H < h) h = H;
  }
  *ow = (int)w;
  *oh = (int)h;
}

static void gravity_offset(int W, int H, int ew, int eh, int gravity, int *x, int *y) {
  long ox = 0, oy = 0;
  switch (gravity) {
    case FI_GRAVITY_NORTHEAST: case FI_GRAVITY_EAST: case FI_GRAVITY_SOUTHEAST:
      ox = (long)((unsigned long)W - (unsigned long)ew);
      break;
    case FI_GRAVITY_NORTH: case FI_GRAVITY_SOUTH: case FI_GRAVITY_CENTER:
      ox = (long)((unsigned long)W / 2 - (unsigned long)ew / 2);
      break;
    default: break;
  }
  switch (gravity) {
    case FI_GRAVITY_SOUTHWEST: case FI_GRAVITY_SOUTH: case FI_GRAVITY_SOUTHEAST:
      oy = (long)((unsigned long)H - (unsigned long)eh);
      break;
    case FI_GRAVITY_EAST: case FI_GRAVITY_WEST: case FI_GRAVITY_CENTER:
      oy = (long)((unsigned long)H / 2 - (unsigned long)eh / 2);
      break;
    default: break;
  }
  *x = (int)ox;
  *y = (int)oy;
}

// ---------------------------------------------------------------------------
// IM 6.9 RotateImage (shear.c): angle reduction, shear constants, BorderImage's
// canvas, the XShearImage / YShearImage arguments and CropToFitImage
// ---------------------------------------------------------------------------
static constexpr double kImPi = 3.14159265358979323846264338327950288419716939937510;  // MagickPI
void plan_rotate_angle(int degrees, ShearPlan *s) {
  *s = ShearPlan();
  double angle = fmod((double)degrees, 360.0);
  if (angle < -45.0) angle += 360.0;
  int rotations = 0;
  for (; angle > 45.0; rotations++) angle -= 90.0;
  rotations %= 4;
  s->rot = 90 * rotations;
  const double rad = kImPi * angle / 180.0;  // DegreesToRadians
  s->sx = -tan(rad / 2.0);
  s->sy = sin(rad);
  s->on = !(s->sx == 0.0 && s->sy == 0.0);
}
// IM's scans clip by themselves where a line's step is too large for the
// canvas: a LEFT / UP line with step > off is skipped, a RIGHT / DOWN line
// drops the iterations that would write past the canvas.  fi_rotate.hip
// reproduces both.  What IM does not guard is the RIGHT / DOWN trailer at off +
// step - 1: past the canvas it leaves the row, and such an image is rejected.
// The lines k = 0 and nlines - 1 carry the largest step (|d| = |s (k - nlines /
// 2)| falls towards the middle line).
static bool shear_contained(double s, int nlines, int ext, int off, int canvas) {
  if (off < 0 || off + ext > canvas) return false;
  for (int k : {0, nlines - 1}) {
    double d = s * ((double)k - nlines / 2.0);
    if (d == 0.0) continue;
    const bool right = d > 0.0;
    if (!right) d *= -1.0;
    if (d > 1e9) return false;
    const long step = (long)floor(d) + 1;
    if (right && off + step > canvas) return false;
  }
  return true;
}
bool plan_shear(int w, int h, ShearPlan *s) {
  const double sx = s->sx, sy = s->sy;
  s->w = w;
  s->h = h;
  const double fbw = fabs((double)h * sx) + w + 0.5;
  if (!(fbw < 1e9)) return false;
  const long bw = (long)fbw;
  const double fbh = fabs((double)bw * sy) + h + 0.5;
  if (!(fbh < 1e9)) return false;
  const long bh = (long)fbh;
  const long sw = (long)(fabs((double)bh * sx) + bw + 0.5);
  const long bx = (long)floor((double)((sw > bw) ? w : bw - sw + 2) / 2.0 + 0.5);
  const long by = (long)floor(((double)bh - h + 2) / 2.0 + 0.5);
  const long cols = w + 2 * bx, rows = h + 2 * by;
  if (bx < 0 || by < 0 || cols > (1 << 30) || rows > (1 << 30)) return false;
  s->bx = (int)bx;
  s->by = (int)by;
  s->cols = (int)cols;
  s->rows = (int)rows;
  // (IM computes these offsets in size_t: a canvas narrower than bounds.width
  // wraps there; here it is simply not contained)
  s->contained = cols >= bw && rows >= bh && rows >= h;
  const int xo = (int)((cols - bw) / 2), yo3 = (int)((rows - bh) / 2);
  s->sh[0] = RotShear{sx, w, h, (int)bx, (int)((rows - h) / 2)};
  s->sh[1] = RotShear{sy, (int)bw, h, xo, (int)by};
  s->sh[2] = RotShear{sx, (int)bw, (int)bh, xo, yo3};
  if (s->contained) {
    for (int k = 0; k < 3; k++) {
      const RotShear &q = s->sh[k];
      const bool ok = k == 1 ? (q.x_off >= 0 && q.x_off + q.width <= s->cols &&
                                shear_contained(q.s, q.width, q.height, q.y_off, s->rows))
                             : (q.y_off >= 0 && q.y_off + q.height <= s->rows &&
                                shear_contained(q.s, q.height, q.width, q.x_off, s->cols));
      s->contained = s->contained && ok;
    }
  }
  // CropToFitImage(rotate = MagickTrue), then CropImage's clip to the canvas
  double minx = 0, miny = 0, maxx = 0, maxy = 0;
  for (int i = 0; i < 4; i++) {
    double x = (i & 1) ? (double)w / 2.0 : (double)(-(double)w / 2.0);
    double y = (i & 2) ? (double)h / 2.0 : (double)(-(double)h / 2.0);
    x += sx * y;
    y += sy * x;
    x += sx * y;
    x += (double)cols / 2.0;
    y += (double)rows / 2.0;
    if (i == 0 || x < minx) minx = x;
    if (i == 0 || x > maxx) maxx = x;
    if (i == 0 || y < miny) miny = y;
    if (i == 0 || y > maxy) maxy = y;
  }
  long cx = (long)ceil(minx - 0.5), cy = (long)ceil(miny - 0.5);
  long cw = (long)floor(maxx - minx + 0.5), ch = (long)floor(maxy - miny + 0.5);
  if (cx < 0) cw += cx, cx = 0;
  if (cy < 0) ch += cy, cy = 0;
  if (cx + cw > cols) cw = cols - cx;
  if (cy + ch > rows) ch = rows - cy;
  if (cw <= 0 || ch <= 0) return false;
  s->cx = (int)cx;
  s->cy = (int)cy;
  s->cw = (int)cw;
  s->ch = (int)ch;
  return true;
}

int plan_im(const fi_image &img, ImPlan *p) {
  *p = ImPlan();
  p->W = img.src_w;
  p->H = img.src_h;
  p->C = img.src_channels;
  auto fail = [&](int code, const char *m) {
    p->status = code;
    p->err = m;
    return code;
  };
  if (img.src_w <= 0 || img.src_h <= 0) return fail(FI_EINVAL, "source dimensions must be positive");
  // RGB8, or RGBA8 (straight alpha, a PNG with an alpha channel: IM's matte
  // image -- Mitchell filter, alpha-weighted resample)
  if (img.src_channels != 3 && img.src_channels != 4)
    return fail(FI_EUNSUPPORTED, "only RGB8 / RGBA8 sources (src_channels 3 or 4) are supported");
  if ((int64_t)img.src_stride < (int64_t)img.src_w * img.src_channels) return fail(FI_EINVAL, "src_stride < C*src_w");
  const bool matte = img.src_channels == 4;
  const uint32_t f = img.flags;
  if ((f & FI_OP_THUMBNAIL) && (f & FI_OP_RESIZE)) return fail(FI_EINVAL, "both -thumbnail and -resize");
  const bool has_geom = img.target_w > 0 || img.target_h > 0;
  p->tw = p->W;
  p->th = p->H;
  if (has_geom) {
    if (!(f & (FI_OP_THUMBNAIL | FI_OP_RESIZE))) return fail(FI_EINVAL, "geometry without a resize operator");
    meta_geometry(p->W, p->H, img.target_w, img.target_h, f & FI_GEOM_FILL, f & FI_GEOM_SHRINK_ONLY, &p->tw,
                  &p->th);
  }
  p->resize = (p->tw != p->W || p->th != p->H);
  p->sw = p->W;
  p->sh = p->H;
  if (p->resize && (f & FI_OP_THUMBNAIL)) {
    // ThumbnailImage: area factor <= 0.1 and 5*w, 5*h >= 128 -> SampleImage
    const double xf = (double)p->tw / (double)p->W, yf = (double)p->th / (double)p->H;
    if (!((xf * yf) > 0.1) && !((5 * p->tw) < 128 || (5 * p->th) < 128)) {
      p->sample = true;
      p->sw = 5 * p->tw;
      p->sh = 5 * p->th;
    }
  }
  if (p->resize) {
    p->xf = (double)p->tw / (double)p->sw;
    p->yf = (double)p->th / (double)p->sh;
    // ResizeImage with the default filter (resize.c): Mitchell for PseudoClass
    // (palette / gray) and matte (alpha) sources and for enlargements, Lanczos otherwise
    const bool pseudo = (f & FI_SRC_PSEUDOCLASS) != 0;
    p->filter = (matte || pseudo || (p->xf * p->yf) > 1.0) ? kFilterMitchell : kFilterLanczos;
    p->hfirst = p->xf > p->yf;
  }
  p->ex0 = p->ey0 = 0;
  p->ew = p->tw;
  p->eh = p->th;
  if (f & FI_OP_EXTENT) {
    const int ew = img.target_w > 0 ? img.target_w : p->tw;
    const int eh = img.target_h > 0 ? img.target_h : p->th;
    int gx, gy;
    gravity_offset(p->tw, p->th, ew, eh, img.gravity ? img.gravity : FI_GRAVITY_CENTER, &gx, &gy);
    if (gx < 0 || gy < 0 || gx + ew > p->tw || gy + eh > p->th)
      return fail(FI_EUNSUPPORTED, "-extent larger than the resized image (background fill) is not supported");
    p->ex0 = gx;
    p->ey0 = gy;
    p->ew = ew;
    p->eh = eh;
  }
  // -monochrome (ImageProcessor.php:90-92) converts to GRAY first (SetImageType Bilevel)
  p->mono = (f & FI_OP_MONOCHROME) != 0;
  p->gray = (f & FI_OP_GRAY) != 0 || p->mono;
  p->rot = 0;
  if (f & FI_OP_ROTATE) {
    if ((img.rotate % 90) && (f & FI_OP_ROTATE_SHEAR)) {
      plan_rotate_angle(img.rotate, &p->shear);
      p->rot = p->shear.rot;
    } else {
      if (img.rotate % 90) return fail(FI_EUNSUPPORTED, "only -rotate by multiples of 90 (IntegralRotateImage)");
      p->rot = ((img.rotate % 360) + 360) % 360;
    }
  }
  if (matte && (f & FI_OP_BACKGROUND)) return fail(FI_EUNSUPPORTED, "-background of an RGBA image is not on the GPU path");
  if (f & FI_OP_BACKGROUND) p->bg = img.background & 0xFFFFFFu;
  if (p->shear.on) {
    if (matte) return fail(FI_EUNSUPPORTED, "-rotate by a non-multiple of 90 of an RGBA image is not on the GPU path");
    if (p->mono) return fail(FI_EUNSUPPORTED, "-rotate by a non-multiple of 90 of a -monochrome image is not on the GPU path");
    if (p->gray && ((p->bg >> 16) != ((p->bg >> 8) & 255u) || (p->bg >> 16) != (p->bg & 255u)))
      return fail(FI_EUNSUPPORTED, "-rotate of a Gray image with a coloured -background is not on the GPU path");
  }
  if (matte && p->mono) return fail(FI_EUNSUPPORTED, "-monochrome of an RGBA source is not on the GPU path");
  if (matte && (f & FI_OP_SMARTCROP))
    return fail(FI_EUNSUPPORTED, "smartcrop of an RGBA image: smartcrop.py fails on RGBA (split(), smartcrop.py:17)");
  p->out_c = matte ? (p->gray ? 2 : 4) : (p->gray ? 1 : 3);
  p->conv = ((f & FI_OP_UNSHARP) ? 1u : 0u) | ((f & FI_OP_SHARPEN) ? 2u : 0u) | ((f & FI_OP_BLUR) ? 4u : 0u);
  if (p->conv) {
    if (matte || p->mono)
      return fail(FI_EUNSUPPORTED, "-unsharp/-sharpen/-blur of an RGBA or -monochrome image are not on the GPU path");
    for (int k = 0; k < 4; k++) p->cv[k] = img.unsharp[k];
    p->cv[4] = img.sharpen[0];
    p->cv[5] = img.sharpen[1];
    p->cv[6] = img.blur[0];
    p->cv[7] = img.blur[1];
    for (double v : p->cv)
      if (!std::isfinite(v) || fabs(v) > 1e6) return fail(FI_EINVAL, "convolution parameter out of range");
    std::vector<double> kk;
    if ((p->conv & 1) && im_blur_kernel(p->cv[0], p->cv[1], &kk) < 0)
      return fail(FI_EUNSUPPORTED, "-unsharp kernel wider than the GPU path supports");
    if ((p->conv & 2) && im_sharpen_kernel(p->cv[4], p->cv[5], &kk) < 0)
      return fail(FI_EUNSUPPORTED, "-sharpen kernel wider than the GPU path supports");
    if ((p->conv & 4) && im_blur_kernel(p->cv[6], p->cv[7], &kk) < 0)
      return fail(FI_EUNSUPPORTED, "-blur kernel wider than the GPU path supports");
  }
  const bool swap = p->rot == 90 || p->rot == 270;
  p->out_w = p->iw = swap ? p->eh : p->ew;
  p->out_h = p->ih = swap ? p->ew : p->eh;
  if (p->shear.on) {
    if (!plan_shear(p->iw, p->ih, &p->shear)) return fail(FI_EUNSUPPORTED, "-rotate: the rotated image is empty or too large");
    if (!p->shear.contained) return fail(FI_EUNSUPPORTED, "-rotate: shear leaves IM's canvas (tall, narrow image)");
    p->out_w = p->shear.cw;
    p->out_h = p->shear.ch;
  }
  return FI_OK;
}

// --- forwarded convolution kernels (IM 6.9 gem.c / morphology.c / effect.c) ----
static double conv_reciprocal(double x) {  // PerceptibleReciprocal
  const double sign = x < 0.0 ? -1.0 : 1.0;
  if ((sign * x) >= kImEpsilon) return 1.0 / x;
  return sign / kImEpsilon;
}
static constexpr double kSq2Pi = 2.50662827463100024161235523934010416269302368164062;  // MagickSQ2PI
static constexpr double k2Pi = 6.283185307179586476925286766559005768394338798750211641949;  // Magick2PI
static int kernel_width_1d(double radius, double sigma) {  // GetOptimalKernelWidth1D
  if (radius > kImEpsilon) return (int)(2.0 * ceil(radius) + 1.0);
  const double gamma = fabs(sigma);
  if (gamma <= kImEpsilon) return 3;
  const double alpha = conv_reciprocal(2.0 * gamma * gamma), beta = conv_reciprocal(kSq2Pi * gamma);
  int width;
  for (width = 5; width < 4 * kConvMaxBlur;) {
    double normalize = 0.0;
    const int j = (width - 1) / 2;
    for (int i = -j; i <= j; i++) normalize += exp(-((double)(i * i)) * alpha) * beta;
    const double value = exp(-((double)(j * j)) * alpha) * beta / normalize;
    if ((value < 1.0 / 65535.0) || (value < kImEpsilon)) break;
    width += 2;
  }
  return width - 2;
}
static int kernel_width_2d(double radius, double sigma) {  // GetOptimalKernelWidth2D
  if (radius > kImEpsilon) return (int)(2.0 * ceil(radius) + 1.0);
  const double gamma = fabs(sigma);
  if (gamma <= kImEpsilon) return 3;
  const double alpha = conv_reciprocal(2.0 * gamma * gamma), beta = conv_reciprocal(k2Pi * gamma * gamma);
  int width;
  for (width = 5; width < 4 * kConvMaxSharpen;) {
    double normalize = 0.0;
    const int j = (width - 1) / 2;
    for (int v = -j; v <= j; v++)
      for (int u = -j; u <= j; u++) normalize += exp(-((double)(u * u + v * v)) * alpha) * beta;
    const double value = exp(-((double)(j * j)) * alpha) * beta / normalize;
    if ((value < 1.0 / 65535.0) || (value < kImEpsilon)) break;
    width += 2;
  }
  return width - 2;
}
int im_blur_kernel(double radius, double sigma, std::vector<double> *k) {
  sigma = fabs(sigma);
  const int width = radius >= 1.0 ? (int)radius * 2 + 1 : kernel_width_1d(radius, sigma);
  if (width < 1 || width > kConvMaxBlur) return -1;
  k->assign(width, 0.0);
  const int x = (width - 1) / 2;
  if (sigma > kImEpsilon) {  // KernelRank 3: a Gaussian 3x as wide, binned
    const int v = (width * 3 - 1) / 2;
    const double s3 = sigma * 3.0;
    const double alpha = 1.0 / (2.0 * s3 * s3), beta = 1.0 / (kSq2Pi * s3);
    for (int u = -v; u <= v; u++) (*k)[(u + v) / 3] += exp(-((double)(u * u)) * alpha) * beta;
  } else {
    (*k)[x] = 1.0;
  }
  double pos = 0.0;  // ScaleKernelInfo(1.0, CorrelateNormalizeValue): 1 / positive range
  for (double v : *k)
    if (v > 0.0) pos += v;
  const double scale = 1.0 / (fabs(pos) >= kImEpsilon ? pos : 1.0);
  for (double &v : *k) v *= scale;
  return width;
}
int im_sharpen_kernel(double radius, double sigma, std::vector<double> *k) {
  const int width = kernel_width_2d(radius, sigma);
  if (width < 1 || width > kConvMaxSharpen) return -1;
  k->assign((size_t)width * width, 0.0);
  const double ms = fabs(sigma) < kImEpsilon ? kImEpsilon : sigma;  // MagickSigma
  const int j = (width - 1) / 2;
  double normalize = 0.0;
  int i = 0;
  for (int v = -j; v <= j; v++)
    for (int u = -j; u <= j; u++) {
      (*k)[i] = -exp(-((double)u * u + v * v) / (2.0 * ms * ms)) /
                (2.0 * 3.14159265358979323846264338327950288419716939937510 * ms * ms);
      normalize += (*k)[i];
      i++;
    }
  (*k)[i / 2] = (-2.0) * normalize;
  normalize = 0.0;
  for (double v : *k) normalize += v;
  const double gamma = conv_reciprocal(normalize);
  for (double &v : *k) v *= gamma;
  return width;
}

// --- resize.c filters --------------------------------------------------------
static double sinc(double x) {
  if (x != 0.0) {
    const double alpha = 3.14159265358979323846264338327950288419716939937510 * x;
    return sin(alpha) / alpha;
  }
  return 1.0;
}
static double sincfast(double x) {
  if (x > 4.0) return sinc(x);
  const double xx = x * x;
  const double c0 = 0.173611107357320220183368594093166520811e-2;
  const double c1 = -0.384240921114946632192116762889211361285e-3;
  const double c2 = 0.394201182359318128221229891724947048771e-4;
  const double c3 = -0.250963301609117217660068889165550534856e-5;
  const double c4 = 0.111902032818095784414237782071368805120e-6;
  const double c5 = -0.372895101408779549368465614321137048875e-8;
  const double c6 = 0.957694196677572570319816780188718518330e-10;
  const double c7 = -0.187208577776590710853865174371617338991e-11;
  const double c8 = 0.253524321426864752676094495396308636823e-13;
  const double c9 = -0.177084805010701112639035485248501049364e-15;
  const double p =
      c0 + xx * (c1 + xx * (c2 + xx * (c3 + xx * (c4 + xx * (c5 + xx * (c6 + xx * (c7 + xx * (c8 + xx * c9))))))));
  return (xx - 1.0) * (xx - 4.0) * (xx - 9.0) * (xx - 16.0) * p;
}
static double mitchell(double x) {
  const double B = 1.0 / 3.0, C = 1.0 / 3.0, twoB = B + B;
  const double k0 = 1.0 - (1.0 / 3.0) * B, k1 = -3.0 + twoB + C, k2 = 2.0 - 1.5 * B - C;
  const double k3 = (4.0 / 3.0) * B + 4.0 * C, k4 = -8.0 * C - twoB, k5 = B + 5.0 * C,
               k6 = (-1.0 / 6.0) * B - C;
  if (x < 1.0) return k0 + x * (x * (k1 + x * k2));
  if (x < 2.0) return k3 + x * (k4 + x * (k5 + x * k6));
  return 0.0;
}
static double filter_weight(int filter, double x) {
  const double xb = fabs(x) / 1.0;
  if (filter == kFilterLanczos) {
    const double scale = 1.0 / 3.0;
    const double win = sincfast(xb * scale);
    return win * sincfast(xb);
  }
  return 1.0 * mitchell(xb);
}
static double perceptible_reciprocal(double x) {
  const double sign = x < 0.0 ? -1.0 : 1.0;
  if ((sign * x) >= kImEpsilon) return 1.0 / x;
  return sign / kImEpsilon;
}

void build_axis(int filter, double factor, int in_sampled, int out_size, int o0, int o1, bool sample,
                int in_src, AxisTable *t) {
  (void)out_size;
  *t = AxisTable();
  double scale = fmax(1.0 / factor + kImEpsilon, 1.0);
  double support = scale * (filter == kFilterLanczos ? 3.0 : 2.0);
  if (support < 0.5) {
    support = 0.5;
    scale = 1.0;
  }
  scale = perceptible_reciprocal(scale);
  std::vector<double> w;
  std::vector<double> merged;
  t->src_lo = 1 << 30;
  t->src_hi = 0;
  for (int o = o0; o < o1; o++) {
    const double bisect = (double)(o + 0.5) / factor + kImEpsilon;
    const long s = (long)fmax(bisect - support + 0.5, 0.0);
    const long e = (long)fmin(bisect + support + 0.5, (double)in_sampled);
    const int n = (int)(e - s);
    w.assign(n > 0 ? n : 0, 0.0);
    double density = 0.0;
    for (int i = 0; i < n; i++) {
      w[i] = filter_weight(filter, scale * ((double)(s + i) - bisect + 0.5));
      density += w[i];
    }
    if (density != 0.0 && density != 1.0) {
      density = perceptible_reciprocal(density);
      for (int i = 0; i < n; i++) w[i] *= density;
    }
    // map sampled taps to source indices (SampleImage offsets) and merge
    auto src_of = [&](long j) -> long {
      if (!sample) return j;
      return (long)((((double)j + (0.5 - kImEpsilon)) * in_src) / in_sampled);
    };
    const long m0 = n > 0 ? src_of(s) : 0;
    const long m1 = n > 0 ? src_of(s + n - 1) : -1;
    const int cnt = (int)(m1 - m0 + 1);
    merged.assign(cnt > 0 ? cnt : 0, 0.0);
    for (int i = 0; i < n; i++) merged[src_of(s + i) - m0] += w[i];
    t->start.push_back((int32_t)m0);
    t->count.push_back(cnt);
    t->woff.push_back((int32_t)t->w.size());
    for (int i = 0; i < cnt; i++) {
      t->w.push_back((float)merged[i]);
      t->wd.push_back(merged[i]);
    }
    t->maxtaps = std::max(t->maxtaps, cnt);
    t->src_lo = std::min<int32_t>(t->src_lo, (int32_t)m0);
    t->src_hi = std::max<int32_t>(t->src_hi, (int32_t)(m0 + cnt));
  }
  if (o1 <= o0) t->src_lo = 0;
  // source indices carrying a non-zero weight (SampleImage skips some when it decimates)
  std::vector<uint8_t> used(std::max(t->src_hi - t->src_lo, 0), 0);
  for (size_t o = 0; o < t->start.size(); o++)
    for (int j = 0; j < t->count[o]; j++)
      if (t->w[t->woff[o] + j] != 0.0f) used[t->start[o] + j - t->src_lo] = 1;
  t->touched = 0;
  for (uint8_t u : used) t->touched += u;
}

// ---- ScaleImage contribution lists (resize.c ScaleImage; oracle
// or_im_scale_q16 is the literal loop) ----------------------------------------
void im_scale_rows(int H, int oh, ScaleList *L) {
  *L = ScaleList();
  L->off.push_back(0);
  if (oh == H) {  // rows copied (scanline = x_vector)
    for (int y = 0; y < oh; y++) {
      L->idx.push_back(y);
      L->w.push_back(1.0);
      L->off.push_back((int32_t)L->idx.size());
    }
    return;
  }
  int number_rows = 0, i = 0, cur = -1;
  bool next_row = true;
  double span_y = 1.0, scale_y = (double)oh / (double)H;
  for (int y = 0; y < oh; y++) {
    while (scale_y < span_y) {
      if (next_row && number_rows < H) {
        cur = i++;
        number_rows++;
      }
      L->idx.push_back(cur);
      L->w.push_back(scale_y);
      span_y -= scale_y;
      scale_y = (double)oh / (double)H;
      next_row = true;
    }
    if (next_row && number_rows < H) {
      cur = i++;
      number_rows++;
      next_row = false;
    }
    L->idx.push_back(cur);
    L->w.push_back(span_y);
    L->off.push_back((int32_t)L->idx.size());
    scale_y -= span_y;
    if (scale_y <= 0) {
      scale_y = (double)oh / (double)H;
      next_row = true;
    }
    span_y = 1.0;
  }
}

void im_scale_cols(int W, int ow, ScaleList *L) {
  *L = ScaleList();
  std::vector<std::vector<std::pair<int32_t, double>>> col(ow);
  if (ow == W) {
    for (int x = 0; x < ow; x++) col[x].push_back({x, 1.0});
  } else {
    std::vector<std::pair<int32_t, double>> cur;  // additions to `pixel` since its last reset
    bool next_column = false;
    int t = 0;
    double span_x = 1.0, scale_x = 0;
    for (int x = 0; x < W; x++) {
      scale_x = (double)ow / (double)W;
      while (scale_x >= span_x) {
        if (next_column) {
          cur.clear();
          t++;
        }
        cur.push_back({x, span_x});
        if (t < ow) col[t] = cur;  // scale_scanline[t] = pixel
        scale_x -= span_x;
        span_x = 1.0;
        next_column = true;
      }
      if (scale_x > 0) {
        if (next_column) {
          cur.clear();
          next_column = false;
          t++;
        }
        cur.push_back({x, scale_x});
        span_x -= scale_x;
      }
    }
    if (span_x > 0) cur.push_back({W - 1, span_x});
    if (!next_column && t < ow) col[t] = cur;
  }
  L->off.push_back(0);
  for (int x = 0; x < ow; x++) {
    for (auto &e : col[x]) {
      L->idx.push_back(e.first);
      L->w.push_back(e.second);
    }
    L->off.push_back((int32_t)L->idx.size());
  }
}

int im_percent_size(int size, double percent) { return (int)floor(percent * (double)size / 100.0 + 0.5); }

}  // namespace fi
