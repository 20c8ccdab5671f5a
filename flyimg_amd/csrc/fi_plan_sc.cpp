// fi_plan_sc.cpp -- host planner: the smartcrop side.  Every floating-point
// expression mirrors the reference's evaluation order (built with
// -ffp-contract=off):
//   * Pillow 12.2 Image.thumbnail/resize/reduce (PIL/Image.py:2831-2915,
//     :2328-2470) and Resample.c precompute_coeffs, used by
//     python/smartcrop.py:157-172;
//   * smartcrop.py crop() geometry (:137-191), crops() (:193-229) and
//     importance()/thirds() (:276-298, :30-34);
// and the exact-integer MFMA tables of the prescale kernels (plan_sc_prep) and
// of k_sc_score3 (sc_score_btab).
#include <math.h>

#include <algorithm>
#include <array>
#include <cmath>

#include "fi_plan_frag.h"

namespace fi {

// ---------------------------------------------------------------------------
// Pillow
// ---------------------------------------------------------------------------
static double pil_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
static double pil_lanczos(double x) {
  if (-3.0 <= x && x < 3.0) return pil_sinc(x) * pil_sinc(x / 3);
  return 0.0;
}

int pil_coeffs(int in_size, float in0, float in1, int out_size, std::vector<int32_t> *bounds,
               std::vector<int32_t> *kk) {
  double scale, filterscale;
  filterscale = scale = (double)(in1 - in0) / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 3.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  std::vector<double> k(ksize);
  bounds->assign((size_t)out_size * 2, 0);
  kk->assign((size_t)out_size * ksize, 0);
  for (int xx = 0; xx < out_size; xx++) {
    const double center = in0 + (xx + 0.5) * scale;
    double ww = 0.0;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    int x;
    for (x = 0; x < xmax; x++) {
      const double w = pil_lanczos((x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    for (x = 0; x < xmax; x++)
      if (ww != 0.0) k[x] /= ww;
    for (; x < ksize; x++) k[x] = 0;
    for (x = 0; x < ksize; x++)
      (*kk)[(size_t)xx * ksize + x] =
          k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << 22)) : (int32_t)(0.5 + k[x] * (1 << 22));
    (*bounds)[xx * 2 + 0] = xmin;
    (*bounds)[xx * 2 + 1] = xmax;
  }
  return ksize;
}

// Image.thumbnail preserve_aspect_ratio (PIL/Image.py:2878-2893)
static int pil_thumbnail_size(int W, int H, int x, int y, int *tw, int *th) {
  if (x >= W && y >= H) return 1;
  if (y == 0) return FI_EINVAL;  // ZeroDivisionError in x / y
  const double aspect = (double)W / (double)H;
  if ((double)x / (double)y >= aspect) {
    const double num = y * aspect, f = floor(num), c = ceil(num);
    const double kf = fabs(aspect - f / y), kc = fabs(aspect - c / y);
    const double r = (kc < kf) ? c : f;
    x = r < 1 ? 1 : (int)r;
  } else {
    const double num = x / aspect, f = floor(num), c = ceil(num);
    if (f == 0 && c == 0) {
      y = 1;
    } else {
      const double kf = (f == 0) ? 0 : fabs(aspect - x / f), kc = (c == 0) ? 0 : fabs(aspect - x / c);
      const double r = (kc < kf) ? c : f;
      y = r < 1 ? 1 : (int)r;
    }
  }
  *tw = x;
  *th = y;
  return 0;
}

// ---------------------------------------------------------------------------
// smartcrop.py geometry
// ---------------------------------------------------------------------------
int plan_sc(int W, int H, int width, int height, const fi_smartcrop_options &o, ScPlan *p) {
  *p = ScPlan();
  p->W = W;
  p->H = H;
  auto fail = [&](int code, const char *m) {
    p->status = code;
    p->err = m;
    return code;
  };
  if (W <= 0 || H <= 0 || width <= 0 || height <= 0) return fail(FI_EINVAL, "smartcrop: bad dimensions");
  const double sw = (double)W / width, sh = (double)H / height;
  const double scale = (sh < sw) ? sh : sw;  // min(a, b)
  int cw = (int)floor(width * scale), ch = (int)floor(height * scale);
  double min_scale = o.min_scale;
  {
    const double inv = 1 / scale;
    const double m = (min_scale > inv) ? min_scale : inv;          // max(1/scale, min_scale)
    min_scale = (m < o.max_scale) ? m : o.max_scale;                // min(max_scale, .)
  }
  double pre = 1;
  int aw = W, ah = H;
  if (o.prescale) {
    pre = 1 / scale / min_scale;
    if (pre < 1) {
      const int tx = (int)(W * pre), ty = (int)(H * pre);
      int tw = W, th = H;
      const int r = pil_thumbnail_size(W, H, tx, ty, &tw, &th);
      if (r < 0) return fail(FI_EINVAL, "smartcrop: thumbnail size division by zero");
      if (r == 1) {
        tw = W;
        th = H;
      }
      if (tw != W || th != H) {
        p->thumb = true;
        // Image.resize(reducing_gap=2.0)
        const int fx = (int)((double)W / tw / 2.0), fy = (int)((double)H / th / 2.0);
        p->fx = fx ? fx : 1;
        p->fy = fy ? fy : 1;
        float bx1 = (float)W, by1 = (float)H;
        int iw = W, ih = H;
        if (p->fx > 1 || p->fy > 1) {
          iw = (W + p->fx - 1) / p->fx;
          ih = (H + p->fy - 1) / p->fy;
          bx1 = (float)((double)W / p->fx);
          by1 = (float)((double)H / p->fy);
        }
        p->rw = iw;
        p->rh = ih;
        p->need_h = tw != iw || bx1 != (float)iw;
        p->need_v = th != ih || by1 != (float)ih;
        p->ksh = pil_coeffs(iw, 0.0f, bx1, tw, &p->hb, &p->hk);
        p->ksv = pil_coeffs(ih, 0.0f, by1, th, &p->vb, &p->vk);
        p->ybox_first = p->vb[0];
        const int ybox_last = p->vb[th * 2 - 2] + p->vb[th * 2 - 1];
        if (p->need_h) {
          for (int i = 0; i < th; i++) p->vb[i * 2] -= p->ybox_first;
          p->hrows = ybox_last - p->ybox_first;
        } else {
          p->hrows = 0;
        }
      }
      aw = tw;
      ah = th;
      cw = (int)floor(cw * pre);
      ch = (int)floor(ch * pre);
    } else {
      pre = 1;
    }
  }
  if (!p->thumb) {
    p->rw = W;
    p->rh = H;
  }
  p->prescale = pre;
  p->aw = aw;
  p->ah = ah;
  p->cw = cw;
  p->ch = ch;
  // crops() (smartcrop.py:193-229)
  const int i0 = (int)(o.max_scale * 100), i1 = (int)((min_scale - o.scale_step) * 100);
  const int di = -(int)(o.scale_step * 100);
  if (di >= 0 || o.step <= 0) return fail(FI_EINVAL, "smartcrop: bad scale_step/step");
  for (int i = i0; i > i1; i += di) {
    const double s = i / 100.0;
    for (int y = 0; y < ah; y += o.step) {
      if (!(y + ch * s <= ah)) break;
      for (int x = 0; x < aw; x += o.step) {
        if (!(x + cw * s <= aw)) break;
        CropHost c;
        c.fx = x;
        c.fy = y;
        c.fw = cw * s;
        c.fh = ch * s;
        c.x0 = x;
        c.y0 = y;
        c.nin_x = std::min(aw - x, (int)ceil(x + c.fw) - x);
        c.nin_y = std::min(ah - y, (int)ceil(y + c.fh) - y);
        if (c.nin_x < 0) c.nin_x = 0;
        if (c.nin_y < 0) c.nin_y = 0;
        c.rx = (int32_t)floor(c.fx / pre);
        c.ry = (int32_t)floor(c.fy / pre);
        c.rw = (int32_t)floor(c.fw / pre);
        c.rh = (int32_t)floor(c.fh / pre);
        p->crops.push_back(c);
      }
    }
  }
  if (p->crops.empty()) return fail(FI_ENOCROP, "smartcrop: no crop windows (smartcrop.py:227-228 ValueError)");
  plan_sc_prep(p);
  return FI_OK;
}


// Pillow coefficient of output o at source index s (0 outside its taps)
static int32_t pil_tap(const std::vector<int32_t> &bounds, const std::vector<int32_t> &kk, int ks, int o, int s) {
  const int xmin = bounds[2 * o], cnt = bounds[2 * o + 1];
  return s >= xmin && s < xmin + cnt ? kk[(size_t)o * ks + (s - xmin)] : 0;
}
// first tap and one past the last tap of the outputs [o0, o1)
static void pil_window(const std::vector<int32_t> &bounds, int o0, int o1, int *lo, int *hi) {
  *lo = 1 << 30;
  *hi = 0;
  for (int o = o0; o < o1; o++) {
    *lo = std::min(*lo, bounds[2 * o]);
    *hi = std::max(*hi, bounds[2 * o] + bounds[2 * o + 1]);
  }
}

// k_sc_hrows / k_sc_vmaps launch geometry (fi_sc_prep.hip): row chunks and
// the LDS each needs (transposed H coefficients + staged source rows; staged
// H-stage rows + prescaled rows of an output chunk with its one-row halo).
// Exact-integer MFMA form of Pillow's horizontal pass (k_sc_hmfma): for each
// block of 16 output columns, the banded coefficient matrix over a window of
// 64 * ks source columns, split into three signed-byte limbs
// (k = L0 + 256 L1 + 65536 L2), laid out in the MFMA B-fragment order.
static void plan_sc_hmfma(ScPlan *p, int sw) {
  p->hm_ok = false;
  const int aw = p->aw, nb = (aw + 15) / 16;
  int ks = 1, maxend = sw;
  std::vector<int32_t> s0(nb);
  for (int b = 0; b < nb; b++) {
    int lo, hi;
    pil_window(p->hb, 16 * b, std::min(aw, 16 * b + 16), &lo, &hi);
    s0[b] = lo / 8 * 8;  // fragment reads are two 8-byte LDS reads: 8-B aligned
    ks = std::max(ks, (hi - s0[b] + 63) / 64);
  }
  for (int b = 0; b < nb; b++) maxend = std::max(maxend, s0[b] + 64 * ks);
  const int pitch = (maxend + 15) / 16 * 16;
  int rows = 32;
  while (rows >= 16 && (int64_t)3 * rows * pitch > kHmMaxLds) rows -= 16;
  if (rows < 16 || ks > 2) return;
  p->hm_ks = ks;
  p->hm_pitch = pitch;
  p->hm_rows = rows;
  p->hm_nb = nb;
  p->hm_lds = 3 * rows * pitch;
  p->hm_chunks = (p->hrows + rows - 1) / rows;
  p->hmS0 = s0;
  p->hmC.assign(aw, 0);
  for (int x = 0; x < aw; x++) {
    int64_t sum = 0;
    for (int j = 0; j < p->hb[2 * x + 1]; j++) sum += p->hk[(size_t)x * p->ksh + j];
    p->hmC[x] = (int32_t)((1 << 21) + 128 * sum);
  }
  p->hmB.assign((size_t)nb * ks * 3 * 256, 0);
  for (int b = 0; b < nb; b++)
    for (int t = 0; t < ks; t++)
      fill_frag<3>(p->hmB, (size_t)(b * ks + t) * 3 * 256, [&](int r, int k) {
        return 16 * b + r < aw ? pil_tap(p->hb, p->hk, p->ksh, 16 * b + r, s0[b] + 64 * t + k) : 0;
      });
  p->hm_ok = true;
}

// k_sc_vq tables: per chunk of kVqRows analysed rows, the 16 prescaled rows
// [pa, pa + 16) (pa = y0 - 1 clamped) as one MFMA block over a window of <= 64
// H-stage rows starting at vqK0; coefficients as three signed-byte limbs.
static void plan_sc_vq(ScPlan *p) {
  p->vq_ok = false;
  if (!(p->thumb && p->need_h && p->need_v)) return;
  const int ah = p->ah, chunks = (ah + kVqRows - 1) / kVqRows;
  p->vqC.assign(ah, 0);  // (k_sc_vx's bias too, whether or not k_sc_vq's windows fit)
  for (int y = 0; y < ah; y++) {
    int64_t sum = 0;
    for (int j = 0; j < p->vb[2 * y + 1]; j++) sum += p->vk[(size_t)y * p->ksv + j];
    p->vqC[y] = (int32_t)((1 << 21) + 128 * sum);
  }
  p->vqK0.assign(chunks, 0);
  p->vqA.assign((size_t)chunks * 3 * 256, 0);
  for (int c = 0; c < chunks; c++) {
    const int y0 = kVqRows * c, pa = std::max(0, y0 - 1), pe = std::min(ah, pa + 16);
    const int k0 = p->vb[2 * pa];
    for (int y = pa; y < pe; y++)
      if (p->vb[2 * y] < k0 || p->vb[2 * y] + p->vb[2 * y + 1] - k0 > 64) return;
    p->vqK0[c] = k0;
    fill_frag<3>(p->vqA, (size_t)c * 3 * 256,
                 [&](int r, int k) { return pa + r < pe ? pil_tap(p->vb, p->vk, p->ksv, pa + r, k0 + k) : 0; });
  }
  const int apitch = (p->aw * 3 + 15) / 16 * 16;
  p->vq_lds = 64 * apitch + 16 * apitch + 16 * ((p->aw + 3) / 4 * 4);
  if (p->vq_lds > kPrepMaxLds) return;
  p->vq_chunks = chunks;
  p->vq_ok = true;
}

// k_sc_hx / k_sc_vx tables (fi_plan.h ScPlan::cx_*): per chunk of kVqRows
// analysed rows, the 16 prescaled rows [pa, pa + 16) over the H-stage rows
// [K0, K0 + 64 kv), K0 = the chunk's first tap rounded down to a multiple of 4,
// coefficients as three signed-byte limbs in A-fragment order (row pa + (l & 15),
// K slot mfma_i8_k(l, j) of k-step t).  Needs k_sc_hmfma's horizontal tables.
static void plan_sc_cx(ScPlan *p) {
  p->cx_ok = false;
  p->cxA.clear();
  p->cxK0.clear();
  if (!p->hm_ok || !(p->thumb && p->need_h && p->need_v) || (int)p->vqC.size() != p->ah) return;
  const int ah = p->ah, chunks = (ah + kVqRows - 1) / kVqRows;
  int kv = 1, tp = p->hrows;
  p->cxK0.assign(chunks, 0);
  for (int c = 0; c < chunks; c++) {
    const int y0 = kVqRows * c, pa = std::max(0, y0 - 1), pe = std::min(ah, pa + 16);
    int lo, hi;
    pil_window(p->vb, pa, pe, &lo, &hi);
    p->cxK0[c] = lo & ~3;
    kv = std::max(kv, (hi - p->cxK0[c] + 63) / 64);
  }
  if (kv > 2) return;
  for (int c = 0; c < chunks; c++) tp = std::max(tp, p->cxK0[c] + 64 * kv);
  p->cx_tp = (tp + 15) / 16 * 16 + 16;  // + one row block: the V pass's 16-B reads straddle two
  p->cx_kv = kv;
  p->cxA.assign((size_t)chunks * kv * 3 * 256, 0);
  for (int c = 0; c < chunks; c++) {
    const int y0 = kVqRows * c, pa = std::max(0, y0 - 1), pe = std::min(ah, pa + 16);
    for (int t = 0; t < kv; t++)
      fill_frag<3>(p->cxA, ((size_t)c * kv + t) * 3 * 256, [&](int r, int k) {
        return pa + r < pe ? pil_tap(p->vb, p->vk, p->ksv, pa + r, p->cxK0[c] + 64 * t + k) : 0;
      });
  }
  p->cx_ok = true;
}

void plan_sc_prep(ScPlan *p) {
  p->prep_ok = false;
  p->hkT.clear();
  const bool reduced = p->fx > 1 || p->fy > 1;
  const int sw = reduced ? p->rw : p->W;
  const int64_t apitch = (p->aw * 3 + 15) / 16 * 16, spitch = (sw * 3 + 15) / 16 * 16;
  p->h_chunks = 0;
  p->h_lds = 0;
  if (p->thumb && p->need_h) {
    p->hkT.assign((size_t)p->ksh * p->aw, 0);
    for (int x = 0; x < p->aw; x++)
      for (int j = 0; j < p->ksh; j++) p->hkT[(size_t)j * p->aw + x] = p->hk[(size_t)x * p->ksh + j];
    p->h_chunks = (p->hrows + kPrepRows - 1) / kPrepRows;
    const int64_t lds = ((int64_t)p->ksh * p->aw * 4 + 15) / 16 * 16 + kPrepRows * spitch;
    if (lds > kPrepMaxLds) return;
    p->h_lds = (int)lds;
    plan_sc_hmfma(p, sw);
  }
  p->v_chunks = (p->ah + kPrepRows - 1) / kPrepRows;
  int64_t vmax = 0;
  const bool need_v = p->thumb && p->need_v;
  for (int c = 0; c < p->v_chunks; c++) {
    const int y0 = c * kPrepRows, y1 = std::min(y0 + kPrepRows, p->ah);
    const int pa = std::max(0, y0 - 1), pb = std::min(p->ah, y1 + 1);
    int lo = pa, hi = pb;
    if (need_v) {
      lo = p->vb[2 * pa];
      hi = 0;
      for (int y = pa; y < pb; y++) {
        if (p->vb[2 * y] < lo) return;  // kernel stages from the first row's window start
        hi = std::max(hi, p->vb[2 * y] + p->vb[2 * y + 1]);
      }
    }
    vmax = std::max(vmax, (int64_t)(hi - lo) * apitch + (int64_t)(pb - pa) * apitch);
  }
  if (vmax > kPrepMaxLds) return;
  p->v_lds = (int)vmax;
  p->prep_ok = true;
  plan_sc_vq(p);
  // k_sc_fz: both MFMA passes in one per-image workgroup (no reduce step; the
  // source block's items fit the kernel's 4 register slots per thread)
  p->fz_ok = false;
  if (p->hm_ok && p->vq_ok && !reduced && p->hm_pitch <= 1024) {
    const int64_t lpitch = (p->aw + 3) / 4 * 4;
    const int64_t lds = 80 * apitch + std::max<int64_t>(3 * 16 * (int64_t)p->hm_pitch, 16 * apitch + 16 * lpitch);
    if (lds <= kFzMaxLds) {
      p->fz_lds = (int)lds;
      p->fz_ok = true;
    }
  }
  if (!reduced) plan_sc_cx(p);
}

static double thirds(double x) {
  x = (fmod(x + 2.0 / 3.0, 2.0) * 0.5 - 0.5) * 16;
  const double v = 1 - x * x;
  return (0 > v) ? 0.0 : v;
}

void sc_importance_table(const fi_smartcrop_params &P, double fw, double fh, int nx, int ny,
                         std::vector<double> *out) {
  out->assign((size_t)nx * ny, 0.0);
  for (int dy = 0; dy < ny; dy++)
    for (int dx = 0; dx < nx; dx++) {
      const double xr = dx / fw, yr = dy / fh;
      const double px = fabs(0.5 - xr) * 2, py = fabs(0.5 - yr) * 2;
      double ddx = px - 1 + P.edge_radius, ddy = py - 1 + P.edge_radius;
      if (0 > ddx) ddx = 0;
      if (0 > ddy) ddy = 0;
      const double d = (ddx * ddx + ddy * ddy) * P.edge_weight;
      double s = 1.41 - sqrt(px * px + py * py);
      if (P.rule_of_thirds) {
        double m = s + d + 0.5;
        if (0 > m) m = 0;
        s += (m * 1.2) * (thirds(px) + thirds(py));
      }
      (*out)[(size_t)dy * nx + dx] = s + d;
    }
}


// k_sc_score3's B fragments (fi_internal.h ScGroup, v_mfma_i32_16x16x64_i8:
// lane l holds B[k = mfma_i8_k(l, j)][n = l & 15]).  Column n = digit n % 5 of
// slot n / 5.  Tq is formed exactly: imp 2^q and oi 2^q are doubles scaled by
// a power of two, their difference is exact in long double (|.| < 2^44 with
// no bit below 2^-10), then rounded once, so |Tq 2^-q - (imp - oi)| <= 2^-q-1.
void sc_score_btab(const std::vector<double> &imp, int nx, int ny, double oi, int nslot, int step, ScoreBTab *out) {
  *out = ScoreBTab();
  if (nx <= 0 || ny <= 0 || nslot < 1 || nslot > kSgSlots) return;
  double m = 0;
  for (double v : imp) m = std::max(m, std::fabs(v - oi));
  int q = 38;
  while (q > 0 && std::ldexp(m, q) * (1 + 1e-9) + 1 >= std::ldexp(1.0, 38) * 1.9) q--;
  const int ks = (nx + 63) / 64;
  if (ks > kSgMaxKs) return;
  std::vector<std::array<int8_t, kSgDigits>> dg((size_t)nx * ny);
  for (int v = 0; v < ny; v++)
    for (int u = 0; u < nx; u++) {
      const long double a = (long double)std::ldexp(imp[(size_t)v * nx + u], q);
      const long double b = (long double)std::ldexp(oi, q);
      int64_t d[kSgDigits + 1];  // the digits and what is left above them
      limbs<kSgDigits + 1>((int64_t)std::llrintl(a - b), d);
      for (int i = 0; i < kSgDigits; i++) {
        dg[(size_t)v * nx + u][i] = (int8_t)d[i];
        out->S[i] += (int32_t)d[i];
      }
      if (d[kSgDigits] != 0) return;  // |Tq| beyond five digits (cannot happen with q above)
    }
  out->q = q;
  out->ks = ks;
  out->nrows = ny + step * (nslot - 1);
  out->frag.assign((size_t)out->nrows * ks * 256, 0);
  // one single-limb fragment per row and k-step: the weight of column n at
  // K slot k is that digit of window row r - step * slot, column 64 t + k
  for (int r = 0; r < out->nrows; r++)
    for (int t = 0; t < ks; t++)
      fill_frag<1>(out->frag, ((size_t)r * ks + t) * 256, [&](int n, int k) {
        const int slot = n / kSgDigits, v = r - step * slot, u = 64 * t + k;
        return slot < nslot && v >= 0 && v < ny && u < nx ? dg[(size_t)v * nx + u][n % kSgDigits] : 0;
      });
  out->ok = true;
}

}  // namespace fi
