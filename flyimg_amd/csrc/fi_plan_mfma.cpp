// fi_plan_mfma.cpp -- host planner: weight quantisation of a tap axis
// (fi_plan.cpp build_axis) and the exact-integer MFMA tables of the three
// resample kernels: k_rs_vm (build_mfma_h, build_vm_v), k_rs_vr (build_mfma_h's
// two-limb form, build_vr_v) and k_rs_hv (build_hv_h, build_hv_v).
#include <math.h>

#include <algorithm>

#include "fi_plan_frag.h"

namespace fi {

static int32_t quant_w(float w) { return (int32_t)lrint((double)w * (double)(1 << kMfmaWBits)); }
// W = rint(w * 2^shift) per tap, then per output the |d| taps whose rounding
// residual points furthest the needed way move by one so that sum(W) =
// 2^shift: IM's weights are normalised to sum 1, and a
// quantised row that keeps its sum reproduces a flat region exactly (rounding
// each tap alone leaves a bias that repeats on every output at integral
// factors: 98.5 % exact at 1/10 against 99.98 % with the sum kept)
static void quant_axis(const AxisTable &t, int shift, std::vector<int32_t> *wq) {
  wq->assign(t.w.size(), 0);
  const double sc = (double)(1 << shift);
  std::vector<int> ord;
  for (size_t o = 0; o < t.start.size(); o++) {
    const int n = t.count[o], w0 = t.woff[o];
    int64_t sq = 0;
    for (int j = 0; j < n; j++) {
      (*wq)[w0 + j] = (int32_t)lrint((double)t.w[w0 + j] * sc);
      sq += (*wq)[w0 + j];
    }
    // IM normalises every row to sum 1 (resize.c density): the target is 2^shift,
    // not the float-rounded sum of the float weights
    int64_t d = (n > 0 ? ((int64_t)1 << shift) : 0) - sq;
    if (d == 0) continue;
    const int dir = d > 0 ? 1 : -1;
    ord.clear();
    for (int j = 0; j < n; j++)
      if (t.w[w0 + j] != 0.0f) ord.push_back(j);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
      const double ra = ((double)t.w[w0 + a] * sc - (*wq)[w0 + a]) * dir;
      const double rb = ((double)t.w[w0 + b] * sc - (*wq)[w0 + b]) * dir;
      return ra > rb;
    });
    for (size_t k = 0; d != 0 && !ord.empty(); k = (k + 1) % ord.size(), d -= dir) (*wq)[w0 + ord[k]] += dir;
  }
}
int vr_quant(const AxisTable &t, std::vector<int32_t> *wq) {
  for (int s = kVrMaxShift; s >= kVrMinShift; s--) {
    quant_axis(t, s, wq);
    bool ok = true;
    for (int32_t q : *wq)
      if (q < -32896 || q > 32639) {
        ok = false;
        break;
      }
    if (ok) return s;
  }
  wq->clear();
  return 0;
}

// touched indices (non-zero weight) of an axis, ascending, and their list index
static void touched_list(const AxisTable &t, std::vector<int32_t> *list, std::vector<int32_t> *idx) {
  const int span = std::max(t.src_hi - t.src_lo, 0);
  idx->assign(span, -1);
  for (size_t o = 0; o < t.start.size(); o++)
    for (int j = 0; j < t.count[o]; j++)
      if (t.w[t.woff[o] + j] != 0.0f) (*idx)[t.start[o] + j - t.src_lo] = 1;
  list->clear();
  for (int r = 0; r < span; r++)
    if ((*idx)[r] >= 0) {
      (*idx)[r] = (int32_t)list->size();
      list->push_back(t.src_lo + r);
    }
}
// list-index range [lo, hi] of output o's non-zero taps (lo > hi: none)
static void tap_range(const AxisTable &t, const std::vector<int32_t> &idx, int o, int *lo, int *hi) {
  *lo = 1 << 30;
  *hi = -1;
  for (int j = 0; j < t.count[o]; j++)
    if (t.w[t.woff[o] + j] != 0.0f) {
      const int li = idx[t.start[o] + j - t.src_lo];
      *lo = std::min(*lo, li);
      *hi = std::max(*hi, li);
    }
}
// list-index range [lo, hi] of the taps of the 16-output block b (false: an
// output without taps)
static bool block_tap_range(const AxisTable &t, const std::vector<int32_t> &idx, int b, int *lo, int *hi) {
  *lo = 1 << 30;
  *hi = -1;
  for (int o = 16 * b; o < std::min((int)t.start.size(), 16 * b + 16); o++) {
    int a, e;
    tap_range(t, idx, o, &a, &e);
    if (e < a) return false;
    *lo = std::min(*lo, a);
    *hi = std::max(*hi, e);
  }
  return true;
}
// rstep > 0: rows[k] == row0 + rstep * k; 0: unevenly spaced
static void row_step(const std::vector<int32_t> &rows, int32_t *row0, int32_t *rstep) {
  const int nl = (int)rows.size();
  *row0 = rows[0];
  *rstep = nl > 1 ? rows[1] - rows[0] : 1;
  for (int k = 1; k < nl && *rstep > 0; k++)
    if (rows[k] != *row0 + *rstep * k) *rstep = 0;
}
// The 2^22-scaled weights of k_rs_vm (and k_sc-independent: AxisTable::w
// order): k_rs_vr's two-limb weights (vr_quant, shift s) times 2^(22 - s) when
// the axis has them, else rint(w 2^22).  k_rs_vm's float conversions then see
// k_rs_vr's integer sums times a power of two, so the two kernels give the
// same pixels bit for bit and an image's output does not depend on which of
// them its batch ran (the choice is per batch: classes, ring fit).
int axis_q22(const AxisTable &t, std::vector<int32_t> *q) {
  std::vector<int32_t> wq;
  const int s = vr_quant(t, &wq);
  q->resize(t.w.size());
  for (size_t i = 0; i < t.w.size(); i++) (*q)[i] = s > 0 ? wq[i] * (1 << (kMfmaWBits - s)) : quant_w(t.w[i]);
  return s > 0 ? s : kMfmaWBits;
}
// quantized weight (wq: AxisTable::w order) of output o at list index li (0 if not a tap)
static int32_t tap_w(const AxisTable &t, const std::vector<int32_t> &wq, const std::vector<int32_t> &list, int o,
                     int li) {
  if (li < 0 || li >= (int)list.size()) return 0;
  const int j = list[li] - t.start[o];
  if (j < 0 || j >= t.count[o]) return 0;
  return wq[t.woff[o] + j];
}

bool build_mfma_h(const AxisTable &h, MfmaH *m, int max_nx) {
  *m = MfmaH();
  const int nx = (int)h.start.size();
  if (nx == 0) return false;
  std::vector<int32_t> idx;
  touched_list(h, &m->cols, &idx);
  std::vector<int32_t> lo(nx), hi(nx);
  for (int x = 0; x < nx; x++) {
    tap_range(h, idx, x, &lo[x], &hi[x]);
    if (hi[x] < lo[x]) return false;  // an output px without taps
    if (x > 0 && (lo[x] < lo[x - 1] || hi[x] < hi[x - 1])) return false;  // not monotone
  }
  std::vector<int32_t> q22;
  axis_q22(h, &q22);
  m->wsum.assign(nx, 0);
  for (int x = 0; x < nx; x++)
    for (int j = 0; j < h.count[x]; j++) m->wsum[x] += q22[h.woff[x] + j];
  std::vector<int32_t> wq2;
  m->shift2 = vr_quant(h, &wq2);
  m->wsum2.assign(nx, 0);
  if (m->shift2 > 0)
    for (int x = 0; x < nx; x++)
      for (int j = 0; j < h.count[x]; j++) m->wsum2[x] += wq2[h.woff[x] + j];
  auto bytes_of = [&](int x0, int x1, int *b0) {
    *b0 = (3 * m->cols[lo[x0]]) / 16 * 16;
    const int be = (3 * (m->cols[hi[x1 - 1]] + 1) + 15) / 16 * 16;
    return be - *b0;
  };
  for (int x0 = 0; x0 < nx;) {
    int x1 = x0 + 1, b0;
    if (bytes_of(x0, x1, &b0) > kMfmaStripBytes) return false;
    while (x1 < nx && x1 - x0 < max_nx && bytes_of(x0, x1 + 1, &b0) <= kMfmaStripBytes) x1++;
    // strips end on multiples of 4 px (the last one at nx): every strip's output
    // segment then starts 12-byte aligned in its row, so with a dword-aligned
    // destination row the stores are whole dwords / 8-byte units, no byte stores
    if (x1 < nx && (x1 & ~3) > x0) x1 &= ~3;
    MfmaStrip S{};
    S.x0 = x0;
    S.x1 = x1;
    S.nbytes = bytes_of(x0, x1, &S.b0);
    S.c_lo = lo[x0];
    S.ncols = hi[x1 - 1] + 1 - S.c_lo;
    S.nocb = (x1 - x0 + 15) / 16;
    S.ks = 1;
    S.s0 = m->s0.size();
    // per 16-px output block: window start (8-B aligned for the two 8-byte
    // fragment reads) and its own k-steps; s0 holds (w0, ks) pairs
    int pitch = S.ncols;
    for (int ob = 0; ob < S.nocb; ob++) {
      const int xa = x0 + 16 * ob, xb = std::min(x1, xa + 16);
      const int w0 = (lo[xa] - S.c_lo) / 8 * 8;
      const int ks = (hi[xb - 1] - S.c_lo + 1 - w0 + 63) / 64;
      S.ks = std::max(S.ks, ks);
      m->s0.push_back(w0);
      m->s0.push_back(ks);
      pitch = std::max(pitch, w0 + 64 * ks);
    }
    if (S.ks > 2) return false;
    // plane pitch = 8 (mod 32) bytes: the fold's byte writes of rows 4 apart and the
    // fragment reads of rows 1 apart spread over the LDS banks
    S.pitch = pitch + ((8 - pitch % 32) + 32) % 32;
    if (S.pitch > kMfmaMaxPitch) return false;
    S.vpitch = (pitch + 15) / 16 * 16;
    S.lut_px0 = S.b0 / 3;
    S.lut_n = (S.b0 + S.nbytes + 2) / 3 - S.lut_px0;
    S.lut = m->lut.size();
    for (int k = 0; k < S.lut_n; k++) {
      const int px = S.lut_px0 + k;
      int ci = -1;
      if (px >= h.src_lo && px < h.src_hi && idx[px - h.src_lo] >= 0) ci = idx[px - h.src_lo] - S.c_lo;
      m->lut.push_back(ci >= 0 && ci < S.ncols ? ci : -1);
    }
    while (m->lut.size() % 4) m->lut.push_back(-1);  // 16-byte rows: k_rs_vr stages the LUT by LDS-DMA
    S.frag = m->frag.size();
    m->frag.resize(m->frag.size() + (size_t)S.nocb * S.ks * 3 * 256, 0);
    S.frag2 = m->frag2.size();
    if (m->shift2 > 0) m->frag2.resize(m->frag2.size() + (size_t)S.nocb * S.ks * 2 * 256, 0);
    for (int ob = 0; ob < S.nocb; ob++)
      for (int t = 0; t < S.ks; t++) {
        const int xa = x0 + 16 * ob, li0 = S.c_lo + m->s0[S.s0 + 2 * ob] + 64 * t;
        fill_frag<3>(m->frag, S.frag + (size_t)(ob * S.ks + t) * 3 * 256,
                     [&](int r, int k) { return xa + r < x1 ? tap_w(h, q22, m->cols, xa + r, li0 + k) : 0; });
        if (m->shift2 > 0)
          fill_frag<2>(m->frag2, S.frag2 + (size_t)(ob * S.ks + t) * 2 * 256,
                       [&](int r, int k) { return xa + r < x1 ? tap_w(h, wq2, m->cols, xa + r, li0 + k) : 0; });
      }
    m->strips.push_back(S);
    x0 = x1;
  }
  return true;
}

bool build_vm_v(const AxisTable &v, VmV *m) {
  *m = VmV();
  const int ny = (int)v.start.size();
  if (ny == 0) return false;
  std::vector<int32_t> q22;
  axis_q22(v, &q22);
  std::vector<int32_t> idx;
  touched_list(v, &m->rows, &idx);
  const int nl = (int)m->rows.size();
  if (nl == 0) return false;
  m->nblk = (ny + 15) / 16;
  std::vector<int> L(m->nblk), R(m->nblk);
  for (int b = 0; b < m->nblk; b++) {
    int hi;
    if (!block_tap_range(v, idx, b, &L[b], &hi)) return false;  // an output row without taps
    R[b] = hi + 1;
    if (b > 0 && (L[b] < L[b - 1] || R[b] < R[b - 1])) return false;  // not monotone
  }
  // pieces: block b owns [R(b-1), R(b)), R(-1) = L(0)
  std::vector<int> pstart(m->nblk + 1);  // first piece of block b
  for (int b = 0; b < m->nblk; b++) {
    pstart[b] = (int)m->plo.size();
    const int a = b == 0 ? L[0] : R[b - 1], e = R[b];
    // the taps of block b must lie in the pieces of blocks b - 1 and b
    const int own_lo = b == 0 ? L[0] : (b == 1 ? L[0] : R[b - 2]);
    if (L[b] < own_lo) return false;
    int k = a;
    do {
      const int n = std::min(64, e - k);
      m->plo.push_back(k);
      m->pn.push_back(std::max(n, 0));
      m->pblk.push_back(b);
      m->plast.push_back(0);
      k += std::max(n, 0);
    } while (k < e);
    m->plast.back() = 1;
  }
  pstart[m->nblk] = (int)m->plo.size();
  const int np = (int)m->plo.size();
  m->frag.assign((size_t)np * 6 * 256, 0);
  for (int p = 0; p < np; p++)
    for (int s = 0; s < 2; s++) {
      const int bb = m->pblk[p] + s;
      if (bb >= m->nblk) continue;
      fill_frag<3>(m->frag, (size_t)(p * 2 + s) * 3 * 256, [&](int r, int k) {
        const int y = 16 * bb + r;
        return y < ny && k < m->pn[p] ? tap_w(v, q22, m->rows, y, m->plo[p] + k) : 0;
      });
    }
  // every tap is covered exactly once by (its block's pieces) U (previous block's pieces)
  for (int y = 0; y < ny; y++) {
    const int b = y / 16;
    const int lo_list = b == 0 ? L[0] : m->plo[pstart[b - 1]];
    for (int j = 0; j < v.count[y]; j++) {
      if (v.w[v.woff[y] + j] == 0.0f) continue;
      const int li = idx[v.start[y] + j - v.src_lo];
      if (li < lo_list || li >= R[b]) return false;
    }
  }
  m->w128.assign((size_t)16 * (m->nblk + 2), 0);  // two zero blocks: k_rs_vm loads block b + 2 unconditionally
  for (int y = 0; y < ny; y++)
    for (int j = 0; j < v.count[y]; j++) m->w128[y] += 128 * q22[v.woff[y] + j];
  row_step(m->rows, &m->row0, &m->rstep);
  return true;
}

bool build_vr_v(const AxisTable &v, VrV *m) {
  *m = VrV();
  const int ny = (int)v.start.size();
  if (ny == 0) return false;
  std::vector<int32_t> idx;
  touched_list(v, &m->rows, &idx);
  const int nl = (int)m->rows.size();
  if (nl == 0) return false;
  m->nblk = (ny + 15) / 16;
  std::vector<int32_t> wq;
  m->shift = vr_quant(v, &wq);
  if (m->shift == 0) return false;
  m->frag.assign((size_t)m->nblk * 4 * 256, 0);
  m->w128.assign((size_t)16 * m->nblk, 0);
  int pK0 = 0, pR = 0;
  for (int b = 0; b < m->nblk; b++) {
    int lo, hi;
    if (!block_tap_range(v, idx, b, &lo, &hi)) return false;  // an output row without taps
    const int K0 = lo / 16 * 16, R = hi + 1;
    const int ks = (R - K0 + 63) / 64;
    if (ks > 2) return false;
    if (b > 0 && (K0 < pK0 || R < pR)) return false;  // not monotone
    pK0 = K0;
    pR = R;
    m->bmeta.insert(m->bmeta.end(), {K0, ks, R, 0});
    for (int t = 0; t < ks; t++)
      fill_frag<2>(m->frag, (size_t)(b * 2 + t) * 2 * 256, [&](int r, int k) {
        return 16 * b + r < ny ? tap_w(v, wq, m->rows, 16 * b + r, K0 + 64 * t + k) : 0;
      });
  }
  for (int y = 0; y < ny; y++)
    for (int j = 0; j < v.count[y]; j++) m->w128[y] += 128 * wq[v.woff[y] + j];
  // k_rs_vr's MFMA bias is the constant 128 * 2^shift: every row must sum to 2^shift
  for (int y = 0; y < ny; y++)
    if (m->w128[y] != (128 << m->shift)) return false;
  row_step(m->rows, &m->row0, &m->rstep);
  // unevenly spaced rows (ThumbnailImage sampling, e.g. cfg1's 2000 -> 1250)
  // stream from the touched-row list (fi_vr.hip issue_rows)
  for (int k = 1; k < nl; k++) m->maxgap = std::max(m->maxgap, m->rows[k] - m->rows[k - 1]);
  return true;
}

// source-index range [a, e] of output o's non-zero taps (false: none)
static bool src_range(const AxisTable &t, int o, int *a, int *e) {
  *a = 1 << 30;
  *e = -1;
  for (int j = 0; j < t.count[o]; j++)
    if (t.w[t.woff[o] + j] != 0.0f) {
      *a = std::min(*a, t.start[o] + j);
      *e = std::max(*e, t.start[o] + j);
    }
  return *e >= *a;
}
// quantized weight of output o at source index s (0 if not a tap)
static int32_t tap_w_src(const AxisTable &t, int o, int s) {
  const int j = s - t.start[o];
  return (j < 0 || j >= t.count[o]) ? 0 : quant_w(t.w[t.woff[o] + j]);
}
// per-output tap ranges, monotone in o (false otherwise)
static bool monotone_ranges(const AxisTable &t, std::vector<int> *lo, std::vector<int> *hi) {
  const int n = (int)t.start.size();
  lo->resize(n);
  hi->resize(n);
  for (int o = 0; o < n; o++) {
    if (!src_range(t, o, &(*lo)[o], &(*hi)[o])) return false;
    if (o > 0 && ((*lo)[o] < (*lo)[o - 1] || (*hi)[o] < (*hi)[o - 1])) return false;
  }
  return true;
}

bool build_hv_h(const AxisTable &h, HvH *m) {
  *m = HvH();
  const int nx = (int)h.start.size();
  std::vector<int> lo, hi;
  if (nx == 0 || !monotone_ranges(h, &lo, &hi)) return false;
  m->w128.assign(nx, 0);
  for (int x = 0; x < nx; x++)
    for (int j = 0; j < h.count[x]; j++) m->w128[x] += 128 * quant_w(h.w[h.woff[x] + j]);
  m->col0 = lo[0];
  // strip [x0, x1): window starts / k-steps per 16-px block (false: a block
  // needs more than 2 k-steps or the window more than kHvMaxPP px)
  auto try_strip = [&](int x0, int x1, HvStrip *S, std::vector<int32_t> *s0) {
    S->x0 = x0;
    S->x1 = x1;
    S->px0 = lo[x0] / 16 * 16;
    S->nocb = (x1 - x0 + 15) / 16;
    int pp = 0;
    s0->clear();
    for (int ob = 0; ob < S->nocb; ob++) {
      const int xa = x0 + 16 * ob, xb = std::min(x1, xa + 16);
      const int w0 = (lo[xa] - S->px0) / 8 * 8;
      const int ks = (hi[xb - 1] + 1 - S->px0 - w0 + 63) / 64;
      if (ks > 2) return false;
      s0->push_back(w0);
      s0->push_back(ks);
      pp = std::max(pp, w0 + 64 * ks);
    }
    S->pp = (pp + 15) / 16 * 16;
    return S->pp <= kHvMaxPP;
  };
  for (int x0 = 0; x0 < nx;) {
    HvStrip S{};
    std::vector<int32_t> s0;
    int x1 = std::min(nx, x0 + kHvMaxNx);
    while (!try_strip(x0, x1, &S, &s0)) {
      if (x1 - x0 <= 16) return false;
      x1 = x0 + (x1 - x0 - 1) / 16 * 16;
    }
    S.s0 = m->s0.size();
    m->s0.insert(m->s0.end(), s0.begin(), s0.end());
    S.frag = m->frag.size();
    m->frag.resize(m->frag.size() + (size_t)S.nocb * 2 * 3 * 256, 0);
    for (int ob = 0; ob < S.nocb; ob++)
      for (int t = 0; t < s0[2 * ob + 1]; t++)  // (zero past the block's k-steps)
        fill_frag<3>(m->frag, S.frag + (size_t)(ob * 2 + t) * 3 * 256, [&](int r, int k) {
          const int x = x0 + 16 * ob + r;
          return x < x1 ? tap_w_src(h, x, S.px0 + s0[2 * ob] + 64 * t + k) : 0;
        });
    m->strips.push_back(S);
    x0 = x1;
  }
  return true;
}

bool build_hv_v(const AxisTable &v, HvV *m) {
  *m = HvV();
  const int ny = (int)v.start.size();
  std::vector<int> lo, hi;
  if (ny == 0 || !monotone_ranges(v, &lo, &hi)) return false;
  m->row0 = lo[0];
  m->nrows = hi[ny - 1] + 1 - m->row0;
  m->nblk = (ny + 15) / 16;
  m->frag.assign((size_t)m->nblk * 2 * 3 * 256, 0);
  m->wsum.assign((size_t)16 * m->nblk, 0);
  for (int b = 0; b < m->nblk; b++) {
    const int ye = std::min(ny, 16 * b + 16);
    const int K0 = lo[16 * b] - m->row0;
    const int ks = (hi[ye - 1] + 1 - m->row0 - K0 + 63) / 64;
    if (ks > 2) return false;
    m->k0ks.push_back(K0);
    m->k0ks.push_back(ks);
    for (int t = 0; t < ks; t++)
      fill_frag<3>(m->frag, (size_t)(b * 2 + t) * 3 * 256, [&](int r, int k) {
        return 16 * b + r < ny ? tap_w_src(v, 16 * b + r, m->row0 + K0 + 64 * t + k) : 0;
      });
  }
  for (int y = 0; y < ny; y++)
    for (int j = 0; j < v.count[y]; j++) m->wsum[y] += quant_w(v.w[v.woff[y] + j]);
  return true;
}

}  // namespace fi
