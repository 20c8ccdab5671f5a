// fi_sc_score.hip -- smartcrop.py's saliency stage, part 2: every crop's score
// and the argmax, one workgroup per image, from the maps of fi_sc_prep.hip.
//
//   k_sc_score2   every crop's score (smartcrop.py:300-338) + the argmax
//                 (:116-133), maps resident in LDS: fast f64 pass with a
//                 rigorous error bound, exact sequential re-score of the
//                 crops whose interval reaches the best lower bound.
//   k_sc_score3   the same with the fast pass as exact-integer MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fi_internal.h"
#include "fi_sc_device.h"

namespace fi {

constexpr int kScoreThreads = 1024;
constexpr int kScoreWaves = kScoreThreads / 64;
#ifndef FI_SC_BANDS
#define FI_SC_BANDS 0
#endif
constexpr bool kScoreBands = FI_SC_BANDS;

// MODE 0: maps read from global memory; 1: maps in LDS.
template <int MODE>
__global__ __launch_bounds__(kScoreThreads) void k_sc_score2(const ScDesc *__restrict__ descs,
                                                             const DevCrop *__restrict__ crops,
                                                             const double *__restrict__ ad,
                                                             CropScore *__restrict__ scores,
                                                             ScResult *__restrict__ results, const ScParamsDev P,
                                                             const int32_t *__restrict__ ai) {
  constexpr bool LDS_MAPS = MODE >= 1;
  extern __shared__ __attribute__((aligned(16))) uint32_t smaps[];
  __shared__ double lut[256];
  __shared__ double part[kScoreWaves][3];
  __shared__ double T[3];
  __shared__ double s_tot[kScoreMaxCrops];
  __shared__ double s_bnd[kScoreMaxCrops];
  __shared__ int32_t cand[kScoreMaxCrops];
  __shared__ double s_part[kScoreMaxCrops][3];  // band partial sums (crop-major)
  __shared__ int32_t ncand_s, first_cand_s;
  const ScDesc &D = descs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncrops = D.ncrops;
  // more crops than the LDS arrays hold (analysed images beyond ~14:1, or a
  // small step): totals, bounds and the candidate marks live in the image's
  // CropScore slots instead (exact = 2 marks a candidate until re-scored)
  const bool big = ncrops > kScoreMaxCrops;
  CropScore *const sco = scores + D.score0;
  const int W = D.aw, H = D.ah, npx = W * H;
  const uint32_t *maps = D.maps;
  if (LDS_MAPS) {
    const uint4 *g = reinterpret_cast<const uint4 *>(D.maps);
    for (int k = tid; k < (npx >> 2); k += kScoreThreads) reinterpret_cast<uint4 *>(smaps)[k] = g[k];
    for (int k = (npx & ~3) + tid; k < npx; k += kScoreThreads) smaps[k] = D.maps[k];
    maps = smaps;
  }
  if (tid < 256) lut[tid] = (double)tid / 255.0;  // Python int / 255 (correctly rounded)
  __syncthreads();
  const double sb = P.skin_bias, tb = P.saturation_bias, oi = P.outside_importance;
  // image totals of the three per-pixel terms (the outside part of every crop)
  {
    double t0 = 0, t1 = 0, t2 = 0;
    for (int p = tid; p < npx; p += kScoreThreads) {
      const uint32_t m = maps[p];
      const double d = lut[(m >> 8) & 255];
      t0 += d;
      t1 += lut[m & 255] * (d + sb);
      t2 += lut[(m >> 16) & 255] * (d + tb);
    }
    t0 = wave_sum(t0);
    t1 = wave_sum(t1);
    t2 = wave_sum(t2);
    if (lane == 0) {
      part[wave][0] = t0;
      part[wave][1] = t1;
      part[wave][2] = t2;
    }
    __syncthreads();
    if (tid < 3) {
      double s = 0;
      for (int w = 0; w < kScoreWaves; w++) s += part[w][tid];
      T[tid] = s;
    }
    __syncthreads();
  }
  const double u = 1.1102230246251565e-16;  // 2^-53
  const double nn = (double)npx + 1.0;
  const double aoi = fabs(oi);
  const double wd = P.detail_weight, ws = P.skin_weight, wt = P.saturation_weight;

  // ---- fast pass: one wave per (crop, band of the window's rows), lanes
  // across the window's columns.  Bands (FI_SC_BANDS=1) balance the waves
  // when the crops are few (cfg2: 37 crops -> 74 items on 16 waves, not 3
  // rounds of 16 / 16 / 5) but measured slower (0.40 vs 0.37 ms per cfg2
  // step: per-item reductions), so the default is one band per crop.
  // F = sum_in (imp - oi) a + oi * total(a): the outside pixels need no pass,
  // the inside ones weigh by the table of fl(importance - oi) -- 7 f64
  // operations per (crop, pixel) instead of 10
  auto finalize = [&](int c, double sd, double ss, double st) {
    const DevCrop &cr = crops[D.crop0 + c];
    const double Fd = sd + oi * T[0], Fs = ss + oi * T[1], Ft = st + oi * T[2];
    // |python_sum - F| <= 6 gamma(n+4) (imax + imax2 + |oi|) total(a), a >= 0 (biases
    // >= 0, host-checked): python's sequential sum (5 gamma(n+1) sum |imp a|) plus
    // this pass (fl(imp - oi), one FMA per term, <= nin_y + 16 additions deep
    // with the band and wave reductions)
    const double g4 = (nn + 3.0) * u / (1.0 - (nn + 3.0) * u);
    const double kb = 6.0 * g4 * (cr.imax + cr.imax2 + aoi) * 1.0000001;
    const double Ed = kb * T[0], Es = kb * T[1], Et = kb * T[2];
    const double area = cr.fw * cr.fh;
    const double tot = (Fd * wd + Fs * ws + Ft * wt) / area;
    const double mag = fabs(wd) * (fabs(Fd) + Ed) + fabs(ws) * (fabs(Fs) + Es) + fabs(wt) * (fabs(Ft) + Et);
    const double B = ((fabs(wd) * Ed + fabs(ws) * Es + fabs(wt) * Et) * (1.0 + 16.0 * u) + 16.0 * u * mag) /
                     area * 1.01;
    if (!big) {
      s_tot[c] = tot;
      s_bnd[c] = B;
    }
    CropScore &o = sco[c];
    o.detail = Fd;
    o.saturation = Ft;
    o.skin = Fs;
    o.total = tot;
    o.bound = B;
    o.exact = 0;
  };
  const int nbands = big || !kScoreBands ? 1 : max(1, min(min(8, kScoreMaxCrops / ncrops), (4 * kScoreWaves + ncrops - 1) / ncrops));
  const int nitems = ncrops * nbands;
  for (int item = __builtin_amdgcn_readfirstlane(wave); item < nitems; item += kScoreWaves) {
    const int c = item / nbands, band = item - c * nbands;
    const DevCrop cr = crops[D.crop0 + c];
    const int bh = (cr.nin_y + nbands - 1) / nbands;
    const int ya = min(cr.nin_y, band * bh), yb = min(cr.nin_y, ya + bh);
    const int t2w = cr.table2_w;
    const __amdgpu_buffer_rsrc_t trs =
        __builtin_amdgcn_make_buffer_rsrc((void *)(ad + cr.table2), (short)0, cr.nin_y * t2w * 8, 0x00020000);
    double sd = 0, ss = 0, st = 0;
    auto row_terms = [&](uint32_t m, double imp) {
      const double d = lut[(m >> 8) & 255];
      const double a1 = lut[m & 255] * (d + sb);
      const double a2 = lut[(m >> 16) & 255] * (d + tb);
      sd = fma(imp, d, sd);
      ss = fma(imp, a1, ss);
      st = fma(imp, a2, st);
    };
    for (int dx0 = 0; dx0 < cr.nin_x; dx0 += 64) {
      const int dx = dx0 + lane;
      // LDS maps: lanes past the window read whatever lies there (finite
      // terms) and weigh it by the table's zero padding, so no lane test and
      // the table rows load by scalar base + lane offset; global maps keep
      // the column clamp (the read must stay inside the buffer)
      const bool act = LDS_MAPS || dx < cr.nin_x;
      const int dxc = act ? dx : 0;
      const uint32_t *mcol = maps + (int64_t)cr.y0 * W + cr.x0 + dxc;
      // table row r, column dxc: buffer load, row offset in an SGPR
      auto tload = [&](int r) {
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(trs, 8u * (uint32_t)dxc,
                                                                               (uint32_t)(r * t2w * 8), 0));
      };
      // rows in groups of 4: the four map words, then the four table values,
      // go out together (a conditional read put an exec-masked block and a
      // full LDS wait between consecutive rows)
      int dy = ya;
#pragma unroll 1
      for (; dy + 4 <= yb; dy += 4) {
        uint32_t m[4];
        double imp[4];
#pragma unroll
        for (int u = 0; u < 4; u++) m[u] = mcol[(dy + u) * W];
#pragma unroll
        for (int u = 0; u < 4; u++) imp[u] = tload(dy + u);
#pragma unroll
        for (int u = 0; u < 4; u++) row_terms(act ? m[u] : 0u, imp[u]);  // m = 0: every term is 0
      }
#pragma unroll 1
      for (; dy < yb; dy++) {
        const uint32_t m = mcol[dy * W];
        row_terms(act ? m : 0u, tload(dy));
      }
    }
    sd = wave_sum(sd);
    ss = wave_sum(ss);
    st = wave_sum(st);
    if (lane == 0) {
      if (nbands == 1) {
        finalize(c, sd, ss, st);
      } else {
        s_part[item][0] = sd;
        s_part[item][1] = ss;
        s_part[item][2] = st;
      }
    }
  }
  if (nbands > 1) {
    __syncthreads();
    for (int c = tid; c < ncrops; c += kScoreThreads) {
      double sd = 0, ss = 0, st = 0;  // bands in order: deterministic
      for (int k = 0; k < nbands; k++) {
        sd += s_part[c * nbands + k][0];
        ss += s_part[c * nbands + k][1];
        st += s_part[c * nbands + k][2];
      }
      finalize(c, sd, ss, st);
    }
  }
  __syncthreads();
  // candidates: every crop whose interval reaches the best lower bound
  auto tot_of = [&](int c) { return big ? sco[c].total : s_tot[c]; };
  auto bnd_of = [&](int c) { return big ? sco[c].bound : s_bnd[c]; };
  if (tid == 0) {
    double best_lo = -1.0e308;
    for (int c = 0; c < ncrops; c++) best_lo = fmax(best_lo, tot_of(c) - bnd_of(c));
    int k = 0, first = -1;
    for (int c = 0; c < ncrops; c++)
      if (D.exact_all || tot_of(c) + bnd_of(c) >= best_lo) {
        if (first < 0) first = c;
        if (big)
          sco[c].exact = 2;
        else
          cand[k] = c;
        k++;
      }
    ncand_s = k;
    first_cand_s = first;
  }
  __syncthreads();
  const int ncand = ncand_s;
  const bool need_exact = D.exact_all || ncand > 1;
  if (need_exact) {
    // exact re-score: one lane per candidate, the reference's row-major order
    for (int k = tid; k < (big ? ncrops : ncand); k += kScoreThreads) {
      if (big && sco[k].exact != 2) continue;
      const int c = big ? k : cand[k];
      const DevCrop cr = crops[D.crop0 + c];
      const double *tab = ad + cr.table;
      double skin = 0, detail = 0, sat = 0;
      for (int y = 0; y < H; y++) {
        const bool yin = y >= cr.y0 && y < cr.y0 + cr.nin_y;
        const uint32_t *mrow = maps + (int64_t)y * W;
        const int64_t trow = (int64_t)(y - cr.y0) * cr.table_w - cr.x0;
#pragma unroll 4
        for (int x = 0; x < W; x++) {
          const bool in = yin && x >= cr.x0 && x < cr.x0 + cr.nin_x;
          const double tv = tab[in ? trow + x : 0];
          const double imp = in ? tv : oi;
          const uint32_t m = mrow[x];
          const double det = lut[(m >> 8) & 255];
          skin = skin + lut[m & 255] * (det + sb) * imp;
          detail = detail + det * imp;
          sat = sat + lut[(m >> 16) & 255] * (det + tb) * imp;
        }
      }
      const double tot = (detail * wd + skin * ws + sat * wt) / (cr.fw * cr.fh);
      if (!big) s_tot[c] = tot;
      CropScore &o = sco[c];
      o.detail = detail;
      o.saturation = sat;
      o.skin = skin;
      o.total = tot;
      o.bound = 0;
      o.exact = 1;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int top = first_cand_s;
    double best = tot_of(top);
    if (need_exact) {
      best = -9223372036854775807.0;  // -sys.maxsize; strict > keeps the first max
      // candidates in crop order (the re-scored ones carry exact = 1)
      for (int k = 0; k < (big ? ncrops : ncand); k++) {
        const int c = big ? k : cand[k];
        if (big && sco[c].exact != 1) continue;
        const double v = tot_of(c);
        if (v > best) {
          best = v;
          top = c;
        }
      }
    }
    if (big && !need_exact) sco[top].exact = 0;  // the one candidate's mark (fast score kept)
    results[D.result].top = top;
    results[D.result].n_candidates = ncand;
    results[D.result].total = best;
  }
}

// ---------------------------------------------------------------------------
// k_sc_score3: k_sc_score2's fast pass as exact-integer MFMA (fi_internal.h
// ScGroup).  One 16-wave workgroup per image:
//   1. the maps -> seven signed-byte planes in LDS (edge, skin, sat and the
//      low / high bytes of skin * edge, sat * edge, each as value - 128) and
//      the f64 image totals of the three terms (the outside part);
//   2. the waves take the groups' rows r = wave, wave + 16, ...: per 64-px
//      k-step, the B fragment (digits of Tq over that row segment, one per
//      y slot) from the host table, and per plane one MFMA whose A rows are
//      the 16 x origins' 64 pixels -- D[plane][x origin][digit, slot] sums
//      sum_window Tq_digit (value - 128) exactly in int32;
//   3. cross-wave sums in LDS (the planes are dead), then per crop
//        sum_in Tq x = sum_digit 256^digit D + 128 sum_window Tq
//      for x = edge, skin, sat, skin * edge, sat * edge, and the three terms
//        detail     = 2^-q sum Tq e / 255
//        skin       = 2^-q (sum Tq s e / 65025 + skin_bias sum Tq s / 255)
//        saturation = 2^-q (sum Tq t e / 65025 + sat_bias sum Tq t / 255)
//      are the exact-real sums of (importance - oi) a over the window, up to
//      the quantisation of Tq; F = that + oi total(a) as in k_sc_score2;
//   4. the rigorous bound, candidates, the exact sequential re-score and the
//      argmax exactly as k_sc_score2 (maps reloaded into LDS when needed).
// Bound per term (a >= 0: biases >= 0, host-checked):
//   |python - F| <= [2 gamma(n+5) (imax + |oi|) + 2^-(q+1) + |oi| gamma(n+16)]
//                   total(a) (1 + gamma(n+16)) + gamma(24) |F|_abs
// python's per-term roundings and sequential sum, the rint of Tq, the f64
// image totals (from exact integer sums), and the f64 combination of the integer sums (its absolute
// value carried alongside).
constexpr int kS3Threads = 1024;
constexpr int kS3Waves = kS3Threads / 64;
constexpr int kS3Pre = 8;  // plane items per thread with their map loads in flight together
#ifndef FI_S3_ABL
#define FI_S3_ABL 0
#endif
constexpr int kS3Abl = FI_S3_ABL;  // profiling ablations (wrong scores): 1 no MFMA pass, 2 no plane build, 4 no finalize

__global__ __launch_bounds__(kS3Threads) void k_sc_score3(const ScDesc *__restrict__ descs,
                                                          const DevCrop *__restrict__ crops,
                                                          const ScGroup *__restrict__ groups,
                                                          const double *__restrict__ ad,
                                                          CropScore *__restrict__ scores,
                                                          ScResult *__restrict__ results, const ScParamsDev P,
                                                          const int32_t *__restrict__ ai) {
  typedef __attribute__((address_space(3))) const i32x2 l_ci32x2;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds3[];
  __shared__ double lut[256];
  __shared__ uint32_t ipart[kS3Waves][5];
  __shared__ double T[3];
  __shared__ double s_tot[kSgMaxCrops];
  __shared__ double s_bnd[kSgMaxCrops];
  __shared__ int32_t cand[kSgMaxCrops];
  __shared__ int32_t ncand_s, first_cand_s;
  const ScDesc &D = descs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncrops = D.ncrops;
  CropScore *const sco = scores + D.score0;
  const int W = D.aw, H = D.ah, npx = W * H;
  const int pitch = sg_pitch(W), psz = H * pitch;
  const int ng = D.ngrp;
  const ScGroup *G = groups + D.sg0;
  const double sb = P.skin_bias, tb = P.saturation_bias, oi = P.outside_importance;
  if (tid < 256) lut[tid] = (double)tid / 255.0;  // Python int / 255 (correctly rounded)
  __syncthreads();
  // ---- 1. planes + image totals ----
  // items (row, 4-pixel quad), kS3Pre per thread with every map load in flight
  // before the first is used; the totals as exact integer sums (sum e, s, t,
  // s e, t e) turned into the three f64 terms at the end (|error| <= 3 u T)
  {
    const int nq = (W + 3) >> 2, nit = H * nq;
    uint32_t se_s = 0, te_s = 0, e_s = 0, s_s = 0, t_s = 0;
#pragma unroll 1
    for (int base = 0; base < ((kS3Abl & 2) ? 0 : nit); base += kS3Pre * kS3Threads) {
      uint32_t mm[kS3Pre][4];
#pragma unroll
      for (int j = 0; j < kS3Pre; j++) {
        const int it = base + tid + j * kS3Threads;
        const int y = it / nq, x = 4 * (it - y * nq);
#pragma unroll
        for (int k = 0; k < 4; k++) mm[j][k] = (it < nit && x + k < W) ? D.maps[(int64_t)y * W + x + k] : 0u;
      }
#pragma unroll
      for (int j = 0; j < kS3Pre; j++) {
        const int it = base + tid + j * kS3Threads;
        if (it >= nit) break;
        const int y = it / nq, x = 4 * (it - y * nq);
        uint32_t pl[kSgPlanes] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t m = mm[j][k];  // 0 past the row end: adds nothing
          const uint32_t sk = m & 255u, e = (m >> 8) & 255u, t = (m >> 16) & 255u;
          const uint32_t se = sk * e, te = t * e;
          pl[0] |= e << (8 * k);
          pl[1] |= sk << (8 * k);
          pl[2] |= t << (8 * k);
          pl[3] |= (se & 255u) << (8 * k);
          pl[4] |= (se >> 8) << (8 * k);
          pl[5] |= (te & 255u) << (8 * k);
          pl[6] |= (te >> 8) << (8 * k);
          e_s += e;
          s_s += sk;
          t_s += t;
          se_s += se;
          te_s += te;
        }
#pragma unroll
        for (int p = 0; p < kSgPlanes; p++)
          *reinterpret_cast<uint32_t *>(lds3 + p * psz + y * pitch + x) = pl[p] ^ 0x80808080u;  // value - 128
      }
    }
    // wave sums (each < 2^32: <= 22.7 K pixels per image fit k_sc_score3's LDS)
    uint32_t v5[5] = {e_s, s_s, t_s, se_s, te_s};
#pragma unroll
    for (int i = 0; i < 5; i++)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v5[i] += __shfl_xor(v5[i], o, 64);
    if (lane == 0)
#pragma unroll
      for (int i = 0; i < 5; i++) ipart[wave][i] = v5[i];
    __syncthreads();
    if (tid == 0) {
      uint64_t S5[5] = {0, 0, 0, 0, 0};
      for (int w = 0; w < kS3Waves; w++)
        for (int i = 0; i < 5; i++) S5[i] += ipart[w][i];
      T[0] = (double)S5[0] / 255.0;
      T[1] = (double)S5[3] / 65025.0 + sb * ((double)S5[1] / 255.0);
      T[2] = (double)S5[4] / 65025.0 + tb * ((double)S5[2] / 255.0);
    }
  }
  // ---- 2. MFMA pass: the waves split between the groups in proportion to
  // their rows (one group's accumulators per wave); a wave takes rows
  // r, r + nw, ... of its group, each row's B fragments (L2) loaded three of
  // its rows ahead ----
  int gw = 0, w0 = 0, nw = kS3Waves;
  if (ng == 2) {
    const int r0 = G[0].nrows, r1 = G[1].nrows;
    const int n0 = min(kS3Waves - 1, max(1, (kS3Waves * r0 + (r0 + r1) / 2) / (r0 + r1)));
    if (wave >= n0) {
      gw = 1;
      w0 = n0;
      nw = kS3Waves - n0;
    } else {
      nw = n0;
    }
  }
  i32x4 acc[kSgPlanes];
#pragma unroll
  for (int p = 0; p < kSgPlanes; p++) acc[p] = i32x4{0, 0, 0, 0};
  if (!(kS3Abl & 1)) {
    const ScGroup *Gg = G + gw;
    const int nrows = __builtin_amdgcn_readfirstlane(Gg->nrows);
    const int ks = __builtin_amdgcn_readfirstlane(Gg->ks);
    const int ybase = __builtin_amdgcn_readfirstlane(Gg->ybase);
    const int nB = kSgDigits * __builtin_amdgcn_readfirstlane(Gg->nslot);
    const bool bl = (lane & 15) < nB;
    const i32x4 *bf = reinterpret_cast<const i32x4 *>(ai + Gg->bfrag);
    const int aoff = Gg->x0[lane & 15] + 16 * (lane >> 4);
    auto loadb = [&](int r, i32x4 (&b)[kSgMaxKs]) {
#pragma unroll
      for (int t = 0; t < kSgMaxKs; t++)
        b[t] = (r < nrows && t < ks && bl) ? bf[((int64_t)r * ks + t) * 64 + lane] : i32x4{0, 0, 0, 0};
    };
    auto row = [&](int r, const i32x4 (&b)[kSgMaxKs]) {
      const uint8_t *rowp = lds3 + (ybase + r) * pitch + aoff;
#pragma unroll
      for (int t = 0; t < kSgMaxKs; t++) {
        if (t < ks) {
#pragma unroll
          for (int p = 0; p < kSgPlanes; p++) {
            const uint8_t *a = rowp + p * psz + 64 * t;
            const i32x2 lo = *(l_ci32x2 *)(const __attribute__((address_space(3))) uint8_t *)a;
            const i32x2 hi = *(l_ci32x2 *)(const __attribute__((address_space(3))) uint8_t *)(a + 8);
            acc[p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(i32x4{lo.x, lo.y, hi.x, hi.y}, b[t], acc[p], 0, 0, 0);
          }
        }
      }
    };
    const int rs = wave - w0;
    i32x4 b0[kSgMaxKs], b1[kSgMaxKs], b2[kSgMaxKs];
    loadb(rs, b0);
    loadb(rs + nw, b1);
    loadb(rs + 2 * nw, b2);
#pragma unroll 1
    for (int r = rs; r < nrows; r += 3 * nw) {
      row(r, b0);
      loadb(r + 3 * nw, b0);
      if (r + nw < nrows) row(r + nw, b1);
      loadb(r + 4 * nw, b1);
      if (r + 2 * nw < nrows) row(r + 2 * nw, b2);
      loadb(r + 5 * nw, b2);
    }
  }
  // ---- 3. cross-wave sums (the planes are dead), then per crop ----
  __syncthreads();
  int32_t *red = reinterpret_cast<int32_t *>(lds3);  // [g][plane][16 x origins][16 (digit, slot)]
  auto red_at = [&](int g, int p, int i) { return ((g * kSgPlanes + p) * 16 + 4 * (lane >> 4) + i) * 16 + (lane & 15); };
  // the first wave of each group stores, the others add
  if (wave == w0) {
#pragma unroll
    for (int p = 0; p < kSgPlanes; p++)
#pragma unroll
      for (int i = 0; i < 4; i++) red[red_at(gw, p, i)] = acc[p][i];
  }
  __syncthreads();
  if (wave != w0) {
#pragma unroll
    for (int p = 0; p < kSgPlanes; p++)
#pragma unroll
      for (int i = 0; i < 4; i++) atomicAdd(&red[red_at(gw, p, i)], acc[p][i]);
  }
  __syncthreads();
  const double u = 1.1102230246251565e-16;  // 2^-53
  auto gam = [&](double n) { return n * u / (1.0 - n * u); };
  const double aoi = fabs(oi);
  const double wd = P.detail_weight, ws = P.skin_weight, wt = P.saturation_weight;
  if (kS3Abl & 4)
    for (int c = tid; c < ncrops; c += kS3Threads) {
      s_tot[c] = c;  // one candidate, no re-score
      s_bnd[c] = 0;
    }
  for (int c = tid; c < ((kS3Abl & 4) ? 0 : ncrops); c += kS3Threads) {
    const DevCrop cr = crops[D.crop0 + c];
    const ScGroup &Gr = G[cr.sg];
    double V[kSgPlanes], A[kSgPlanes];
#pragma unroll
    for (int p = 0; p < kSgPlanes; p++) {
      V[p] = 0;
      A[p] = 0;
#pragma unroll
      for (int k = 0; k < kSgDigits; k++) {
        const double v = ldexp((double)red[((cr.sg * kSgPlanes + p) * 16 + cr.sm) * 16 + kSgDigits * cr.sj + k], 8 * k);
        V[p] += v;
        A[p] += fabs(v);
      }
    }
    double S = 0, AS = 0;
#pragma unroll
    for (int k = 0; k < kSgDigits; k++) {
      const double v = ldexp(128.0 * (double)Gr.S[k], 8 * k);
      S += v;
      AS += fabs(v);
    }
    // sum_window Tq x (x = e, s, t, s e, t e) and their absolute counterparts
    const double xe = V[0] + S, xs = V[1] + S, xt = V[2] + S;
    const double xse = 256.0 * (V[4] + S) + (V[3] + S), xte = 256.0 * (V[6] + S) + (V[5] + S);
    const double ae = A[0] + AS, as = A[1] + AS, at = A[2] + AS;
    const double ase = 256.0 * (A[4] + AS) + (A[3] + AS), ate = 256.0 * (A[6] + AS) + (A[5] + AS);
    const double sc = ldexp(1.0, -Gr.q);
    const double Fd = xe * sc / 255.0 + oi * T[0];
    const double Fs = (xse / 65025.0 + sb * xs / 255.0) * sc + oi * T[1];
    const double Ft = (xte / 65025.0 + tb * xt / 255.0) * sc + oi * T[2];
    const double Ad = ae * sc / 255.0 + aoi * T[0];
    const double As = (ase / 65025.0 + sb * as / 255.0) * sc + aoi * T[1];
    const double At = (ate / 65025.0 + tb * at / 255.0) * sc + aoi * T[2];
    const double nn = (double)npx;
    const double kb = (2.0 * gam(nn + 5.0) * (cr.imax + aoi) + ldexp(1.0, -Gr.q - 1) + aoi * gam(nn + 16.0)) *
                      (1.0 + gam(nn + 16.0));
    const double Ed = kb * T[0] + gam(24.0) * Ad, Es = kb * T[1] + gam(24.0) * As, Et = kb * T[2] + gam(24.0) * At;
    const double area = cr.fw * cr.fh;
    const double tot = (Fd * wd + Fs * ws + Ft * wt) / area;
    const double mag = fabs(wd) * (fabs(Fd) + Ed) + fabs(ws) * (fabs(Fs) + Es) + fabs(wt) * (fabs(Ft) + Et);
    const double B = ((fabs(wd) * Ed + fabs(ws) * Es + fabs(wt) * Et) * (1.0 + 16.0 * u) + 16.0 * u * mag) /
                     area * 1.01;
    s_tot[c] = tot;
    s_bnd[c] = B;
    CropScore &o = sco[c];
    o.detail = Fd;
    o.saturation = Ft;
    o.skin = Fs;
    o.total = tot;
    o.bound = B;
    o.exact = 0;
  }
  __syncthreads();
  // ---- 4. candidates, exact re-score, argmax (k_sc_score2's non-"big" path) ----
  if (tid == 0) {
    double best_lo = -1.0e308;
    for (int c = 0; c < ncrops; c++) best_lo = fmax(best_lo, s_tot[c] - s_bnd[c]);
    int k = 0, first = -1;
    for (int c = 0; c < ncrops; c++)
      if (D.exact_all || s_tot[c] + s_bnd[c] >= best_lo) {
        if (first < 0) first = c;
        cand[k++] = c;
      }
    ncand_s = k;
    first_cand_s = first;
  }
  __syncthreads();
  const int ncand = ncand_s;
  const bool need_exact = D.exact_all || ncand > 1;
  if (need_exact) {
    uint32_t *smaps = reinterpret_cast<uint32_t *>(lds3);
    for (int k = tid; k < npx; k += kS3Threads) smaps[k] = D.maps[k];
    __syncthreads();
    for (int k = tid; k < ncand; k += kS3Threads) {
      const int c = cand[k];
      const DevCrop cr = crops[D.crop0 + c];
      const double *tab = ad + cr.table;
      double skin = 0, detail = 0, sat = 0;
      for (int y = 0; y < H; y++) {
        const bool yin = y >= cr.y0 && y < cr.y0 + cr.nin_y;
        const uint32_t *mrow = smaps + (int64_t)y * W;
        const int64_t trow = (int64_t)(y - cr.y0) * cr.table_w - cr.x0;
#pragma unroll 4
        for (int x = 0; x < W; x++) {
          const bool in = yin && x >= cr.x0 && x < cr.x0 + cr.nin_x;
          const double tv = tab[in ? trow + x : 0];
          const double imp = in ? tv : oi;
          const uint32_t m = mrow[x];
          const double det = lut[(m >> 8) & 255];
          skin = skin + lut[m & 255] * (det + sb) * imp;
          detail = detail + det * imp;
          sat = sat + lut[(m >> 16) & 255] * (det + tb) * imp;
        }
      }
      const double tot = (detail * wd + skin * ws + sat * wt) / (cr.fw * cr.fh);
      s_tot[c] = tot;
      CropScore &o = sco[c];
      o.detail = detail;
      o.saturation = sat;
      o.skin = skin;
      o.total = tot;
      o.bound = 0;
      o.exact = 1;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int top = first_cand_s;
    double best = s_tot[top];
    if (need_exact) {
      best = -9223372036854775807.0;  // -sys.maxsize; strict > keeps the first max
      for (int k = 0; k < ncand; k++) {
        const int c = cand[k];
        if (s_tot[c] > best) {
          best = s_tot[c];
          top = c;
        }
      }
    }
    results[D.result].top = top;
    results[D.result].n_candidates = ncand;
    results[D.result].total = best;
  }
}

int launch_sc_score(hipStream_t s, int mode, const ScDesc *descs, int n, size_t lds, const DevCrop *crops,
                    const double *ad, CropScore *scores, ScResult *results, const ScParamsDev &P, const int32_t *ai) {
  if (n <= 0) return 0;
  if (mode == 1) {
    if (lds > (size_t)kScoreLdsMaps) return -1;
    hipLaunchKernelGGL((k_sc_score2<1>), dim3(n), dim3(kScoreThreads), lds, s, descs, crops, ad, scores, results, P,
                       ai);
  } else {
    hipLaunchKernelGGL((k_sc_score2<0>), dim3(n), dim3(kScoreThreads), 0, s, descs, crops, ad, scores, results, P,
                       ai);
  }
  return 0;
}
int launch_sc_score3(hipStream_t s, const ScDesc *descs, int n, size_t lds, const DevCrop *crops, const ScGroup *groups,
                     const double *ad, CropScore *scores, ScResult *results, const ScParamsDev &P, const int32_t *ai) {
  if (n <= 0) return 0;
  if (lds > (size_t)kScore3Lds) return -1;
  hipLaunchKernelGGL(k_sc_score3, dim3(n), dim3(kS3Threads), lds, s, descs, crops, groups, ad, scores, results, P,
                     ai);
  return 0;
}

}  // namespace fi
