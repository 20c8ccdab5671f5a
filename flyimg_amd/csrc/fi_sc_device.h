// fi_sc_device.h -- smartcrop device functions shared by the generic
// (fi_kernels.hip) and fused (fi_sc_prep.hip, fi_sc_score.hip) kernels, so
// every path computes the same bits: the per-pixel functions first, then the
// phases the prescale kernels have in common.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fi_internal.h"

namespace fi {

// Pillow ImagingConvertMatrix L = R*0.2126 + G*0.7152 + B*0.0722 (smartcrop.py:94):
// float sum in order (no FMA: -ffp-contract=off), +0.5 in double, CLIPF.
__device__ __forceinline__ uint32_t sc_luma(uint32_t r, uint32_t g, uint32_t b) {
  float v = 0.2126f * (float)r + 0.7152f * (float)g;
  v = v + 0.0722f * (float)b;
  v = v + 0.0f;
  v = (float)((double)v + 0.5);
  return v <= 0.0f ? 0u : v >= 255.0f ? 255u : (uint32_t)v;
}

// Pillow Resample.c clip8 of a 22-bit fixed-point accumulator
__device__ __forceinline__ uint8_t pil_clip8(int32_t v) {
  v >>= 22;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// detect_skin (smartcrop.py:250-274) and saturation()/detect_saturation
// (:16-27, :234-248) of one pixel, f64 as numpy: the skin and the saturation
// byte (0 when below the threshold or outside the brightness range)
__device__ __forceinline__ uint32_t sc_skin_f64(double rd_, double gd_, double bd_, const ScParamsDev &P) {
  double rd = -P.skin_color[0], gd = -P.skin_color[1], bd = -P.skin_color[2];
  const double mag = sqrt(rd_ * rd_ + gd_ * gd_ + bd_ * bd_);
  if (!(fabs(mag) < 1e-6)) {
    rd = rd_ / mag - P.skin_color[0];
    gd = gd_ / mag - P.skin_color[1];
    bd = bd_ / mag - P.skin_color[2];
  }
  const double skin = 1 - sqrt(rd * rd + gd * gd + bd * bd);
  return skin > P.skin_threshold ? (uint32_t)(uint8_t)(int)((skin - P.skin_threshold) * (255 / (1 - P.skin_threshold)))
                                 : 0u;
}
__device__ __forceinline__ uint32_t sc_sat_f64(double rd_, double gd_, double bd_, const ScParamsDev &P) {
  const double mx = fmax(fmax(rd_, gd_), bd_), mn = fmin(fmin(rd_, gd_), bd_);
  double s = (mx + mn) / 255, d = (mx - mn) / 255;
  if (mx == mn) {
    d = 0;
    s = 1;
  }
  if (s > 1) s = 2 - d;
  const double sat = d / s;
  const double thr = P.saturation_threshold;
  return sat > thr ? (uint32_t)(uint8_t)(int)((sat - thr) * (255 / (1 - thr))) : 0u;
}
// packed skin | sat << 16
__device__ __forceinline__ uint32_t sc_skin_sat(uint32_t r, uint32_t g, uint32_t b, uint32_t L,
                                                const ScParamsDev &P) {
  const double Ld = (double)L;
  uint32_t S = 0, T = 0;
  if (Ld >= P.skin_brightness_min * 255 && Ld <= P.skin_brightness_max * 255) S = sc_skin_f64(r, g, b, P);
  if (Ld >= P.saturation_brightness_min * 255 && Ld <= P.saturation_brightness_max * 255) T = sc_sat_f64(r, g, b, P);
  return S | (T << 16);
}
// Cheap exact skin / saturation for most pixels (k_sc_fd's maps pass):
// sc_skin_sat_est returns true with the packed bytes when f32 arithmetic with
// an error margin decides them, false when the caller must take the exact
// value (k_sc_skinsat's table, or sc_skin_sat):
//  * brightness: L >= min * 255 <=> L >= ceil(min * 255) for an integer L, so
//    the reference's f64 compares become integer compares;
//  * skin: q = sum (rgb / |rgb| - c)^2 = 1 + |c|^2 - 2 c.rgb / |rgb|; skin =
//    1 - sqrt(q) > thr needs q < (1 - thr)^2.  The f32 q is within ~1e-6 of the
//    exact one (|c| <= 4), far inside the margin q > (1 - thr)^2 + 1e-4 that
//    rejects (skin byte 0); every other pixel in range is a candidate;
//  * saturation: sat = (mx - mn) / (mx + mn), or (mx - mn) / (510 - mx + mn)
//    when mx + mn > 255 (the reference's (mx + mn) / 255 > 1, exact on
//    integers); v = (sat - thr) * K with K = fl(255 / (1 - thr)) is within
//    E = 1e-6 K + 1e-4 of the f64 chain (each f32 step adds a few 2^-24
//    relative; sat <= 1, 0 <= thr <= 0.99), so v + E < 0 gives byte 0, and an interval
//    [v - E, v + E] above 0 with no integer in it gives (int) v.
// k_sc_skinsat builds its table through this function (f64 where it returns
// false), and the all-colours test compares that table with the oracle.
struct ScFast {
  float c0, c1, c2, cc, Q, thr, K, E;
  int32_t slo, shi, tlo, thi;  // brightness bounds (inclusive) on the integer luma
  int32_t skin_est, sat_est;   // the estimates apply to these parameters
};
__host__ __device__ __forceinline__ int32_t sc_lbound(double a) {  // L >= a <=> L >= ceil(a)
  return a <= 0 ? 0 : a > 256 ? 256 : (int32_t)ceil(a);
}
__host__ __device__ __forceinline__ int32_t sc_ubound(double b) {  // L <= b <=> L <= floor(b)
  return b < 0 ? -1 : b >= 255 ? 255 : (int32_t)floor(b);
}
__host__ __device__ __forceinline__ ScFast sc_fast_params(const ScParamsDev &P) {
  ScFast F;
  F.c0 = (float)P.skin_color[0];
  F.c1 = (float)P.skin_color[1];
  F.c2 = (float)P.skin_color[2];
  F.cc = F.c0 * F.c0 + F.c1 * F.c1 + F.c2 * F.c2;
  const double st = P.skin_threshold;
  F.skin_est = fabs(P.skin_color[0]) + fabs(P.skin_color[1]) + fabs(P.skin_color[2]) <= 4.0 && st < 0.9999;
  F.Q = (float)((1.0 - st) * (1.0 - st) + 1e-4);  // q > (1 - thr)^2 + 1e-4: skin < thr certainly
  const double tt = P.saturation_threshold;
  F.thr = (float)tt;
  F.K = (float)(255 / (1 - tt));
  F.E = 1e-6f * F.K + 1e-4f;
  F.sat_est = tt >= 0.0 && tt <= 0.99;
  F.slo = sc_lbound(P.skin_brightness_min * 255);
  F.shi = sc_ubound(P.skin_brightness_max * 255);
  F.tlo = sc_lbound(P.saturation_brightness_min * 255);
  F.thi = sc_ubound(P.saturation_brightness_max * 255);
  return F;
}
__device__ __forceinline__ bool sc_skin_sat_est(const ScFast &F, uint32_t r, uint32_t g, uint32_t b, uint32_t L,
                                                uint32_t &st) {
  const int32_t Li = (int32_t)L;
  uint32_t T = 0;
  if (Li >= F.slo && Li <= F.shi) {
    const uint32_t m2 = r * r + g * g + b * b;
    if (!F.skin_est || m2 == 0) return false;
    const float q = 1.0f + F.cc -
                    2.0f * (F.c0 * (float)r + F.c1 * (float)g + F.c2 * (float)b) * __builtin_amdgcn_rsqf((float)m2);
    if (!(q > F.Q)) return false;  // a skin candidate
  }
  if (Li >= F.tlo && Li <= F.thi) {
    const uint32_t mx = max(max(r, g), b), mn = min(min(r, g), b);
    if (!F.sat_est) return false;
    const uint32_t den = mx + mn > 255 ? 510 - (mx - mn) : mx + mn;
    const float sat = mx == mn ? 0.0f : (float)(mx - mn) * __builtin_amdgcn_rcpf((float)den);
    const float v = (sat - F.thr) * F.K;
    if (!(v + F.E < 0.0f)) {
      if (!(v - F.E > 0.0f) || floorf(v - F.E) != floorf(v + F.E)) return false;
      T = (uint32_t)(uint8_t)(int)v;
    }
  }
  st = T << 16;
  return true;
}

// ---- phases shared by the prescale + maps kernels (fi_sc_prep.hip), one
// definition each so the kernels produce the same bits.  None of them holds a
// barrier; loops, ablation switches and unroll pragmas stay with the callers.
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) i32x2 l_i32x2q;
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));

// 16 interleaved RGB pixels (three 16-byte loads) -> one 16-byte group per
// plane: plane dword k takes bytes 12k + {0,3,6,9} (+1 / +2 for G / B) of the
// three source dwords 3k .. 3k + 2
__device__ __forceinline__ void sc_deint16(const u32x4a (&q)[3], u32x4s &w0, u32x4s &w1, u32x4s &w2) {
  const uint32_t d[12] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    w0[k] = deint_rgb4(0, d[3 * k], d[3 * k + 1], d[3 * k + 2]);
    w1[k] = deint_rgb4(1, d[3 * k], d[3 * k + 1], d[3 * k + 2]);
    w2[k] = deint_rgb4(2, d[3 * k], d[3 * k + 1], d[3 * k + 2]);
  }
}
// the same group byte by byte (gray or unaligned rows, row tails): pixels
// x0 .. x0 + 15 of the row at s; past the row (or a row past the source) 128.
// U is the callers' unroll factor of the two loops (k_sc_fz: 1, registers).
template <int U>
__device__ __forceinline__ void sc_gather16(const uint8_t *s, int x0, bool rowok, int sW, int sC, u32x4s &w0,
                                            u32x4s &w1, u32x4s &w2) {
#pragma unroll U
  for (int k = 0; k < 4; k++) {
    uint32_t a = 0, b = 0, c = 0;
#pragma unroll U
    for (int j = 0; j < 4; j++) {
      const int x = x0 + 4 * k + j;
      const bool ok = rowok && x < sW;
      uint32_t vr, vg, vb;
      if (sC == 3) {
        vr = ok ? s[3 * x] : 128u;
        vg = ok ? s[3 * x + 1] : 128u;
        vb = ok ? s[3 * x + 2] : 128u;
      } else {
        vr = vg = vb = ok ? s[x] : 128u;
      }
      a |= vr << (8 * j);
      b |= vg << (8 * j);
      c |= vb << (8 * j);
    }
    w0[k] = a ^ 0x80808080u;
    w1[k] = b ^ 0x80808080u;
    w2[k] = c ^ 0x80808080u;
  }
}

// horizontal pass, column block b: the lane's B fragments (k-step t, limb q),
// the block's first source column and the lane's column bias
__device__ __forceinline__ void sc_hm_load_b(const int32_t *hmS0, const int32_t *hmC, const i32x4 *hmB, int KS, int b,
                                             int lane, int aw, i32x4 (&Bf)[2][3], int &s0, int32_t &cx) {
  s0 = hmS0[b];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int q = 0; q < 3; q++) Bf[t][q] = t < KS ? hmB[((b * KS + t) * 3 + q) * 64 + lane] : i32x4{0, 0, 0, 0};
  const int x = 16 * b + (lane & 15);
  cx = x < aw ? hmC[x] : 0;
}
// horizontal MFMA of one planar 16-row block (arow: the lane's plane row
// lane & 15 at the block's first source column; k0 / k8 = mfma_i8_k(lane, 0 / 8))
// with one column block: limb sum + bias, clip -> the lane's H-stage bytes of
// rows 4 (lane >> 4) + i, column lane & 15.  The caller stores them (hbuf as p,
// the LDS ring as p - 128).
__device__ __forceinline__ void sc_hm_block(const uint8_t *arow, int KS, int k0, int k8, const i32x4 (&Bf)[2][3],
                                            int32_t cx, uint8_t (&o)[4]) {
  i32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0}, acc2 = {0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 2; t++) {
    if (t < KS) {
      const uint8_t *base = arow + 64 * t;
      const i32x2 lo = *reinterpret_cast<const i32x2 *>(base + k0);
      const i32x2 hi = *reinterpret_cast<const i32x2 *>(base + k8);
      const i32x4 a = {lo.x, lo.y, hi.x, hi.y};
      acc0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, Bf[t][0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, Bf[t][1], acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, Bf[t][2], acc2, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    // modular int32: the limbs' partial products may wrap, the sum fits
    const uint32_t v = (uint32_t)acc0[i] + ((uint32_t)acc1[i] << 8) + ((uint32_t)acc2[i] << 16) + (uint32_t)cx;
    o[i] = pil_clip8((int32_t)v);
  }
}

// vertical MFMA of one tile of 16 byte columns (pA / pB: the lane's two
// transposed 8-byte reads of the 64-row window, at the tile): the chunk's
// prescaled rows m = 4 (lane >> 4) + i < nr, byte column col0 + (lane & 15),
// into prer.  sum = D0 + 256 D1 + 65536 D2 + cy is Pillow's accumulator.
__device__ __forceinline__ void sc_vq_tile(const uint8_t *pA, const uint8_t *pB, const i32x4 &A0, const i32x4 &A1,
                                           const i32x4 &A2, const int32_t (&cy)[4], uint8_t *prer, int apitch,
                                           int col0, int nbytes, int nr, int lane) {
  const i32x2 lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((l_i32x2q *)pA);
  const i32x2 hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((l_i32x2q *)pB);
  const i32x4 B = {lo.x, lo.y, hi.x, hi.y};
  const i32x4 d2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A2, B, i32x4{0, 0, 0, 0}, 0, 0, 0);
  const i32x4 d1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, B, d2 << 8, 0, 0, 0);
  const i32x4 d0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0, B, i32x4{0, 0, 0, 0}, 0, 0, 0);
  const int col = col0 + (lane & 15);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int m = 4 * (lane >> 4) + i;
    // modular int32: the limbs' partial products may wrap, the sum fits
    const int32_t sv = (int32_t)((uint32_t)d0[i] + ((uint32_t)d1[i] << 8) + (uint32_t)cy[i]);
    if (col < nbytes && m < nr) prer[m * apitch + col] = pil_clip8(sv);
  }
}

// luma of one prescaled pixel q into *l; the pixel itself to o when the
// caller keeps the prescaled image (o == nullptr: not kept / a halo row)
__device__ __forceinline__ void sc_luma_item(const uint8_t *q, uint8_t *l, uint8_t *o) {
  *l = (uint8_t)sc_luma(q[0], q[1], q[2]);
  if (o) {
    o[0] = q[0];
    o[1] = q[1];
    o[2] = q[2];
  }
}

// detect_edge (smartcrop.py:231, ImagingFilter3x3 with the Laplacian kernel):
// the interior value from a luma and its four neighbours ...
__device__ __forceinline__ uint32_t sc_edge_clamp(uint32_t L, uint32_t up, uint32_t dn, uint32_t lt, uint32_t rt) {
  const int v = 4 * (int)L - (int)up - (int)dn - (int)lt - (int)rt + 1;
  return (uint32_t)(v <= 0 ? 0 : v >= 255 ? 255 : v);
}
// ... which holds inside a w x h image of at least 3 x 3; the border copies L
__device__ __forceinline__ bool sc_edge_interior(int x, int y, int w, int h) {
  return w >= 3 && h >= 3 && x > 0 && y > 0 && x < w - 1 && y < h - 1;
}
// ... and both from a luma plane (lrow: row y of it, lpitch bytes a row)
__device__ __forceinline__ uint32_t sc_edge(const uint8_t *lrow, int lpitch, int x, int y, int aw, int ah) {
  const uint32_t L = lrow[x];
  return sc_edge_interior(x, y, aw, ah) ? sc_edge_clamp(L, lrow[x - lpitch], lrow[x + lpitch], lrow[x - 1], lrow[x + 1])
                                        : L;
}

// a k_sc_skinsat table entry (skin | sat << 8) as sc_skin_sat packs it
__device__ __forceinline__ uint32_t sc_skinsat_unpack(uint32_t t) { return (t & 255u) | ((t >> 8) << 16); }

// A thread's (row, column) walk over [rows][aw] items it = tid, tid + threads,
// ...: start and step once, no integer division per item.
struct ScWalk {
  int y, x, stepy, stepx, aw;
  __device__ __forceinline__ ScWalk(int tid, int threads, int aw_) : aw(aw_) {
    stepy = threads / aw;
    stepx = threads - stepy * aw;
    y = tid / aw;
    x = tid - y * aw;
  }
  // (row, column) of the current item, then one step on
  __device__ __forceinline__ void next(int &row, int &col) {
    if (x >= aw) {
      x -= aw;
      y++;
    }
    row = y;
    col = x;
    y += stepy;
    x += stepx;
  }
};

}  // namespace fi
