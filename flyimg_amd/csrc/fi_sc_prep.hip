// fi_sc_prep.hip -- smartcrop.py's saliency stage, part 1: prescale + maps.
// (fi_sc_score.hip scores the crops, fi_sc_apply.hip copies the winning box.)
// The phases the kernels have in common are defined once in fi_sc_device.h.
//
//   k_sc_fz       (default) Pillow thumbnail (22-bit fixed-point Lanczos,
//                 Resample.c) horizontal pass as exact-integer MFMA into an LDS
//                 ring, vertical MFMA pass, then the analyse() maps (luma,
//                 Laplacian edge, skin and saturation from the 2^24-colour
//                 table of k_sc_skinsat; smartcrop.py:94-101, 231-274) -> packed
//                 maps (skin | edge << 8 | sat << 16).
//   k_sc_hmfma + k_sc_vq  the same two passes as two kernels (H-stage rows
//                 through HBM) where k_sc_fz's LDS does not fit (reduced
//                 sources, wide analysed images).
//   k_sc_vmaps    the vertical pass + maps on the VALU, where a 16-row
//                 MFMA block's window exceeds 64 H-stage rows (prescale
//                 factors > ~3: cfg5's 400 -> 111).
//   k_sc_fd       k_sc_fz with the source rows streamed by LDS-DMA loader waves.
//   k_sc_hx + k_sc_vx  the same passes without LDS, beside the next resample.
//
// The generic per-row kernels in fi_kernels.hip remain for geometries the
// per-image kernels do not take (no prescale, staging that does not fit LDS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fi_internal.h"
#include "fi_sc_device.h"

namespace fi {

constexpr int kPrepThreads = 256;


// ---- k_sc_hmfma: the same horizontal pass as exact integer MFMA.  One
// workgroup per (image, chunk of hm_rows H-stage rows).  Source rows are
// staged as three planar channels of (p - 128) in signed bytes; each wave
// takes 16-column output blocks: D = A(16 rows x 64 cols of one channel)
// x B(64 cols x 16 outputs) with v_mfma_i32_16x16x64_i8 per coefficient limb,
// then sum = D0 + 256 D1 + 65536 D2 + 2^21 + 128 sum(k) is Pillow's int32
// accumulator bit for bit (Resample.c ImagingResampleHorizontal_8bpc).
__global__ __launch_bounds__(kPrepThreads) void k_sc_hmfma(const ScDesc *__restrict__ descs,
                                                           const int32_t *__restrict__ ai) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds8[];
  const ScDesc &D = descs[blockIdx.x];
  const int R = D.hm_rows, P = D.hm_pitch, KS = D.hm_ks, nb = D.hm_nb;
  const int r0 = blockIdx.y * R;
  if (r0 >= D.hrows) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool reduced = D.fx > 1 || D.fy > 1;
  const uint8_t *src = reduced ? D.red : D.img;
  const int64_t sstride = reduced ? (int64_t)D.rw * 3 : D.stride;
  const int sC = reduced ? 3 : D.C;
  const int sW = reduced ? D.rw : D.W;
  const int aw = D.aw, hrows = D.hrows, yoff = D.ybox_first;
  const int apitch = (aw * 3 + 15) & ~15;
  const int nch = sC == 3 ? 3 : 1;
  // ---- stage rows [r0, r0 + R) as planes [c][row][P] of (p - 128); zero pad.
  // One item = 16 pixels of a row: three 16-byte loads (dword-aligned rows),
  // deinterleaved into one 16-byte LDS store per plane; row tails pad with 128.
  const int ng = P >> 4;  // 16-pixel groups per plane row
  const bool a4 = (((uintptr_t)src | (uintptr_t)sstride) & 3) == 0;
  // batches of 4 items per thread: all 12 loads of a batch are issued before
  // the first is consumed (one HBM round trip per batch, not per item)
  for (int base = 0; base < R * ng; base += 4 * kPrepThreads) {
    u32x4a q[4][3];
    bool fast[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int it = base + u * kPrepThreads + tid;
      const int rr = it / ng, g = it - rr * ng;
      const uint8_t *s = src + (int64_t)(r0 + rr + yoff) * sstride;
      fast[u] = it < R * ng && r0 + rr < hrows && sC == 3 && a4 && 16 * g + 16 <= sW;
      if (fast[u]) {
#pragma unroll
        for (int k = 0; k < 3; k++) q[u][k] = *reinterpret_cast<const u32x4a *>(s + 48 * g + 16 * k);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int it = base + u * kPrepThreads + tid;
      if (it >= R * ng) break;
      const int rr = it / ng, g = it - rr * ng;
      const bool rowok = r0 + rr < hrows;
      const uint8_t *s = src + (int64_t)(r0 + rr + yoff) * sstride;
      u32x4s w0, w1, w2;
      if (fast[u]) {
        sc_deint16(q[u], w0, w1, w2);
      } else {
        sc_gather16<4>(s, 16 * g, rowok, sW, sC, w0, w1, w2);
      }
      *reinterpret_cast<u32x4s *>(lds8 + (0 * R + rr) * P + 16 * g) = w0;
      if (nch == 3) {
        *reinterpret_cast<u32x4s *>(lds8 + (1 * R + rr) * P + 16 * g) = w1;
        *reinterpret_cast<u32x4s *>(lds8 + (2 * R + rr) * P + 16 * g) = w2;
      }
    }
  }
  __syncthreads();
  const int32_t *hmS0 = ai + D.hmS0, *hmC = ai + D.hmC;
  const i32x4 *hmB = reinterpret_cast<const i32x4 *>(ai + D.hmB);
  const int k0 = mfma_i8_k(lane, 0), k8 = mfma_i8_k(lane, 8);
  for (int b = wave; b < nb; b += kPrepThreads / 64) {
    i32x4 Bf[2][3];
    int s0;
    int32_t cx;
    sc_hm_load_b(hmS0, hmC, hmB, KS, b, lane, aw, Bf, s0, cx);
    const int x = 16 * b + (lane & 15);
    for (int c = 0; c < nch; c++) {
      for (int rb = 0; rb < R; rb += 16) {
        uint8_t o[4];
        sc_hm_block(lds8 + (c * R + rb + (lane & 15)) * P + s0, KS, k0, k8, Bf, cx, o);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int row = r0 + rb + 4 * (lane >> 4) + i;
          if (x < aw && row < hrows) {
            uint8_t *dst = D.hbuf + (int64_t)row * apitch + 3 * x;
            if (nch == 3) {
              dst[c] = o[i];
            } else {
              dst[0] = dst[1] = dst[2] = o[i];
            }
          }
        }
      }
    }
  }
}


// ---- k_sc_vmaps: Pillow's vertical pass + analyse() maps, one workgroup per
// (image, chunk of kPrepRows output rows).  The H-stage rows the chunk and its
// one-row halo need are staged in LDS (from hbuf, or from the source when no
// horizontal pass runs), the prescaled rows [y0-1, y1+1) are computed into
// LDS, then the maps of [y0, y1) are written.
__global__ __launch_bounds__(kPrepThreads) void k_sc_vmaps(const ScDesc *__restrict__ descs,
                                                           const int32_t *__restrict__ ai, const ScParamsDev P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds8[];
  const ScDesc &D = descs[blockIdx.x];
  const int aw = D.aw, ah = D.ah;
  const int y0 = blockIdx.y * kPrepRows;
  if (y0 >= ah) return;
  const int y1 = min(y0 + kPrepRows, ah);
  const int pa = max(0, y0 - 1), pb = min(ah, y1 + 1);
  const int tid = threadIdx.x;
  const int apitch = (aw * 3 + 15) & ~15;
  const int32_t *vb = ai + D.vb, *vk = ai + D.vk;
  const bool need_v = D.need_v;
  int lo = pa, hi = pb;
  if (need_v) {
    lo = vb[2 * pa];
    hi = 0;
    for (int y = pa; y < pb; y++) hi = max(hi, vb[2 * y] + vb[2 * y + 1]);
  }
  uint8_t *rows = lds8;                        // [hi - lo][apitch] H-stage rows
  uint8_t *prer = lds8 + (hi - lo) * apitch;   // [pb - pa][apitch] prescaled rows
  if (D.need_h) {
    const int nq = apitch >> 4;
    for (int it = tid; it < (hi - lo) * nq; it += kPrepThreads) {
      const int rr = it / nq, k = it - rr * nq;
      reinterpret_cast<uint4 *>(rows + rr * apitch)[k] =
          reinterpret_cast<const uint4 *>(D.hbuf + (int64_t)(lo + rr) * apitch)[k];
    }
  } else {
    const bool reduced = D.fx > 1 || D.fy > 1;
    const uint8_t *src = reduced ? D.red : D.img;
    const int64_t sstride = reduced ? (int64_t)D.rw * 3 : D.stride;
    const int sC = reduced ? 3 : D.C;
    for (int it = tid; it < (hi - lo) * aw; it += kPrepThreads) {
      const int rr = it / aw, x = it - rr * aw;
      const uint8_t *s = src + (int64_t)(lo + rr) * sstride + x * sC;
      uint8_t *o = rows + rr * apitch + 3 * x;
      o[0] = s[0];
      o[1] = s[sC == 3 ? 1 : 0];
      o[2] = s[sC == 3 ? 2 : 0];
    }
  }
  __syncthreads();
  for (int it = tid; it < (pb - pa) * aw; it += kPrepThreads) {
    const int yr = it / aw, x = it - yr * aw, y = pa + yr;
    uint8_t *q = prer + yr * apitch + 3 * x;
    if (need_v) {
      const int ymin = vb[2 * y], cnt = vb[2 * y + 1];
      const int32_t *k = vk + y * D.ksv;
      const uint8_t *p = rows + (ymin - lo) * apitch + 3 * x;
      int32_t s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
      for (int j = 0; j < cnt; j++) {
        const int32_t kj = k[j];
        s0 += (int32_t)p[j * apitch] * kj;
        s1 += (int32_t)p[j * apitch + 1] * kj;
        s2 += (int32_t)p[j * apitch + 2] * kj;
      }
      q[0] = pil_clip8(s0);
      q[1] = pil_clip8(s1);
      q[2] = pil_clip8(s2);
    } else {
      const uint8_t *p = rows + (y - lo) * apitch + 3 * x;
      q[0] = p[0];
      q[1] = p[1];
      q[2] = p[2];
    }
  }
  __syncthreads();
  for (int it = tid; it < (y1 - y0) * aw; it += kPrepThreads) {
    const int yr = it / aw, x = it - yr * aw, y = y0 + yr;
    const uint8_t *row = prer + (y - pa) * apitch;
    const uint32_t r = row[3 * x], g = row[3 * x + 1], b = row[3 * x + 2];
    if (D.pre) {
      uint8_t *o = D.pre + ((int64_t)y * aw + x) * 3;
      o[0] = (uint8_t)r;
      o[1] = (uint8_t)g;
      o[2] = (uint8_t)b;
    }
    const uint32_t L = sc_luma(r, g, b);
    // detect_edge: ImagingFilter3x3 interior, border copies L
    uint32_t E = L;
    if (sc_edge_interior(x, y, aw, ah)) {
      const uint8_t *up = row - apitch, *dn = row + apitch;
      E = sc_edge_clamp(L, sc_luma(up[3 * x], up[3 * x + 1], up[3 * x + 2]),
                        sc_luma(dn[3 * x], dn[3 * x + 1], dn[3 * x + 2]),
                        sc_luma(row[3 * x - 3], row[3 * x - 2], row[3 * x - 1]),
                        sc_luma(row[3 * x + 3], row[3 * x + 4], row[3 * x + 5]));
    }
    D.maps[(int64_t)y * aw + x] = sc_skin_sat(r, g, b, L, P) | (E << 8);
  }
}

// ---- k_sc_vq: Pillow's vertical pass (Resample.c ImagingResampleVertical_8bpc)
// as exact integer MFMA, fused with analyse()'s maps.  One workgroup per
// (image, chunk of kVqRows analysed rows): the chunk's 16 prescaled rows
// (with the one-row edge halo) are ONE 16-row MFMA block over a window of <= 64
// H-stage rows; N = 16 interleaved channel bytes per tile (the vertical pass
// never mixes columns).  sum = D0 + 256 D1 + 65536 D2 + C[y] is Pillow's int32
// accumulator bit for bit (pixels enter as p - 128, C = 2^21 + 128 sum k).
// Luma is computed once per prescaled pixel into LDS for the 3x3 edge filter.
__global__ __launch_bounds__(kPrepThreads) void k_sc_vq(const ScDesc *__restrict__ descs,
                                                        const int32_t *__restrict__ ai, const ScParamsDev P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds8[];
  const ScDesc &D = descs[blockIdx.x];
  const int c = blockIdx.y;
  const int aw = D.aw, ah = D.ah;
  const int y0 = kVqRows * c;
  if (y0 >= ah) return;
  const int y1 = min(y0 + kVqRows, ah), pa = max(0, y0 - 1), pe = min(ah, pa + 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int apitch = (aw * 3 + 15) & ~15, lpitch = (aw + 3) & ~3;
  uint8_t *stg = lds8;                    // [64][apitch] H-stage rows as p - 128
  uint8_t *prer = lds8 + 64 * apitch;     // [16][apitch] prescaled rows pa..pe-1
  uint8_t *lum = prer + 16 * apitch;      // [16][lpitch] their luma
  const int k0 = ai[D.vqK0 + c], hrows = D.hrows;
  // ---- stage the window (rows past the H stage are zero-weight: any bytes)
  const int nq = apitch >> 4;
  for (int it = tid; it < 64 * nq; it += kPrepThreads) {
    const int r = it / nq, q = it - r * nq;
    const int hr = min(k0 + r, hrows - 1);
    uint4 v = reinterpret_cast<const uint4 *>(D.hbuf + (int64_t)hr * apitch)[q];
    v.x ^= 0x80808080u;
    v.y ^= 0x80808080u;
    v.z ^= 0x80808080u;
    v.w ^= 0x80808080u;
    reinterpret_cast<uint4 *>(stg + r * apitch)[q] = v;
  }
  const i32x4 *af = reinterpret_cast<const i32x4 *>(ai + D.vqA) + (size_t)c * 3 * 64;
  const i32x4 A0 = af[lane], A1 = af[64 + lane], A2 = af[128 + lane];
  int32_t cy[4];
#pragma unroll
  for (int i = 0; i < 4; i++) cy[i] = ai[D.vqC + min(pa + 4 * (lane >> 4) + i, ah - 1)];
  __syncthreads();
  // ---- vertical pass: tiles of 16 byte columns over the waves
  const int rA = 16 * (lane >> 4) + ((lane & 15) >> 1);
  const uint8_t *pA = stg + rA * apitch + 8 * (lane & 1), *pB = pA + 8 * apitch;
  const int nbytes = 3 * aw;
  const int nr = pe - pa;
  for (int t = wave; t < nq; t += kPrepThreads / 64)
    sc_vq_tile(pA + 16 * t, pB + 16 * t, A0, A1, A2, cy, prer, apitch, 16 * t, nbytes, nr, lane);
  __syncthreads();
  // ---- luma of every prescaled pixel (and the prescaled image when kept)
  for (int it = tid; it < nr * aw; it += kPrepThreads) {
    const int m = it / aw, x = it - m * aw, y = pa + m;
    sc_luma_item(prer + m * apitch + 3 * x, lum + m * lpitch + x,
                 D.pre && y >= y0 && y < y1 ? D.pre + ((int64_t)y * aw + x) * 3 : nullptr);
  }
  __syncthreads();
  // ---- maps of the chunk's rows: detect_edge (ImagingFilter3x3 interior,
  // border copies L), skin and saturation
  for (int it = tid; it < (y1 - y0) * aw; it += kPrepThreads) {
    const int yr = it / aw, x = it - yr * aw, y = y0 + yr, m = y - pa;
    const uint8_t *lrow = lum + m * lpitch;
    const uint32_t E = sc_edge(lrow, lpitch, x, y, aw, ah);
    const uint8_t *q = prer + m * apitch + 3 * x;
    D.maps[(int64_t)y * aw + x] = sc_skin_sat(q[0], q[1], q[2], lrow[x], P) | (E << 8);
  }
}

// ---- k_sc_fz: the whole prescale + maps of ONE image per workgroup (k_sc_hmfma
// and k_sc_vq fused; no H-stage round trip through HBM).  The image's source
// rows stream through in blocks of 16 (one MFMA row block of the horizontal
// pass); their H-stage rows (p - 128 bytes) go to an LDS ring of kFzRing rows;
// each chunk of kVqRows analysed rows runs as soon as the ring holds its
// 64-row window (k_sc_vq's vertical MFMA, luma, edge / skin / saturation).
// Two workgroups per CU overlap one's loads with the other's MFMAs.  LDS: ring kFzRing x apitch, then one region shared by the
// source planes (horizontal phase) and the prescaled rows + luma (vertical).
// Arithmetic is k_sc_hmfma's and k_sc_vq's: Pillow's int32 accumulators bit
// for bit.
constexpr int kFzRing = 80;  // a 64-row window at any 16-row block alignment
constexpr int kFzThreads = 512;  // 8 waves; two workgroups per CU (LDS)
#ifndef FI_FZ_ABL
#define FI_FZ_ABL 0
#endif
// profiling ablations (wrong maps): 1 no source loads, 2 no horizontal pass,
// 4 no vertical pass, 8 no luma loop, 16 no maps loop
constexpr int kFzAbl = FI_FZ_ABL;
constexpr int kFzGather = 4;                // skin/saturation table reads in flight per thread
// skin | saturation << 8 of every 24-bit colour (sc_skin_sat of the colour and
// its luma) at sc_colour_key(r, g, b): built once per parameter set, a gather replaces ~200 f64 VALU
// instructions per analysed pixel in k_sc_fz; bit-identical by construction.
__global__ __launch_bounds__(256) void k_sc_skinsat(uint16_t *__restrict__ t, const ScParamsDev P) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;  // (r << 16) | (g << 8) | b
  const uint32_t r = c >> 16, g = (c >> 8) & 255u, b = c & 255u;
  const uint32_t L = sc_luma(r, g, b);
  uint32_t v;
  if (!sc_skin_sat_est(sc_fast_params(P), r, g, b, L, v)) v = sc_skin_sat(r, g, b, L, P);
  t[sc_colour_key(r, g, b)] = (uint16_t)((v & 255u) | ((v >> 16) << 8));
}

// n / d for 0 <= n < 2^22, 0 < d < 2^12 from a float reciprocal and one
// correction each way (exact: the float quotient is within 1 of n / d)
__device__ __forceinline__ int fz_div(int n, int d, float rcp) {
  int q = (int)((float)n * rcp);
  const int r = n - q * d;
  q += r >= d ? 1 : 0;
  q -= r < 0 ? 1 : 0;
  return q;
}

__global__ __launch_bounds__(kFzThreads, 4) void k_sc_fz(const ScDesc *__restrict__ descs,
                                                        const int32_t *__restrict__ ai, const ScParamsDev P,
                                                        const uint16_t *__restrict__ skinsat) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds8[];
  const ScDesc &D = descs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int aw = D.aw, ah = D.ah, hrows = D.hrows, yoff = D.ybox_first;
  const int apitch = (aw * 3 + 15) & ~15, lpitch = (aw + 3) & ~3;
  const int PP = D.hm_pitch, KS = D.hm_ks, nb = D.hm_nb;
  const uint8_t *src = D.img;
  const int64_t sstride = D.stride;
  const int sC = D.C, sW = D.W, nch = sC == 3 ? 3 : 1;
  uint8_t *ring = lds8;                                   // [kFzRing][apitch] H-stage rows, p - 128
  uint8_t *shared = lds8 + kFzRing * apitch;              // source planes [c][16][PP] | prer + lum
  uint8_t *prer = shared, *lum = shared + 16 * apitch;    // [16][apitch] prescaled rows, [16][lpitch] luma
  const int ng = PP >> 4;                                 // 16-pixel groups per plane row
  const float rcp_ng = 1.0f / (float)ng;
  const int nitem = 16 * ng;                              // items of one 16-row block
  const bool a4 = (((uintptr_t)src | (uintptr_t)sstride) & 3) == 0;
  // one block of 16 source rows -> planes of (p - 128): items of 16 pixels of a
  // row, two per thread at a time (six 16-byte loads in flight, then the
  // deinterleave); RGB row tails as dword + byte loads issued together (a
  // byte-by-byte tail loop serialised ~16 load round trips per block); gray
  // or unaligned sources byte by byte
  auto stage_block = [&](int r0) {
#pragma unroll 1
    for (int base = 0; base < nitem; base += 2 * kFzThreads) {
      u32x4a q[2][3];
      bool fast[2];
      int rrs[2], gs[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int it = base + u * kFzThreads + tid;
        const int rr = fz_div(it, ng, rcp_ng), g = it - rr * ng;
        rrs[u] = rr;
        gs[u] = g;
        fast[u] = it < nitem && sC == 3 && a4;
        if (fast[u]) {
          const uint8_t *s = src + (int64_t)(r0 + rr + yoff) * sstride + 48 * g;
          const int remb = r0 + rr < hrows ? 3 * (sW - 16 * g) : 0;  // the group's bytes inside the row
          if (kFzAbl & 1) {  // profiling ablation: no source loads
#pragma unroll
            for (int k = 0; k < 3; k++) q[u][k] = u32x4a{(uint32_t)it, (uint32_t)r0, (uint32_t)k, (uint32_t)g};
          } else if (remb >= 48) {
#pragma unroll
            for (int k = 0; k < 3; k++) q[u][k] = *reinterpret_cast<const u32x4a *>(s + 16 * k);
          } else {
            // row tail (or a row / group past the source): whole dwords, then
            // the last bytes, all loads in flight together; pixels past the
            // row read as 128 like the plane padding
            uint32_t d[12];
#pragma unroll
            for (int k = 0; k < 12; k++) {
              if (4 * k + 4 <= remb) {
                d[k] = *reinterpret_cast<const uint32_t *>(s + 4 * k);
              } else {
                uint32_t v = 0x80808080u;
#pragma unroll
                for (int j = 0; j < 3; j++)
                  if (4 * k + j < remb) v = (v & ~(0xFFu << (8 * j))) | ((uint32_t)s[4 * k + j] << (8 * j));
                d[k] = v;
              }
            }
#pragma unroll
            for (int k = 0; k < 3; k++) q[u][k] = u32x4a{d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]};
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int it = base + u * kFzThreads + tid;
        if (it >= nitem) break;
        const int rr = rrs[u], g = gs[u];
        const bool rowok = r0 + rr < hrows;
        const uint8_t *s = src + (int64_t)(r0 + rr + yoff) * sstride;
        u32x4s w0, w1, w2;
        if (fast[u]) {
          sc_deint16(q[u], w0, w1, w2);
        } else {
          sc_gather16<1>(s, 16 * g, rowok, sW, sC, w0, w1, w2);
        }
        *reinterpret_cast<u32x4s *>(shared + (0 * 16 + rr) * PP + 16 * g) = w0;
        if (nch == 3) {
          *reinterpret_cast<u32x4s *>(shared + (1 * 16 + rr) * PP + 16 * g) = w1;
          *reinterpret_cast<u32x4s *>(shared + (2 * 16 + rr) * PP + 16 * g) = w2;
        }
      }
    }
  };
  const int32_t *hmS0 = ai + D.hmS0, *hmC = ai + D.hmC;
  const i32x4 *hmB = reinterpret_cast<const i32x4 *>(ai + D.hmB);
  const int k0l = mfma_i8_k(lane, 0), k8l = mfma_i8_k(lane, 8);
  auto hpass = [&](int r0) {  // the staged block -> H-stage rows r0 .. r0 + 15 into the ring
    // a wave's two column blocks (b, b + 8) per pass: both blocks' weight
    // fragments are loaded before the first block's MFMAs, so the second
    // block's load latency hides behind the first block's work
    constexpr int kW = kFzThreads / 64;
    if (kFzAbl & 2) return;
#pragma unroll 1
    for (int bp = wave; bp < nb; bp += 2 * kW) {
      i32x4 Bfs[2][2][3];
      int s0s[2];
      int32_t cxs[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int b = bp + h * kW;
        if (b < nb) sc_hm_load_b(hmS0, hmC, hmB, KS, b, lane, aw, Bfs[h], s0s[h], cxs[h]);
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int b = bp + h * kW;
        if (b >= nb) break;
        const int x = 16 * b + (lane & 15);
#pragma unroll 1
        for (int c = 0; c < nch; c++) {
          uint8_t o[4];
          sc_hm_block(shared + (c * 16 + (lane & 15)) * PP + s0s[h], KS, k0l, k8l, Bfs[h], cxs[h], o);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int row = r0 + 4 * (lane >> 4) + i;
            if (x < aw && row < hrows) {
              const uint8_t v = (uint8_t)(o[i] ^ 0x80u);
              uint8_t *dst = ring + (row % kFzRing) * apitch + 3 * x;
              if (nch == 3) {
                dst[c] = v;
              } else {
                dst[0] = dst[1] = dst[2] = v;
              }
            }
          }
        }
      }
    }
  };
  // ---- stream the H stage, run each analysed-row chunk once its window is in
  const int chunks = (ah + kVqRows - 1) / kVqRows;
  int produced = 0;  // H-stage rows in the ring: [produced - ring span, produced)
  const int rA = 16 * (lane >> 4) + ((lane & 15) >> 1);
  const int nq = apitch >> 4, nbytes = 3 * aw;
  const ScWalk walk0(tid, kFzThreads, aw);  // the luma and maps loops' (row, column) walks start here
#pragma unroll 1
  for (int c = 0; c < chunks; c++) {
    const int k0 = ai[D.vqK0 + c];
    const int need = min(k0 + 64, hrows);
    while (produced < need) {
      __syncthreads();  // the shared region's previous readers (vertical phase) are done
      stage_block(produced);
      __syncthreads();
      hpass(produced);
      produced += 16;
    }
    __syncthreads();  // ring rows of the window complete; the shared region is free
    const int y0 = kVqRows * c, y1 = min(y0 + kVqRows, ah), pa = max(0, y0 - 1), pe = min(ah, pa + 16);
    const i32x4 *af = reinterpret_cast<const i32x4 *>(ai + D.vqA) + (size_t)c * 3 * 64;
    const i32x4 A0 = af[lane], A1 = af[64 + lane], A2 = af[128 + lane];
    int32_t cy[4];
#pragma unroll
    for (int i = 0; i < 4; i++) cy[i] = ai[D.vqC + min(pa + 4 * (lane >> 4) + i, ah - 1)];
    // window row r lives in ring row (k0 + r) % kFzRing
    const uint8_t *pA = ring + ((k0 + rA) % kFzRing) * apitch + 8 * (lane & 1);
    const uint8_t *pB = ring + ((k0 + rA + 8) % kFzRing) * apitch + 8 * (lane & 1);
    const int nr = pe - pa;
#pragma unroll 1
    for (int t = wave; t < ((kFzAbl & 4) ? 0 : nq); t += kFzThreads / 64)
      sc_vq_tile(pA + 16 * t, pB + 16 * t, A0, A1, A2, cy, prer, apitch, 16 * t, nbytes, nr, lane);
    __syncthreads();
    ScWalk lw = walk0;
#pragma unroll 1
    for (int it = tid; it < ((kFzAbl & 8) ? 0 : nr * aw); it += kFzThreads) {
      int m, x;
      lw.next(m, x);
      const int y = pa + m;
      sc_luma_item(prer + m * apitch + 3 * x, lum + m * lpitch + x,
                   D.pre && y >= y0 && y < y1 ? D.pre + ((int64_t)y * aw + x) * 3 : nullptr);
    }
    __syncthreads();
    // maps of the chunk's rows: detect_edge (ImagingFilter3x3 interior,
    // border copies L), skin and saturation (kFzGather table reads in flight
    // per thread before they are used)
    const int nit = (y1 - y0) * aw;
    ScWalk mw = walk0;
#pragma unroll 1
    for (int base = tid; base < ((kFzAbl & 16) ? 0 : nit); base += kFzGather * kFzThreads) {
      uint32_t sv[kFzGather];
      int yrs[kFzGather], xs[kFzGather];
#pragma unroll
      for (int u = 0; u < kFzGather; u++) {
        mw.next(yrs[u], xs[u]);
        sv[u] = 0;
        if (base + u * kFzThreads < nit) {
          const uint8_t *qq = prer + (y0 + yrs[u] - pa) * apitch + 3 * xs[u];
          sv[u] = skinsat[sc_colour_key(qq[0], qq[1], qq[2])];
        }
      }
#pragma unroll
      for (int u = 0; u < kFzGather; u++) {
        if (base + u * kFzThreads >= nit) break;
        const int x = xs[u], y = y0 + yrs[u];
        const uint32_t E = sc_edge(lum + (y - pa) * lpitch, lpitch, x, y, aw, ah);
        D.maps[(int64_t)y * aw + x] = sc_skinsat_unpack(sv[u]) | (E << 8);
      }
    }
  }
}

// ---- k_sc_fd: k_sc_fz's passes (same tables, same arithmetic, bit-identical
// maps) with the source stream decoupled from the compute.  One 16-wave
// workgroup per CU: waves 0-13 run the horizontal pass, the vertical pass,
// luma and maps; waves 14-15 copy 16-row source blocks by LDS-DMA
// (global_load_lds_dwordx4, no VGPRs, no VALU) into kFdSlots raw slots, two
// blocks ahead of the horizontal pass, and wait for each with an exact vmcnt.
// k_sc_fz has one block of loads in flight per workgroup only while it stages
// (ablation: 0.24 of its 0.55 ms per cfg2 step are that load latency); here
// they stay in flight through the MFMA and maps phases.  The horizontal pass
// reads its A fragments straight from the raw interleaved rows (three 8-byte
// LDS reads per 8 pixels, v_perm into the three channels), so there is no
// staging pass and no plane buffer.  One barrier per source block, plus three
// per analysed-row chunk.  Needs 3-channel sources with 16-B aligned rows
// readable to fd_rp(W) bytes (the host's ScDesc.fd).
constexpr int kFdThreads = 1024;
constexpr int kFdC = kFdCWaves * 64;
#ifndef FI_FD_ABL
#define FI_FD_ABL 0
#endif
// profiling ablations (wrong maps): 1 no source DMA, 2 no horizontal pass,
// 4 no vertical pass, 8 no luma loop, 16 no maps loop, 64 no map stores
constexpr int kFdAbl = FI_FD_ABL;
// skin / saturation: sc_skin_sat_est per pixel and k_sc_skinsat's table only
// for what it leaves open (not k_sc_fz's table read of every pixel): one
// workgroup per CU has no second workgroup to cover the gathers' latency,
// and the L2 serves divergent gathers one line per request
__device__ __forceinline__ void fd_dma16(uint32_t m0, const uint8_t *sbase, uint32_t voff) {
  // lane i's 16 bytes at sbase + voff land at LDS m0 + 16 i (m0, sbase uniform)
  unsigned keep;
  const uint64_t sb = (uint64_t)(uintptr_t)sbase;
  sbase = reinterpret_cast<const uint8_t *>((uintptr_t)(
      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(sb >> 32)) << 32) |
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sb)));
  m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)m0);
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(m0)
      : "memory");
}
// s_waitcnt vmcnt(n) for n <= 15 (larger n wait for 15: conservative)
__device__ __forceinline__ void fd_wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
    case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
  }
}

// workgroup barrier without the vmcnt(0) that __syncthreads' fence adds: the
// loader waves' DMAs for the next blocks stay in flight across it (LDS
// accesses are complete at lgkmcnt(0); nothing here reads a global store of
// this kernel)
__device__ __forceinline__ void fd_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ __launch_bounds__(kFdThreads) void k_sc_fd(const ScDesc *__restrict__ descs,
                                                      const int32_t *__restrict__ ai, const ScParamsDev P,
                                                      const uint16_t *__restrict__ skinsat) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds8[];
  const ScDesc &D = descs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool loader = wave >= kFdCWaves;
  const int aw = D.aw, ah = D.ah, hrows = D.hrows, yoff = D.ybox_first;
  const int apitch = (aw * 3 + 15) & ~15, lpitch = (aw + 3) & ~3;
  const int PP = D.hm_pitch, KS = D.hm_ks, nb = D.hm_nb;
  const int RP = fd_rp(D.W), slotB = fd_slot_bytes(D.W);
  const int64_t sstride = D.stride;
  uint8_t *raw = lds8;                                         // [kFdSlots][16][RP] source rows
  uint8_t *ring = lds8 + fd_ring_off(D.W, PP);                 // [kFzRing][apitch] H-stage rows, p - 128
  uint8_t *prer = ring + kFzRing * apitch, *lum = prer + 16 * apitch;  // [16][apitch], [16][lpitch]
  uint8_t *abuf = lds8 + fd_tab_off(D.W, PP, aw);             // [chunks][3][64] i32x4 vertical A fragments
  const int chunks = (ah + kVqRows - 1) / kVqRows;
  int32_t *cbuf = reinterpret_cast<int32_t *>(abuf + chunks * 3072);  // [ah] vertical bias
  const int nblk = (min(ai[D.vqK0 + chunks - 1] + 64, hrows) + 15) >> 4;  // blocks the last chunk needs
  // ---- loader side: block blk -> slot blk % kFdSlots, DMA steps i = lw, lw + 2, ...
  const int ninstr = slotB >> 10, lw = wave - kFdCWaves;
  const int cnt = (ninstr - lw + 1) >> 1;  // this loader wave's DMAs per block
  const int rpc = RP >> 4;                 // 16-byte chunks per row
  const float rcp_rpc = 1.0f / (float)rpc;
  const uint32_t raw_m0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)raw;
  const uint32_t ab_m0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)abuf;
  auto issue = [&](int blk) {
    if (blk >= nblk || (kFdAbl & 1)) return;
    const int r0 = blk << 4;
    const uint8_t *sb = D.img + (int64_t)(r0 + yoff) * sstride;
    const int last = hrows - 1 - r0;  // rows past the analysed rows repeat the last one (never used)
#pragma unroll 1
    for (int i = lw; i < ninstr; i += 2) {
      const int j = 64 * i + lane;
      int row = fz_div(j, rpc, rcp_rpc);
      const int col = j - row * rpc;
      row = min(row, min(15, last));  // lanes past the block's 16 rows land in the slot's padding
      fd_dma16(raw_m0 + (uint32_t)((blk % kFdSlots) * slotB + 1024 * i), sb,
               (uint32_t)(row * sstride + 16 * col));
    }
  };
  // ---- compute side: wave w owns column block w (the host admits images of
  // <= kFdCWaves blocks: aw <= 224; cfg2: 13); its B fragments stay in
  // registers for the whole image
  const int32_t *hmS0 = ai + D.hmS0, *hmC = ai + D.hmC;
  const i32x4 *hmB = reinterpret_cast<const i32x4 *>(ai + D.hmB);
  const int k0l = mfma_i8_k(lane, 0), k8l = mfma_i8_k(lane, 8);
  i32x4 Bh[2][3];
  int s0h = 0;
  int32_t cxh = 0;
  if (!loader && wave < nb) sc_hm_load_b(hmS0, hmC, hmB, KS, wave, lane, aw, Bh, s0h, cxh);
  // the slot's 16 rows x column block b -> H-stage rows r0 .. r0 + 15
  auto hpass_block = [&](int r0, const uint8_t *slot, int b, const i32x4 (&Bf)[2][3], int s0, int32_t cx) {
    const int x = 16 * b + (lane & 15);
    i32x4 acc[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int q = 0; q < 3; q++) acc[c][q] = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 2; t++) {
      if (t < KS) {
        const uint8_t *rp = slot + (lane & 15) * RP + 3 * (s0 + 64 * t);
        const i32x2 *p0 = reinterpret_cast<const i32x2 *>(rp + 3 * k0l);
        const i32x2 *p1 = reinterpret_cast<const i32x2 *>(rp + 3 * k8l);
        const i32x2 u0 = p0[0], u1 = p0[1], u2 = p0[2], v0 = p1[0], v1 = p1[1], v2 = p1[2];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const i32x4 a = {(int32_t)deint_rgb4(c, u0.x, u0.y, u1.x), (int32_t)deint_rgb4(c, u1.y, u2.x, u2.y),
                           (int32_t)deint_rgb4(c, v0.x, v0.y, v1.x), (int32_t)deint_rgb4(c, v1.y, v2.x, v2.y)};
#pragma unroll
          for (int q = 0; q < 3; q++) acc[c][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, Bf[t][q], acc[c][q], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int row = r0 + 4 * (lane >> 4) + i;
      if (x < aw && row < hrows) {
        uint8_t *dst = ring + (row % kFzRing) * apitch + 3 * x;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const uint32_t v = (uint32_t)acc[c][0][i] + ((uint32_t)acc[c][1][i] << 8) + ((uint32_t)acc[c][2][i] << 16) +
                             (uint32_t)cx;
          dst[c] = (uint8_t)(pil_clip8((int32_t)v) ^ 0x80u);
        }
      }
    }
  };
  auto hpass = [&](int r0, const uint8_t *slot) {
    if (wave < nb) hpass_block(r0, slot, wave, Bh, s0h, cxh);
  };
  const int rA = 16 * (lane >> 4) + ((lane & 15) >> 1);
  const int nq = apitch >> 4, nbytes = 3 * aw;
  const ScWalk walk0(tid, kFdC, aw);  // the maps loop's (row, column) walk starts here
  const ScFast F = sc_fast_params(P);
  const int ng4 = (aw + 3) >> 2;  // luma: 4-pixel groups per row
  const float rcp_ng4 = 1.0f / (float)ng4;
  // ---- prologue: every chunk's vertical A fragments, source blocks 0 and 1
  // in flight; the vertical bias into LDS; block 0 and the fragments landed
  if (loader) {
    const uint8_t *afrag = reinterpret_cast<const uint8_t *>(ai + D.vqA);
#pragma unroll 1
    for (int k = lw; k < 3 * chunks; k += 2) fd_dma16(ab_m0 + 1024 * k, afrag, (uint32_t)(1024 * k + 16 * lane));
    issue(0);
    issue(1);
    fd_wait_vm(1 < nblk ? cnt : 0);
  } else {
#pragma unroll 1
    for (int i = tid; i < ah; i += kFdC) cbuf[i] = ai[D.vqC + i];
  }
  fd_barrier();
  int blk = 0;  // next block for the horizontal pass (in slot blk % kFdSlots)
#pragma unroll 1
  for (int c = 0; c < chunks; c++) {
    const int k0 = ai[D.vqK0 + c];
    const int need = min(k0 + 64, hrows);
    bool phased = false;
#pragma unroll 1
    while (16 * blk < need) {
      if (loader) {
        issue(blk + 2);                        // into the slot block blk - 1 left
        fd_wait_vm(blk + 2 < nblk ? cnt : 0);  // block blk + 1 landed
      } else if (!(kFdAbl & 2)) {
        hpass(16 * blk, raw + (blk % kFdSlots) * slotB);
      }
      fd_barrier();
      blk++;
      phased = true;
    }
    // the chunk's window is in the ring; the last chunk's maps are done with
    // prer / lum (a barrier of their own when no block ran in between)
    if (!phased) fd_barrier();
    const int y0 = kVqRows * c, y1 = min(y0 + kVqRows, ah), pa = max(0, y0 - 1), pe = min(ah, pa + 16);
    const int nr = pe - pa;
    if (!loader) {
      const i32x4 *af = reinterpret_cast<const i32x4 *>(abuf + c * 3072);
      const i32x4 A0 = af[lane], A1 = af[64 + lane], A2 = af[128 + lane];
      int32_t cy[4];
#pragma unroll
      for (int i = 0; i < 4; i++) cy[i] = cbuf[min(pa + 4 * (lane >> 4) + i, ah - 1)];
      const uint8_t *pA = ring + ((k0 + rA) % kFzRing) * apitch + 8 * (lane & 1);
      const uint8_t *pB = ring + ((k0 + rA + 8) % kFzRing) * apitch + 8 * (lane & 1);
#pragma unroll 1
      for (int t = wave; t < ((kFdAbl & 4) ? 0 : nq); t += kFdCWaves)
        sc_vq_tile(pA + 16 * t, pB + 16 * t, A0, A1, A2, cy, prer, apitch, 16 * t, nbytes, nr, lane);
    }
    fd_barrier();
    const int nit = (y1 - y0) * aw;  // maps items (analysed rows y0 .. y1 - 1)
    if (!loader) {
      // luma of the prescaled rows pa .. pe - 1, four pixels per item
#pragma unroll 1
      for (int it = tid; it < ((kFdAbl & 8) ? 0 : nr * ng4); it += kFdC) {
        const int m = fz_div(it, ng4, rcp_ng4), g = it - m * ng4;
        const uint32_t *q = reinterpret_cast<const uint32_t *>(prer + m * apitch + 12 * g);
        const uint32_t a0 = q[0], a1 = q[1], a2 = q[2];
        const uint32_t R = deint_rgb4(0, a0, a1, a2) ^ 0x80808080u, G = deint_rgb4(1, a0, a1, a2) ^ 0x80808080u,
                       B = deint_rgb4(2, a0, a1, a2) ^ 0x80808080u;
        uint32_t l4 = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
          l4 |= sc_luma((R >> (8 * j)) & 255u, (G >> (8 * j)) & 255u, (B >> (8 * j)) & 255u) << (8 * j);
        *reinterpret_cast<uint32_t *>(lum + m * lpitch + 4 * g) = l4;
        const int y = pa + m;
        if (D.pre && y >= y0 && y < y1) {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int x = 4 * g + j;
            if (x < aw) {
              uint8_t *o = D.pre + ((int64_t)y * aw + x) * 3;
              o[0] = (uint8_t)(R >> (8 * j));
              o[1] = (uint8_t)(G >> (8 * j));
              o[2] = (uint8_t)(B >> (8 * j));
            }
          }
        }
      }
    }
    fd_barrier();
    if (!loader) {
      // kFzGather items per step: skin / saturation by sc_skin_sat_est, the
      // table read only for the items it leaves open (skin candidates,
      // saturation bytes at an integer boundary), all in flight together
      ScWalk mw = walk0;
#pragma unroll 1
      for (int base = tid; base < ((kFdAbl & 16) ? 0 : nit); base += kFzGather * kFdC) {
        uint32_t stv[kFzGather];
        int yrs[kFzGather], xs[kFzGather];
#pragma unroll
        for (int u = 0; u < kFzGather; u++) {
          mw.next(yrs[u], xs[u]);
          stv[u] = 0;
          if (base + u * kFdC < nit) {
            const int m = y0 + yrs[u] - pa;
            const uint8_t *qq = prer + m * apitch + 3 * xs[u];
            const uint32_t r = qq[0], g = qq[1], b = qq[2];
            if (!sc_skin_sat_est(F, r, g, b, lum[m * lpitch + xs[u]], stv[u]))
              stv[u] = sc_skinsat_unpack(skinsat[sc_colour_key(r, g, b)]);
          }
        }
#pragma unroll
        for (int u = 0; u < kFzGather; u++) {
          const int it = base + u * kFdC;
          if (it >= nit) break;
          const int x = xs[u], y = y0 + yrs[u];
          const uint32_t E = sc_edge(lum + (y - pa) * lpitch, lpitch, x, y, aw, ah);
          if (!(kFdAbl & 64)) D.maps[(int64_t)y * aw + x] = stv[u] | (E << 8);
        }
      }
    }
  }
  if (loader) fd_wait_vm(0);  // every DMA landed before the workgroup retires
}

// ---- k_sc_hx + k_sc_vx: the same prescale + maps (same integer arithmetic,
// bit-identical maps) shaped to run BESIDE the next batch's k_rs_vr: no LDS,
// <= 64 VGPRs (launch_bounds(256, 8)), so their waves take the one wave slot
// per SIMD that k_rs_vr's workgroup leaves free (as k_crop_apply3p does),
// instead of a serial stage between two resamples.
//  * k_sc_hx: one wave per (image, 16-column block b), looping over 16-row
//    blocks of the H stage (k_sc_hmfma's B fragments stay in registers).  A
//    lane's A operand is 16 consecutive source pixels (48 contiguous bytes);
//    limbs fold through the accumulator (t = A B2; t = A B1 + (t << 8);
//    t = A B0 + (t << 8) + C', C' = Pillow's bias - 2^29, so the H-stage byte
//    as p - 128 is med3(t >> 22, -128, 127)).  The MFMA result lane
//    (g, n) holds rows 4g .. 4g + 3 of column n: one dword store per channel
//    into the TRANSPOSED H stage tbuf[b][ch][n][row] (p - 128 bytes).
//  * k_sc_vx: one wave per (image, chunk of kVqRows analysed rows): per
//    column block, the chunk's 16 prescaled rows = one MFMA block whose B
//    operand is 16 contiguous bytes of a tbuf column (rows K0 + 16 g ..); the
//    lane then holds R, G, B of 4 vertically adjacent pixels.  Luma is packed
//    4 bytes a dword; the Laplacian's row neighbours come from lanes -+16
//    (ds_bpermute), its column neighbours by DPP within the 16-lane row, the
//    previous / next block's edge column through the rotate's `old` operand, so
//    a block's maps are written one block late.  Skin / saturation: k_sc_fd's
//    estimator, k_sc_skinsat's table for what it leaves open.
// The host runs both on the apply stream behind the batch's resample, so they
// overlap the next batch's k_rs_vr (fi_api.cpp launch_batch).
// (the RGB two-k-step forms at 128 VGPRs: at 64 they spill, and they never
// run beside k_rs_vr -- FI_SC_CX=3 is for uniform cfg2-like batches)
template <int KS, int NCH>
__global__ __launch_bounds__(256, KS == 2 && NCH == 3 ? 4 : 8) void k_sc_hx(const ScDesc *__restrict__ descs,
                                                                          const int32_t *__restrict__ tiles,
                                                                          const int32_t *__restrict__ ai) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int di = tiles[3 * blockIdx.x];
  if (di < 0) return;
  const ScDesc &D = descs[di];
  const int b = tiles[3 * blockIdx.x + 1] + wave, rb0 = tiles[3 * blockIdx.x + 2];
  if (b >= D.hm_nb) return;
  const int g = lane >> 4, r = lane & 15;
  const int aw = D.aw, hrows = D.hrows, yoff = D.ybox_first, tp = D.cx_tp;
  const int rp = NCH == 3 ? fd_rp(D.W) : (D.W + 15) & ~15;  // readable bytes of a row
  const int s0 = ai[D.hmS0 + b];
  const i32x4 *hmB = reinterpret_cast<const i32x4 *>(ai + D.hmB) + (size_t)b * KS * 3 * 64 + lane;
  // B fragments in registers, except at two k-steps of RGB (64 VGPRs: from L1 per item)
  constexpr bool kKeepB = !(KS == 2 && NCH == 3);
  i32x4 Bf[kKeepB ? KS : 1][3];
  if (kKeepB)
#pragma unroll
    for (int t = 0; t < KS; t++)
#pragma unroll
      for (int q = 0; q < 3; q++) Bf[kKeepB ? t : 0][q] = hmB[(t * 3 + q) * 64];
  auto bfrag = [&](int t, int q) {
    const i32x4 *hb = hmB;
    if (!kKeepB) asm volatile("" : "+v"(hb));  // re-read per use: not hoisted out of the row loop
    return kKeepB ? Bf[kKeepB ? t : 0][q] : hb[(t * 3 + q) * 64];
  };
  const int x = 16 * b + r;
  const int32_t cxp = x < aw ? ai[D.hmC + x] - (1 << 29) : 0;
  constexpr int NQ = NCH == 3 ? 3 : 1;  // 16-B loads per k-step
  const int64_t sstride = D.stride;
  // tbuf tiles [b][ch][row block][16 columns][16 rows]: a store instruction
  // writes one whole 256-B tile (lane (g, n): column n, rows 4g .. 4g + 3)
  const int nrbt = tp >> 4;
  uint8_t *tcol = D.tbuf + (int64_t)b * NCH * nrbt * 256 + 16 * r + 4 * g;
  auto load = [&](int rb, u32x4a (&q)[KS][NQ]) {
    const int hr = min(16 * rb + r, hrows - 1);
    const uint8_t *row = D.img + (int64_t)(hr + yoff) * sstride;
#pragma unroll
    for (int t = 0; t < KS; t++)
#pragma unroll
      for (int i = 0; i < NQ; i++) {
        const int off = (NCH == 3 ? 3 : 1) * (s0 + 64 * t + 16 * g) + 16 * i;  // 8-B aligned
        u32x4a v = *reinterpret_cast<const u32x4a *>(row + min(off, rp - 16));
        if (off > rp - 16) v = off == rp - 8 ? u32x4a{v.z, v.w, 0u, 0u} : u32x4a{0u, 0u, 0u, 0u};
        q[t][i] = v;
      }
  };
  // row blocks [rb0, rb0 + kHxRb) of the H stage (the last tile row block is
  // the V pass's straddle margin, never read as data)
  const int nrb = min(nrbt - 1, rb0 + kHxRb);
  constexpr bool kPre = KS * NQ <= 3;  // the next row block's loads in flight (within 64 VGPRs)
  u32x4a cur[KS][NQ], nxt[KS][NQ];
  load(rb0, cur);
#pragma unroll 1
  for (int rb = rb0; rb < nrb; rb++) {
    if (!kPre && rb > rb0) load(rb, cur);
    if (kPre && rb + 1 < nrb) load(rb + 1, nxt);
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
      i32x4 A[KS];
#pragma unroll
      for (int t = 0; t < KS; t++) {
        if (NCH == 3) {
          const uint32_t d[12] = {cur[t][0].x, cur[t][0].y, cur[t][0].z, cur[t][0].w, cur[t][1].x, cur[t][1].y,
                                  cur[t][1].z, cur[t][1].w, cur[t][2].x, cur[t][2].y, cur[t][2].z, cur[t][2].w};
          A[t] = i32x4{(int32_t)deint_rgb4(ch, d[0], d[1], d[2]), (int32_t)deint_rgb4(ch, d[3], d[4], d[5]),
                       (int32_t)deint_rgb4(ch, d[6], d[7], d[8]), (int32_t)deint_rgb4(ch, d[9], d[10], d[11])};
        } else {
          A[t] = i32x4{(int32_t)(cur[t][0].x ^ 0x80808080u), (int32_t)(cur[t][0].y ^ 0x80808080u),
                       (int32_t)(cur[t][0].z ^ 0x80808080u), (int32_t)(cur[t][0].w ^ 0x80808080u)};
        }
      }
      // limbs folded through the accumulator (modular int32)
      i32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < KS; t++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], bfrag(t, 2), acc, 0, 0, 0);
      acc = acc << 8;
#pragma unroll
      for (int t = 0; t < KS; t++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], bfrag(t, 1), acc, 0, 0, 0);
      acc = (acc << 8) + i32x4{cxp, cxp, cxp, cxp};
#pragma unroll
      for (int t = 0; t < KS; t++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], bfrag(t, 0), acc, 0, 0, 0);
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) w |= ((uint32_t)min(max(acc[i] >> 22, -128), 127) & 255u) << (8 * i);
      *reinterpret_cast<uint32_t *>(tcol + ((int64_t)ch * nrbt + rb) * 256) = w;
    }
    if (kPre)
#pragma unroll
      for (int t = 0; t < KS; t++)
#pragma unroll
        for (int i = 0; i < NQ; i++) cur[t][i] = nxt[t][i];
  }
}

__device__ __forceinline__ uint32_t vx_byte(uint32_t v, int i) { return (v >> (8 * i)) & 255u; }

template <int KV, int NCH>
__global__ __launch_bounds__(256, KV == 2 && NCH == 3 ? 4 : 8) void k_sc_vx(const ScDesc *__restrict__ descs,
                                                                          const int32_t *__restrict__ tiles,
                                                                          const int32_t *__restrict__ ai, const ScFast F,
                                                                          const uint16_t *__restrict__ skinsat) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tix = 4 * blockIdx.x + wave;
  const int di = tiles[2 * tix], c = tiles[2 * tix + 1];
  if (di < 0) return;
  const ScDesc &D = descs[di];
  const int g = lane >> 4, n = lane & 15;
  const int aw = D.aw, ah = D.ah, tp = D.cx_tp, nb = D.hm_nb;
  const int y0 = kVqRows * c, y1 = min(y0 + kVqRows, ah), pa = max(0, y0 - 1);
  // the chunk's A fragments, read per block (L1 hits): registers are the budget
  const i32x4 *af = reinterpret_cast<const i32x4 *>(ai + D.cxA) + (size_t)c * KV * 3 * 64 + lane;
  int32_t cy[4];
#pragma unroll
  for (int i = 0; i < 4; i++) cy[i] = ai[D.vqC + min(pa + 4 * g + i, ah - 1)];
  // the window's rows K0 + 64 t + 16 g .. + 15 of column n straddle row blocks
  // rb0 + 4 t + g and the next at dword offset m = (K0 & 15) / 4 (uniform)
  const int K0 = ai[D.cxK0 + c], nrbt = tp >> 4, m4 = (K0 & 15) >> 2;
  const uint8_t *tb = D.tbuf + ((int64_t)(K0 >> 4) + g) * 256 + 16 * n;
  const bool edges = aw >= 3 && ah >= 3;
  // block b's prescaled bytes of the lane's 4 rows, one dword per channel
  auto vpass = [&](int b, uint32_t (&rgb)[3]) {
    const i32x4 *afb = af;
    asm volatile("" : "+v"(afb));  // re-read per block: not hoisted into 12-24 live VGPRs
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
      const uint8_t *col = tb + (int64_t)(b * NCH + ch) * nrbt * 256;
      i32x4 B[KV];
#pragma unroll
      for (int t = 0; t < KV; t++) {
        const i32x4 lo = *reinterpret_cast<const i32x4 *>(col + 1024 * t);
        if (m4 == 0) {
          B[t] = lo;
        } else {
          const i32x4 hi = *reinterpret_cast<const i32x4 *>(col + 1024 * t + 256);
          B[t] = m4 == 1 ? i32x4{lo.y, lo.z, lo.w, hi.x} : m4 == 2 ? i32x4{lo.z, lo.w, hi.x, hi.y}
                                                             : i32x4{lo.w, hi.x, hi.y, hi.z};
        }
      }
      i32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < KV; t++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afb[(t * 3 + 2) * 64], B[t], acc, 0, 0, 0);
      acc = acc << 8;
#pragma unroll
      for (int t = 0; t < KV; t++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afb[(t * 3 + 1) * 64], B[t], acc, 0, 0, 0);
      acc = (acc << 8) + i32x4{cy[0], cy[1], cy[2], cy[3]};
#pragma unroll
      for (int t = 0; t < KV; t++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afb[(t * 3 + 0) * 64], B[t], acc, 0, 0, 0);
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) w |= (uint32_t)pil_clip8(acc[i]) << (8 * i);
      rgb[ch] = w;
      asm volatile("" ::: "memory");  // one channel's fragments live at a time (64 VGPRs)
    }
    if (NCH == 1) rgb[1] = rgb[2] = rgb[0];
  };
  auto luma4 = [&](const uint32_t (&rgb)[3]) {
    uint32_t l4 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) l4 |= sc_luma(vx_byte(rgb[0], i), vx_byte(rgb[1], i), vx_byte(rgb[2], i)) << (8 * i);
    return l4;
  };
  uint32_t cur[3] = {0, 0, 0}, prv[3] = {0, 0, 0};
  uint32_t Lc = 0, Lp = 0, Lpp = 0;  // luma of blocks b, b - 1, b - 2
#pragma unroll 1
  for (int b = 0; b <= nb; b++) {
    if (b < nb) {
      vpass(b, cur);
      Lc = luma4(cur);
    }
    if (b > 0) {  // maps of block b - 1
      const int x = 16 * (b - 1) + n;
      const uint32_t up = (uint32_t)__shfl((int)Lp, lane - 16, 64), dn = (uint32_t)__shfl((int)Lp, lane + 16, 64);
      const uint32_t lt = (uint32_t)__builtin_amdgcn_update_dpp(
          __builtin_amdgcn_update_dpp(0, (int)Lpp, 0x121, 0xF, 0xF, false), (int)Lp, 0x111, 0xF, 0xF, false);
      const uint32_t rt = (uint32_t)__builtin_amdgcn_update_dpp(
          __builtin_amdgcn_update_dpp(0, (int)Lc, 0x12F, 0xF, 0xF, false), (int)Lp, 0x101, 0xF, 0xF, false);
      uint32_t stv[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t rr = vx_byte(prv[0], i), gg = vx_byte(prv[1], i), bb = vx_byte(prv[2], i);
        if (!sc_skin_sat_est(F, rr, gg, bb, vx_byte(Lp, i), stv[i]))
          stv[i] = sc_skinsat_unpack(skinsat[sc_colour_key(rr, gg, bb)]);
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int y = pa + 4 * g + i;
        if (x >= aw || y < y0 || y >= y1) continue;
        const uint32_t L = vx_byte(Lp, i);
        uint32_t E = L;
        if (edges && x > 0 && y > 0 && x < aw - 1 && y < ah - 1) {
          const uint32_t u = i > 0 ? vx_byte(Lp, i - 1) : vx_byte(up, 3);
          const uint32_t d = i < 3 ? vx_byte(Lp, i + 1) : vx_byte(dn, 0);
          E = sc_edge_clamp(L, u, d, vx_byte(lt, i), vx_byte(rt, i));
        }
        D.maps[(int64_t)y * aw + x] = stv[i] | (E << 8);
        if (D.pre) {  // the prescaled image, when the caller keeps it
          uint8_t *o = D.pre + ((int64_t)y * aw + x) * 3;
          o[0] = (uint8_t)vx_byte(prv[0], i);
          o[1] = (uint8_t)vx_byte(prv[1], i);
          o[2] = (uint8_t)vx_byte(prv[2], i);
        }
      }
    }
    Lpp = Lp;
    Lp = Lc;
#pragma unroll
    for (int k = 0; k < 3; k++) prv[k] = cur[k];
  }
}

int launch_sc_hx(hipStream_t s, int ks, int nch, const ScDesc *descs, const int32_t *tiles, int ntiles,
                 const int32_t *ai) {
  if (ntiles <= 0) return 0;
  const dim3 grid(ntiles), blk(256);
  if (ks == 1 && nch == 3) hipLaunchKernelGGL((k_sc_hx<1, 3>), grid, blk, 0, s, descs, tiles, ai);
  else if (ks == 2 && nch == 3) hipLaunchKernelGGL((k_sc_hx<2, 3>), grid, blk, 0, s, descs, tiles, ai);
  else if (ks == 1 && nch == 1) hipLaunchKernelGGL((k_sc_hx<1, 1>), grid, blk, 0, s, descs, tiles, ai);
  else if (ks == 2 && nch == 1) hipLaunchKernelGGL((k_sc_hx<2, 1>), grid, blk, 0, s, descs, tiles, ai);
  else return -1;
  return 0;
}
int launch_sc_vx(hipStream_t s, int kv, int nch, const ScDesc *descs, const int32_t *tiles, int ntiles,
                 const int32_t *ai, const ScParamsDev &P, const uint16_t *skinsat) {
  if (ntiles <= 0) return 0;
  if (ntiles % 4) return -1;  // four waves (tiles) a workgroup; the host pads
  const dim3 grid(ntiles / 4), blk(256);
  const ScFast F = sc_fast_params(P);  // host-side: kernel arguments stay in SGPRs
  if (kv == 1 && nch == 3) hipLaunchKernelGGL((k_sc_vx<1, 3>), grid, blk, 0, s, descs, tiles, ai, F, skinsat);
  else if (kv == 2 && nch == 3) hipLaunchKernelGGL((k_sc_vx<2, 3>), grid, blk, 0, s, descs, tiles, ai, F, skinsat);
  else if (kv == 1 && nch == 1) hipLaunchKernelGGL((k_sc_vx<1, 1>), grid, blk, 0, s, descs, tiles, ai, F, skinsat);
  else if (kv == 2 && nch == 1) hipLaunchKernelGGL((k_sc_vx<2, 1>), grid, blk, 0, s, descs, tiles, ai, F, skinsat);
  else return -1;
  return 0;
}

int launch_sc_h(hipStream_t s, const ScDesc *descs, int n, int chunks, int lds, const int32_t *ai) {
  if (n <= 0 || chunks <= 0) return 0;
  if (lds > kHmMaxLds) return -1;
  hipLaunchKernelGGL(k_sc_hmfma, dim3(n, chunks), dim3(kPrepThreads), lds, s, descs, ai);
  return 0;
}
int launch_sc_skinsat(hipStream_t s, uint16_t *table, const ScParamsDev &P) {
  hipLaunchKernelGGL(k_sc_skinsat, dim3(1u << 16), dim3(256), 0, s, table, P);
  return 0;
}
int launch_sc_fz(hipStream_t s, const ScDesc *descs, int n, int lds, const int32_t *ai, const ScParamsDev &P,
                 const uint16_t *skinsat) {
  if (n <= 0) return 0;
  if (lds > kFzMaxLds || !skinsat) return -1;
  hipLaunchKernelGGL(k_sc_fz, dim3(n), dim3(kFzThreads), lds, s, descs, ai, P, skinsat);
  return 0;
}
int launch_sc_fd(hipStream_t s, const ScDesc *descs, int n, int lds, const int32_t *ai, const ScParamsDev &P,
                 const uint16_t *skinsat) {
  if (n <= 0) return 0;
  if (lds > kFdMaxLds || !skinsat) return -1;
  hipLaunchKernelGGL(k_sc_fd, dim3(n), dim3(kFdThreads), lds, s, descs, ai, P, skinsat);
  return 0;
}
int launch_sc_vq(hipStream_t s, const ScDesc *descs, int n, int chunks, int lds, const int32_t *ai,
                 const ScParamsDev &P) {
  if (n <= 0) return 0;
  if (lds > kPrepMaxLds) return -1;
  hipLaunchKernelGGL(k_sc_vq, dim3(n, chunks), dim3(kPrepThreads), lds, s, descs, ai, P);
  return 0;
}
int launch_sc_v(hipStream_t s, const ScDesc *descs, int n, int chunks, int lds, const int32_t *ai,
                const ScParamsDev &P) {
  if (n <= 0) return 0;
  if (lds > kPrepMaxLds) return -1;
  hipLaunchKernelGGL(k_sc_vmaps, dim3(n, chunks), dim3(kPrepThreads), lds, s, descs, ai, P);
  return 0;
}

}  // namespace fi
