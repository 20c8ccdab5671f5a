// fi_jpeg_enc.hip -- baseline JPEG encode on the GPU, byte-identical with
// libjpeg-turbo through Pillow 12.2.0's Image.save(buf, "JPEG", quality=q,
// subsampling=s, restart_marker_rows=1): the mirror image of fi_jpeg.hip.
// One restart interval per MCU row makes the entropy coder parallel (every
// interval is byte aligned and starts from DC prediction 0).
//
//   host     (fi_jpeg_write.cpp) quantisation tables, the Annex K Huffman
//            tables as encoding tables, the header bytes SOI..SOS;
//   k_jpeg_fdct   one thread per 8x8 block, in MCU order: reads the source
//            pixels (clamped coordinates, no padded copy), jccolor.c RGB ->
//            YCbCr, jcsample.c h2v2_downsample, level shift, jfdctint.c
//            jpeg_fdct_islow, jcdctmgr.c quantize -> int16 blocks in zigzag
//            order, and the bits the block's AC symbols will take;
//   k_jpeg_henc   one wave per restart interval, a lane per block, 64 blocks
//            at a time: DC difference against the component's previous block,
//            wave prefix sum of the block bit lengths, every lane ORs its
//            block's codes (jchuff.c encode_one_block) into an LDS bit buffer at
//            its offset; then a dword of the buffer per lane: a second prefix
//            sum over the 0xFF bytes places the stuffed zeros on the way to the
//            interval's worst-case slot; 1-bit padding, RSTn;
//   k_jpeg_scan + k_jpeg_pack   exclusive scan of the interval lengths (with
//            the headers and EOIs) over the batch, then one workgroup per
//            interval copies its slot behind the image's header into one
//            contiguous stream, which the host fetches with one copy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fi_enc_batch.h"
#include "fi_enc_dev.h"
#include "fi_enc_pack.h"
#include "fi_internal.h"
#include "fi_jpeg_enc.h"
#include "fi_jpeg_enc_dev.h"

namespace fi {

struct JpegEncIv {       // one restart interval = one MCU row
  int32_t img, row;
};

constexpr int kEncWords = 64 * kJpegEncBlockBytes / 4 + 8;  // LDS bit buffer: 64 blocks + the carried byte + slack

#define FI_HD __host__ __device__ __forceinline__

FI_HD int jpeg_imin(int a, int b) { return a < b ? a : b; }
FI_HD int jpeg_imax(int a, int b) { return a > b ? a : b; }
FI_HD int jpeg_enc_nbits(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

// (Y, Cb, Cr)[comp] of the source pixel (x, y), both clamped by the caller
FI_HD int jpeg_enc_sample(const uint8_t *p, int C, int comp) {
  if (C == 1) return p[0];
  const int r = p[0], g = p[1], b = p[2];
  // jccolor.c rgb_ycc_convert: FIX(x) = (int)(x * 65536 + 0.5); CBCR_OFFSET + ONE_HALF - 1
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Block `k` of MCU (mx, my): samples, FDCT, quantisation.  out = 64 int16 in
// zigzag order; returns the bits of the block's AC symbols.  qts: the batch's
// table pairs, aclen: code lengths of the two AC tables (luminance, chrominance).
FI_HD int jpeg_enc_block(const JpegEncDesc &D, const uint16_t *__restrict__ qts, const uint8_t *aclen, int mx, int my,
                         int k, int16_t *__restrict__ out) {
  const int W = D.W, H = D.H, C = D.C;
  int comp = 0, bx = mx, by = my;
  bool dummy = false;
  if (D.bpm == 3) comp = k;
  if (D.bpm == 6) {
    if (k >= 4) {
      comp = k - 3;
    } else {
      // jccoefct.c compress_data: luma blocks wholly beyond the image are
      // dummies -- AC 0, DC of the block before them in MCU order
      const bool right = 2 * mx + 1 >= (W + 7) / 8, bottom = 2 * my + 1 >= (H + 7) / 8;
      int s = k;
      if (k == 1 && right) s = 0;
      if (k >= 2 && bottom) s = right ? 0 : 1;
      if (k == 3 && !bottom && right) s = 2;
      dummy = s != k;
      bx = 2 * mx + (s & 1);
      by = 2 * my + (s >> 1);
    }
  }
  int d[64];
  if (D.bpm == 6 && comp) {
    // jcsample.c h2v2_downsample: bias 1, 2, 1, 2, ... by output column.  Right
    // edge: full-resolution pixels replicated.  Bottom edge: full-resolution
    // rows are replicated to an even count only; below that the downsampled
    // last row repeats (jcprepct.c pads the *output* to the iMCU height).
    const int ch = (H + 1) / 2;
#pragma unroll
    for (int y = 0; y < 8; y++) {
      const int cy = jpeg_imin(by * 8 + y, ch - 1);
      const uint8_t *r0 = D.src + (int64_t)jpeg_imin(2 * cy, H - 1) * D.stride;
      const uint8_t *r1 = D.src + (int64_t)jpeg_imin(2 * cy + 1, H - 1) * D.stride;
#pragma unroll
      for (int x = 0; x < 8; x++) {
        const int cx = bx * 8 + x;
        const int x0 = jpeg_imin(2 * cx, W - 1) * C, x1 = jpeg_imin(2 * cx + 1, W - 1) * C;
        const int s = jpeg_enc_sample(r0 + x0, C, comp) + jpeg_enc_sample(r0 + x1, C, comp) +
                      jpeg_enc_sample(r1 + x0, C, comp) + jpeg_enc_sample(r1 + x1, C, comp);
        d[8 * y + x] = ((s + 1 + (x & 1)) >> 2) - 128;
      }
    }
  } else {
#pragma unroll
    for (int y = 0; y < 8; y++) {
      const uint8_t *r = D.src + (int64_t)jpeg_imin(by * 8 + y, H - 1) * D.stride;
#pragma unroll
      for (int x = 0; x < 8; x++) d[8 * y + x] = jpeg_enc_sample(r + jpeg_imin(bx * 8 + x, W - 1) * C, C, comp) - 128;
    }
  }
  // jfdctint.c jpeg_fdct_islow: CONST_BITS 13, PASS1_BITS 2
  constexpr int CB = 13, P1 = 2;
  constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const int st = pass ? 8 : 1, adv = pass ? 1 : 8;  // rows, then columns
    const int S = pass ? CB + P1 : CB - P1, R = 1 << (S - 1);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      int *p = d + i * adv;
      int tmp0 = p[0] + p[7 * st], tmp7 = p[0] - p[7 * st];
      int tmp1 = p[st] + p[6 * st], tmp6 = p[st] - p[6 * st];
      int tmp2 = p[2 * st] + p[5 * st], tmp5 = p[2 * st] - p[5 * st];
      int tmp3 = p[3 * st] + p[4 * st], tmp4 = p[3 * st] - p[4 * st];
      const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
      if (pass == 0) {
        p[0] = (tmp10 + tmp11) * (1 << P1);
        p[4 * st] = (tmp10 - tmp11) * (1 << P1);
      } else {
        p[0] = (tmp10 + tmp11 + (1 << (P1 - 1))) >> P1;
        p[4 * st] = (tmp10 - tmp11 + (1 << (P1 - 1))) >> P1;
      }
      int z1 = (tmp12 + tmp13) * F0541;
      p[2 * st] = (z1 + tmp13 * F0765 + R) >> S;
      p[6 * st] = (z1 + tmp12 * (-F1847) + R) >> S;
      z1 = tmp4 + tmp7;
      int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
      const int z5 = (z3 + z4) * F1175;
      tmp4 *= F0298;
      tmp5 *= F2053;
      tmp6 *= F3072;
      tmp7 *= F1501;
      z1 *= -F0899;
      z2 *= -F2562;
      z3 *= -F1961;
      z4 *= -F0390;
      z3 += z5;
      z4 += z5;
      p[7 * st] = (tmp4 + z1 + z3 + R) >> S;
      p[5 * st] = (tmp5 + z2 + z4 + R) >> S;
      p[3 * st] = (tmp6 + z2 + z3 + R) >> S;
      p[st] = (tmp7 + z1 + z4 + R) >> S;
    }
  }
  // jcdctmgr.c quantize: divisor = table << 3, round half away from zero;
  // jchuff.c encode_one_block's AC symbols counted on the way
  constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  const uint16_t *q = qts + (int64_t)D.qt * 128 + (comp ? 64 : 0);
  const uint8_t *al = aclen + (comp ? 256 : 0);
  int bits = 0, run = 0;
#pragma unroll
  for (int z = 0; z < 64; z++) {
    const int c = d[zz[z]], div = (int)q[zz[z]] << 3;
    const int a = ((c < 0 ? -c : c) + (div >> 1)) / div;
    const int v = dummy && z ? 0 : (c < 0 ? -a : a);
    out[z] = (int16_t)v;
    if (z) {
      if (v == 0) {
        run++;
      } else {
        const int s = jpeg_enc_nbits((uint32_t)(v < 0 ? -v : v));
        bits += (run >> 4) * al[0xF0] + al[((run & 15) << 4) | s] + s;
        run = 0;
      }
    }
  }
  if (run) bits += al[0];
  return bits;
}

// MSB-first bit writer into a zeroed word buffer other writers OR into as well
struct JpegBitW {
  uint32_t *buf;
  uint32_t cw;
  int wi, fill;
  FI_HD void flush() {
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(&buf[wi], cw);
#else
    buf[wi] |= cw;
#endif
  }
  FI_HD void init(uint32_t *b, int bit) {
    buf = b;
    wi = bit >> 5;
    fill = bit & 31;
    cw = 0;
  }
  FI_HD void put(uint32_t code, int len) {  // len <= 32, code < 2^len
    if (!len) return;
    const int room = 32 - fill;
    if (len < room) {
      cw |= code << (room - len);
      fill += len;
    } else {
      cw |= code >> (len - room);
      flush();
      wi++;
      fill = len - room;
      cw = fill ? code << (32 - fill) : 0u;
    }
  }
  FI_HD void finish() {
    if (fill) flush();
  }
};

// the DC symbol of a difference: (code and value bits, their length)
FI_HD uint32_t jpeg_enc_dc(const uint32_t *tab, int diff, int *len) {
  const int s = jpeg_enc_nbits((uint32_t)(diff < 0 ? -diff : diff));
  const uint32_t e = tab[s];
  const uint32_t v = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u);
  *len = (int)(e >> 16) + s;
  return ((e & 0xFFFFu) << s) | v;
}

// jchuff.c encode_one_block; dct / act: the component's DC / AC tables
template <typename TAB>
FI_HD void jpeg_enc_emit(JpegBitW &bw, const TAB *dct, const TAB *act, const int16_t *__restrict__ blk, int pdc) {
  int len;
  const uint32_t dc = jpeg_enc_dc(dct, (int)blk[0] - pdc, &len);
  bw.put(dc, len);
  int run = 0;
  for (int z = 1; z < 64; z++) {
    const int v = blk[z];
    if (v == 0) {
      run++;
      continue;
    }
    for (; run > 15; run -= 16) bw.put(act[0xF0] & 0xFFFFu, (int)(act[0xF0] >> 16));
    const int s = jpeg_enc_nbits((uint32_t)(v < 0 ? -v : v));
    const uint32_t e = act[(run << 4) | s];
    bw.put(((e & 0xFFFFu) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (int)(e >> 16) + s);
    run = 0;
  }
  if (run) bw.put(act[0] & 0xFFFFu, (int)(act[0] >> 16));
  bw.finish();
}

// component of block j of an interval, and the component's previous block (-1: none)
FI_HD int jpeg_enc_comp(int bpm, int j, int *prev) {
  if (bpm == 1) {
    *prev = j - 1;
    return 0;
  }
  const int k = j % bpm;
  if (bpm == 3) {
    *prev = j - 3;
    return k;
  }
  *prev = k >= 4 ? j - 6 : k ? j - 1 : j - 3;  // Y: the MCU's previous block, or the previous MCU's fourth
  return k >= 4 ? k - 3 : 0;
}

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------
// (grid-stride: a dispatch's work-item count is 32-bit, see k_jpeg_idct)
__global__ __launch_bounds__(256) void k_jpeg_fdct(const JpegEncDesc *__restrict__ descs, int nimg, int64_t nblocks,
                                                   const uint16_t *__restrict__ qts, const uint32_t *__restrict__ huff,
                                                   int16_t *__restrict__ coef, uint16_t *__restrict__ acbits) {
  __shared__ uint8_t aclen[512];  // code lengths of the luminance / chrominance AC tables
  for (int i = threadIdx.x; i < 512; i += 256) aclen[i] = (uint8_t)(huff[256 + 512 * (i >> 8) + (i & 255)] >> 16);
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nblocks; i += (int64_t)gridDim.x * 256) {
    const JpegEncDesc D = descs[enc_find_image(descs, nimg, i, &JpegEncDesc::blk0)];
    const int64_t b = i - D.blk0;
    const int mcu = (int)(b / D.bpm), k = (int)(b - (int64_t)mcu * D.bpm);
    const int my = mcu / D.mcux, mx = mcu - my * D.mcux;
    __attribute__((aligned(16))) int16_t o[64];
    const int bits = jpeg_enc_block(D, qts, aclen, mx, my, k, o);
    uint4 *dst = reinterpret_cast<uint4 *>(coef + i * 64);
#pragma unroll
    for (int t = 0; t < 8; t++) dst[t] = reinterpret_cast<const uint4 *>(o)[t];
    acbits[i] = (uint16_t)bits;
  }
}

void jpeg_enc_launch_fdct(hipStream_t st, const JpegEncDesc *descs, int nimg, int64_t nblocks, const uint16_t *qts,
                          const uint32_t *huff, int16_t *coef, uint16_t *acbits) {
  hipLaunchKernelGGL(k_jpeg_fdct, dim3((unsigned)std::min<int64_t>((nblocks + 255) / 256, 1 << 20)), dim3(256), 0, st,
                     descs, nimg, nblocks, qts, huff, coef, acbits);
}

__global__ __launch_bounds__(64) void k_jpeg_henc(const JpegEncDesc *__restrict__ descs,
                                                  const JpegEncIv *__restrict__ ivs, int niv,
                                                  const uint32_t *__restrict__ huff, const int16_t *__restrict__ coef,
                                                  const uint16_t *__restrict__ acbits, uint8_t *__restrict__ slots,
                                                  int32_t *__restrict__ ivlen) {
  __shared__ uint32_t tab[1024];
  __shared__ uint32_t bits[kEncWords];
  const int lane = threadIdx.x;
  for (int i = lane; i < 1024; i += 64) tab[i] = huff[i];
  const int iv = blockIdx.x;
  if (iv >= niv) return;
  const JpegEncIv I = ivs[iv];
  const JpegEncDesc D = descs[I.img];
  const int bpm = D.bpm, nb = D.mcux * bpm;
  const int64_t b0 = D.blk0 + (int64_t)I.row * nb;
  uint8_t *out = slots + D.slot0 + (int64_t)I.row * D.slot_bytes;
  const int64_t cap = D.slot_bytes - 2;  // (the bound holds by construction; no store leaves the slot regardless)
  int outpos = 0;          // bytes written to the slot (wave-uniform)
  int carry_bits = 0;      // bits of the last, incomplete byte carried into the next chunk
  uint32_t carry_word = 0; // that byte, in the top bits
  for (int c0 = 0; c0 < nb; c0 += 64) {
    __syncthreads();
    for (int i = lane; i < kEncWords; i += 64) bits[i] = i ? 0u : carry_word;
    __syncthreads();
    const int j = c0 + lane;
    const bool on = j < nb;
    int len = 0, pdc = 0, comp = 0;
    if (on) {
      int prev;
      comp = jpeg_enc_comp(bpm, j, &prev);
      pdc = prev >= 0 ? coef[(b0 + prev) * 64] : 0;
      int dl;
      (void)jpeg_enc_dc(tab + (comp ? 512 : 0), (int)coef[(b0 + j) * 64] - pdc, &dl);
      len = dl + acbits[b0 + j];
    }
    const int incl = enc_scan64(len);
    int total = carry_bits + __shfl(incl, 63, 64);
    if (on) {
      JpegBitW bw;
      bw.init(bits, carry_bits + incl - len);
      jpeg_enc_emit(bw, tab + (comp ? 512 : 0), tab + (comp ? 768 : 256), coef + (b0 + j) * 64, pdc);
    }
    __syncthreads();
    const bool last = c0 + 64 >= nb;
    if (last && (total & 7)) {  // pad the interval's last byte with 1-bits
      const int pad = 8 - (total & 7);
      if (lane == 0) bits[total >> 5] |= ((1u << pad) - 1u) << (32 - (total & 31) - pad);
      total += pad;
      __syncthreads();
    }
    const int nbytes = total >> 3;
    // bytes -> slot, a dword of the buffer per lane; every 0xFF is followed by a stuffed 0
    int ffs = 0;  // 0xFF bytes of the chunk so far (wave-uniform)
    for (int w0 = 0; w0 * 4 < nbytes; w0 += 64) {
      const int w = w0 + lane;
      const int nv = jpeg_imin(4, jpeg_imax(0, nbytes - 4 * w));
      const uint32_t word = nv ? bits[w] : 0u;
      int nff = 0;
      for (int t = 0; t < nv; t++) nff += ((word >> (24 - 8 * t)) & 255u) == 255u;
      const int incl_ff = enc_scan64(nff);
      int64_t o = (int64_t)outpos + 4 * w + ffs + (incl_ff - nff);
      for (int t = 0; t < nv; t++) {
        const uint8_t b = (uint8_t)(word >> (24 - 8 * t));
        if (o < cap) out[o] = b;
        o++;
        if (b == 255u) {
          if (o < cap) out[o] = 0;
          o++;
        }
      }
      ffs += __shfl(incl_ff, 63, 64);
    }
    outpos += nbytes + ffs;
    carry_bits = total & 7;
    carry_word = carry_bits ? ((bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u) << 24 : 0u;
  }
  if (I.row != D.mcuy - 1) {  // RSTn
    if (lane == 0 && outpos <= cap) {
      out[outpos] = 0xFF;
      out[outpos + 1] = (uint8_t)(0xD0 + (I.row & 7));
    }
    outpos += 2;
  }
  if (lane == 0) ivlen[iv] = (int32_t)(outpos < D.slot_bytes ? outpos : D.slot_bytes);
}

// Exclusive scan, over the batch's intervals, of the bytes each contributes to
// the packed stream: its slot's length, the image's header before its first
// interval and EOI after its last.  One workgroup.  ivdst[iv] = where the
// contribution starts; imgpos[2 i] / [2 i + 1] = start / end of image i.
__global__ __launch_bounds__(256) void k_jpeg_scan(const JpegEncDesc *__restrict__ descs,
                                                   const JpegEncIv *__restrict__ ivs, int niv,
                                                   const int32_t *__restrict__ ivlen, int64_t *__restrict__ ivdst,
                                                   int64_t *__restrict__ imgpos) {
  enc_scan_items(
      niv,
      [=](int iv) {
        const JpegEncIv I = ivs[iv];
        const bool first = I.row == 0, last = I.row == descs[I.img].mcuy - 1;
        return EncItem{ivlen[iv] + (first ? descs[I.img].hdr_len : 0) + (last ? 2 : 0), I.img, first, last};
      },
      ivdst, imgpos);
}

// one workgroup per interval: header (first interval), slot, EOI (last) -> packed
__global__ __launch_bounds__(256) void k_jpeg_pack(const JpegEncDesc *__restrict__ descs,
                                                   const JpegEncIv *__restrict__ ivs, int niv,
                                                   const int32_t *__restrict__ ivlen,
                                                   const int64_t *__restrict__ ivdst, const uint8_t *__restrict__ hdrs,
                                                   const uint8_t *__restrict__ slots, uint8_t *__restrict__ packed) {
  const int iv = blockIdx.x, t = threadIdx.x;
  if (iv >= niv) return;
  const JpegEncIv I = ivs[iv];
  const JpegEncDesc &D = descs[I.img];
  uint8_t *dst = packed + ivdst[iv];
  if (I.row == 0) {
    const uint8_t *h = hdrs + D.hdr_off;
    for (int i = t; i < D.hdr_len; i += 256) dst[i] = h[i];
    dst += D.hdr_len;
  }
  const uint8_t *s = slots + D.slot0 + (int64_t)I.row * D.slot_bytes;
  const int n = ivlen[iv];
  enc_copy_aligned(dst, s, n, t, 256);
  if (I.row == D.mcuy - 1 && t == 0) {  // EOI
    dst[n] = 0xFF;
    dst[n + 1] = 0xD9;
  }
}

// ---------------------------------------------------------------------------
// host: batch plan + launches
// ---------------------------------------------------------------------------
// Plans and runs one encode batch.  `alloc(which, bytes)` returns memory that
// stays valid until the stream has run: 0 device upload (tables, descriptors,
// headers), 1 device work (coefficients, slots, lengths), 2 the packed
// streams, 3 pinned host staging (asked for twice: the upload, then -- after
// the stream has run -- the download).  `stage(name)` brackets the kernels for
// the caller's timing (nullptr: the end of the last one).
int jpeg_encode_batch(hipStream_t st, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                      const int32_t *channels, const int64_t *src_stride, const int32_t *quality,
                      const int32_t *subsampling, int n, uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                      int32_t *status, void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *),
                      void *actx, std::string *err) {
  std::vector<JpegEncDesc> descs;
  std::vector<int> desc_img;
  std::vector<JpegEncIv> ivs;
  JpegEncQts qts;
  std::vector<uint8_t> hdrs;
  int64_t nblocks = 0;
  size_t slot_total = 0, bound_total = 0;
  for (int i = 0; i < n; i++) {
    out_len[i] = 0;
    status[i] = enc_io_status(jpeg_enc_check(w[i], h[i], channels[i], quality[i], subsampling[i]), src[i],
                              src_stride[i], w[i], channels[i], out[i], out_cap[i]);
    if (status[i]) continue;
    JpegEncDesc D =
        jpeg_enc_desc(src[i], src_stride[i], w[i], h[i], channels[i], quality[i], subsampling[i], nblocks, &qts);
    D.iv0 = (int)ivs.size();
    D.slot0 = (int64_t)slot_total;
    D.slot_bytes = (int64_t)((jpeg_enc_slot_bytes(D.bpm, D.mcux) + 15) & ~(size_t)15);
    D.hdr_off = (int32_t)hdrs.size();
    jpeg_enc_write_header(D.W, D.H, D.C, quality[i], subsampling[i], &hdrs);
    D.hdr_len = (int32_t)hdrs.size() - D.hdr_off;
    if ((size_t)ivs.size() + D.mcuy > (size_t)1 << 30 || hdrs.size() > (size_t)1 << 30) {
      *err = "JPEG encode batch too large";
      return FI_EINVAL;
    }
    for (int r = 0; r < D.mcuy; r++) ivs.push_back({(int32_t)descs.size(), r});
    nblocks += (int64_t)D.bpm * D.mcux * D.mcuy;
    slot_total += (size_t)D.slot_bytes * D.mcuy;
    size_t bnd = 0;
    (void)jpeg_enc_bound(D.W, D.H, D.C, quality[i], subsampling[i], &bnd);
    bound_total += bnd;
    descs.push_back(D);
    desc_img.push_back(i);
  }
  if (descs.empty()) return 0;
  const int nd = (int)descs.size(), niv = (int)ivs.size();
  // upload: descriptors, intervals, quantisation tables, Huffman tables, headers
  uint32_t huff[1024];
  jpeg_enc_huff_tables(huff);
  EncArena up, work;
  const size_t o_desc = up.add(descs.size() * sizeof(JpegEncDesc));
  const size_t o_iv = up.add(ivs.size() * sizeof(JpegEncIv));
  const size_t o_qt = up.add(qts.tabs.size() * 2);
  const size_t o_huff = up.add(sizeof(huff));
  const size_t o_hdr = up.add(hdrs.size());
  const size_t up_total = up.total();
  // work: coefficients, AC bit counts, interval lengths / destinations, image positions, slots
  const size_t k_coef = work.add((size_t)nblocks * 128);
  const size_t k_bits = work.add((size_t)nblocks * 2);
  const size_t k_ivlen = work.add((size_t)niv * 4);
  const size_t k_ivdst = work.add((size_t)niv * 8);
  const size_t k_pos = work.add((size_t)nd * 16);
  const size_t k_slots = work.add(slot_total);
  const size_t work_total = work.total();
  uint8_t *dup = (uint8_t *)alloc(actx, 0, up_total);
  uint8_t *hst = (uint8_t *)alloc(actx, 3, std::max(up_total, (size_t)nd * 16));
  uint8_t *dwork = (uint8_t *)alloc(actx, 1, work_total);
  uint8_t *dpack = (uint8_t *)alloc(actx, 2, bound_total);
  if (!dup || !hst || !dwork || !dpack) {
    *err = "memory for the JPEG encode batch";
    return FI_ENOMEM;
  }
  memcpy(hst + o_desc, descs.data(), descs.size() * sizeof(JpegEncDesc));
  memcpy(hst + o_iv, ivs.data(), ivs.size() * sizeof(JpegEncIv));
  memcpy(hst + o_qt, qts.tabs.data(), qts.tabs.size() * 2);
  memcpy(hst + o_huff, huff, sizeof(huff));
  memcpy(hst + o_hdr, hdrs.data(), hdrs.size());
  if (hipMemcpyAsync(dup, hst, up_total, hipMemcpyHostToDevice, st) != hipSuccess) {
    *err = "JPEG encode batch upload";
    return FI_EDEVICE;
  }
  const JpegEncDesc *dd = (const JpegEncDesc *)(dup + o_desc);
  const JpegEncIv *div = (const JpegEncIv *)(dup + o_iv);
  const uint32_t *dhuff = (const uint32_t *)(dup + o_huff);
  int16_t *dcoef = (int16_t *)(dwork + k_coef);
  uint16_t *dbits = (uint16_t *)(dwork + k_bits);
  int32_t *divlen = (int32_t *)(dwork + k_ivlen);
  int64_t *divdst = (int64_t *)(dwork + k_ivdst);
  int64_t *dpos = (int64_t *)(dwork + k_pos);
  stage(actx, "k_jpeg_fdct");
  jpeg_enc_launch_fdct(st, dd, nd, nblocks, (const uint16_t *)(dup + o_qt), dhuff, dcoef, dbits);
  stage(actx, "k_jpeg_henc");
  hipLaunchKernelGGL(k_jpeg_henc, dim3((unsigned)niv), dim3(64), 0, st, dd, div, niv, dhuff, dcoef, dbits,
                     dwork + k_slots, divlen);
  stage(actx, "k_jpeg_pack");
  hipLaunchKernelGGL(k_jpeg_scan, dim3(1), dim3(256), 0, st, dd, div, niv, divlen, divdst, dpos);
  hipLaunchKernelGGL(k_jpeg_pack, dim3((unsigned)niv), dim3(256), 0, st, dd, div, niv, divlen, divdst, dup + o_hdr,
                     dwork + k_slots, dpack);
  stage(actx, nullptr);
  return enc_finish(st, alloc, actx, hst, dpos, nd, nullptr, dpack, bound_total, "JPEG", desc_img, out, out_cap, out_len,
                    status, true, err);
}
}  // namespace fi
