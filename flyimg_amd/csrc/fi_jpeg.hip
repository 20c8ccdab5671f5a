// fi_jpeg.hip -- baseline JPEG decode on the GPU, bit-exact with the
// libjpeg-turbo decoder the host codec path uses (Pillow 12.2.0 bundles
// libjpeg-turbo 3.x; SURVEY.md 8(f) 1: "nvJPEG-style batched decode").
//
//   host     marker parse (SOF0/SOF1 8-bit, DQT, DHT, DRI, one SOS), canonical
//            Huffman tables deduplicated over the batch, restart intervals
//            located by their RSTn markers;
//   k_jpeg_huff   one 64-lane workgroup per restart interval (the whole scan
//            when there is none), the lanes in lockstep on wave-uniform state,
//            the segment window spread over the lanes: jdhuff.c's sequential decode -- DC prediction, AC run /
//            size symbols, HUFF_EXTEND -- into int16 coefficient blocks in
//            zigzag order (the IDCT reads them back in natural order); byte stuffing and markers as jdhuff.c (a marker
//            feeds zero bits);
//   k_jpeg_idct   one thread per 8x8 block: jidctint.c jpeg_idct_islow
//            (dequantise, 13-bit constants, PASS1_BITS 2, range limit);
//   k_jpeg_color  one thread per output pixel: jdsample.c fancy upsampling
//            (h2v1 / h2v2 triangle filters, edge replication) and jdcolor.c
//            ycc_rgb_convert with its 16-bit fixed-point tables;
//   k_jpeg_color_view  the same stage for the images decoded through a view
//            (fi_jpeg_decode_device_view: an EXIF orientation and a rectangle
//            of the oriented image), one workgroup per 32x32 output tile, the
//            transposing orientations through LDS.
//
// Unsupported streams (progressive, arithmetic, 12-bit, CMYK / Adobe
// transforms, other samplings, several scans, restart markers out of
// sequence) return FI_EUNSUPPORTED from jpeg_parse so the caller decodes them
// on the host.  Corrupt entropy data is decoded as libjpeg decodes it (data
// that runs out: BitReader::short_of_data); where that is not worth restating
// (coefficients beyond the range in which libjpeg's SIMD IDCT equals
// jidctint.c, a progressive symbol stored outside its scan's band) a kernel
// raises the image's handover flag, read back as FI_EUNSUPPORTED.
//
// Opt-in (FI_JPEG_PROGRESSIVE): complete Huffman progressive (SOF2) streams.
//   host     every SOS up to EOI into a scan list (the tables and DRI in force
//            at each), libjpeg's progression checks; each scan gets a level --
//            1 + the highest level of an earlier scan sharing a component over
//            an overlapping band -- and is cut into restart intervals;
//   k_jpeg_prog   one launch per level, one 64-lane workgroup per (image,
//            scan, restart interval): jdphuff.c's DC / AC first and refinement
//            procedures (fi_jpeg_prog.h, shared with the host decoder of
//            fi_jpeg_prog_host.cpp) into the zeroed coefficient planes;
//   then the same k_jpeg_idct and k_jpeg_color launches as the baseline
//   images of the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "fi_internal.h"
#include "fi_jpeg.h"
#include "fi_jpeg_prog.h"
#include "fi_jpeg_view.h"

namespace fi {

// ---------------------------------------------------------------------------
// device: Huffman decode
// ---------------------------------------------------------------------------
constexpr int kJpegLdsTabs = 8;  // distinct Huffman tables staged in LDS (more: read from global)

typedef __attribute__((address_space(1))) const uint32_t g_u32;
// All 64 lanes of the workgroup decode the same interval in lockstep (the
// values are wave-uniform, so no lane diverges): the 256-byte window of the
// segment is spread over the lanes, lane i holding bytes [wbase + 4 i, + 4),
// read with v_readlane; the next 256 bytes are in flight in `nxt` (their
// latency hides behind the decode of the current window).  The segment is
// zero padded by >= 512 bytes.
// `fake` counts the zero bits supplied after a marker or the end of the data
// (they sit below the real ones): once nbits < fake a request went beyond the
// real bits, which is when jdhuff.c sets insufficient_data; fills add to both
// counts alike, so the condition holds from then on.  libjpeg finishes that
// MCU from the zero bits and leaves the later MCUs of the interval zero.
struct BitReader {
  const uint8_t *p;
  uint32_t win, nxt;
  int wbase, pos, end;
  uint64_t buf;
  int nbits, fake;
  bool marker;
  __device__ __forceinline__ bool short_of_data() const { return nbits < fake; }
  __device__ __forceinline__ void advance_window() {
    if (pos - wbase >= 256) {  // bytes [pos, pos + 4) stay inside win + the first dword of nxt
      win = nxt;
      wbase += 256;
      nxt = *(g_u32 *)(p + wbase + 256 + 4 * (threadIdx.x & 63));
    }
  }
  // the 4 bytes at pos, little-endian
  __device__ __forceinline__ uint32_t word_at_pos() const {
    const int o = __builtin_amdgcn_readfirstlane(pos - wbase), k = o >> 2;
    const uint32_t lo = __builtin_amdgcn_readlane(win, k);
    const uint32_t hi = k < 63 ? __builtin_amdgcn_readlane(win, k + 1) : __builtin_amdgcn_readfirstlane(nxt);
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(o & 3));
  }
  __device__ void init(const uint8_t *ecs, int byte0, int len) {
    p = ecs;
    wbase = byte0 & ~255;
    win = *(g_u32 *)(p + wbase + 4 * (threadIdx.x & 63));
    nxt = *(g_u32 *)(p + wbase + 256 + 4 * (threadIdx.x & 63));
    pos = byte0;
    end = len;
    buf = 0;
    nbits = 0;
    fake = 0;
    marker = false;
  }
  // jdhuff.c jpeg_fill_bit_buffer: stuffed 0xFF00 -> 0xFF; at a marker (or the
  // end of the data) zero bits are supplied.  Called once per symbol: leaves
  // >= 32 bits, enough for a code (<= 16) and its value bits (<= 16); four
  // bytes at a time while they hold no 0xFF, else byte by byte.
  __device__ __forceinline__ void fill() {
    if (nbits >= 32) return;
    const uint32_t w = word_at_pos();
    const uint32_t t = ~w;
    const bool ff = ((t - 0x01010101u) & ~t & 0x80808080u) != 0u;  // some byte of w is 0xFF
    if (!ff && !marker && pos + 4 <= end) {
      buf = (buf << 32) | __builtin_bswap32(w);
      nbits += 32;
      pos += 4;
      advance_window();
      return;
    }
    while (nbits < 32) {
      uint32_t b = 0;
      if (!marker && pos < end) {
        const uint32_t x = word_at_pos();
        b = x & 255u;
        if (b == 0xFFu) {
          if (((x >> 8) & 255u) == 0u) {
            pos += 2;
          } else {
            marker = true;
            b = 0;
            fake += 8;
          }
        } else {
          pos++;
        }
        advance_window();
      } else {
        fake += 8;
      }
      buf = (buf << 8) | b;
      nbits += 8;
    }
  }
  __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)(buf >> (nbits - n)) & ((1u << n) - 1u); }
  __device__ __forceinline__ void skip(int n) { nbits -= n; }
};

template <typename TAB>
__device__ __forceinline__ int jpeg_decode_sym(BitReader &br, const TAB *t) {
  br.fill();
  const uint32_t lk = t->look[br.peek(9)];
  if (lk) {
    br.skip(lk >> 8);
    return lk & 255;
  }
  int l = 10;
  int32_t code = (int32_t)br.peek(10);
  while (l <= 16 && code > t->maxcode[l]) {
    l++;
    code = (int32_t)br.peek(l);
  }
  if (l > 16) {  // corrupt data: jdhuff.c warns and returns 0, the 17 bits it tried consumed
    br.skip(17);
    return 0;
  }
  br.skip(l);
  return t->huffval[(code + t->valoff[l]) & 255];
}
__device__ __forceinline__ int jpeg_extend(uint32_t r, int s) {  // HUFF_EXTEND
  return r < (1u << (s - 1)) ? (int)r - (1 << s) + 1 : (int)r;
}

template <bool LDS>
__global__ __launch_bounds__(64) void k_jpeg_huff(const JpegDesc *__restrict__ descs,
                                                  const JpegInterval *__restrict__ ivs, int niv,
                                                  const JpegHuff *__restrict__ huff, int nhuff,
                                                  uint8_t *__restrict__ work) {
  __shared__ JpegHuff sh[kJpegLdsTabs];
  __shared__ __attribute__((aligned(16))) int16_t blk[64];
  const int tid = threadIdx.x;
  if (LDS) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(huff);
    uint32_t *dstw = reinterpret_cast<uint32_t *>(sh);
    const int nw = nhuff * (int)sizeof(JpegHuff) / 4;
    for (int i = tid; i < nw; i += 64) dstw[i] = src[i];
  }
  if (tid < 32) reinterpret_cast<uint32_t *>(blk)[tid] = 0;
  __syncthreads();
  const int iv = blockIdx.x;
  if (iv >= niv) return;
  const JpegInterval I = ivs[iv];
  const JpegDesc *Dp = descs + I.img;
  // the descriptor in registers (the block stores below may alias it for the
  // compiler: fields read through the pointer would be reloaded per block)
  const int ncomp = Dp->ncomp, mcux = Dp->mcux;
  int tdc[3], tac[3], hs[3], vs[3], bw[3];
  int64_t co[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const bool on = c < ncomp;
    tdc[c] = on ? Dp->ht[Dp->td[c]] : 0;
    tac[c] = on ? Dp->ht[2 + Dp->ta[c]] : 0;
    hs[c] = on ? Dp->h[c] : 0;
    vs[c] = on ? Dp->v[c] : 0;
    bw[c] = on ? Dp->bw[c] : 0;
    co[c] = on ? Dp->coef[c] : 0;
  }
  // the address space of the table reads is static: LDS reads (ds_read, ~100
  // cycles) or global ones, never flat pointers into either
  typedef __attribute__((address_space(3))) const JpegHuff l_huff;
  typedef __attribute__((address_space(1))) const JpegHuff g_huff;
  BitReader br;
  br.init(Dp->ecs, I.byte0, Dp->ecs_len);
  int pred[3] = {0, 0, 0};  // DC predictions (static indices only: registers)
  int16_t *b = blk;
  for (int mcu = I.mcu0; mcu < I.mcu1; mcu++) {
    const int my = mcu / mcux, mx = mcu - my * mcux;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (c >= ncomp) break;
      for (int by = 0; by < vs[c]; by++)
        for (int bx = 0; bx < hs[c]; bx++) {
          // DC: difference from the component's previous block
          int s = LDS ? jpeg_decode_sym(br, (l_huff *)(sh + tdc[c])) : jpeg_decode_sym(br, (g_huff *)(huff + tdc[c]));
          if (s) {  // (the symbol's fill left enough bits for its value)
            const uint32_t r = br.peek(s);
            br.skip(s);
            s = jpeg_extend(r, s);
          }
          pred[c] += s;
          b[0] = (int16_t)pred[c];
          // AC: run / size symbols
          for (int k = 1; k < 64; k++) {
            br.fill();
            const int fa = LDS ? ((l_huff *)(sh + tac[c]))->fast_ac[br.peek(9)]
                               : ((g_huff *)(huff + tac[c]))->fast_ac[br.peek(9)];
            if (fa) {  // code + value in one lookahead
              k += (fa >> 4) & 15;
              br.skip(fa & 15);
              b[k < 63 ? k : 63] = (int16_t)(fa >> 8);
              continue;
            }
            const int rs = LDS ? jpeg_decode_sym(br, (l_huff *)(sh + tac[c]))
                               : jpeg_decode_sym(br, (g_huff *)(huff + tac[c]));
            const int r = rs >> 4, sz = rs & 15;
            if (sz) {
              k += r;
              const uint32_t v = br.peek(sz);
              br.skip(sz);
              b[k < 63 ? k : 63] = (int16_t)jpeg_extend(v, sz);  // zigzag order (k > 63: jpeg_natural_order's guard -> 63)
            } else {
              if (r != 15) break;
              k += 15;
            }
          }
          // block -> work (lanes 0-7: 16 bytes each), and clear the staging block
          const int row = my * vs[c] + by, col = mx * hs[c] + bx;
          if (tid < 8) {
            uint4 *o = reinterpret_cast<uint4 *>(work + co[c] + ((int64_t)row * bw[c] + col) * 128);
            uint4 *bb = reinterpret_cast<uint4 *>(b);
            o[tid] = bb[tid];
            bb[tid] = uint4{0, 0, 0, 0};
          }
        }
    }
    if (!br.short_of_data()) continue;
    // jdhuff.c insufficient_data: this MCU was finished from zero bits; the
    // later ones of the interval stay zero (uniform grey)
    for (int m = mcu + 1; m < I.mcu1; m++) {
      const int zy = m / mcux, zx = m - zy * mcux;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (c >= ncomp) break;
        for (int by = 0; by < vs[c]; by++)
          for (int bx = 0; bx < hs[c]; bx++) {
            const int row = zy * vs[c] + by, col = zx * hs[c] + bx;
            if (tid < 8)
              reinterpret_cast<uint4 *>(work + co[c] + ((int64_t)row * bw[c] + col) * 128)[tid] = uint4{0, 0, 0, 0};
          }
      }
    }
    break;
  }
}

// ---------------------------------------------------------------------------
// device: progressive scans (jdphuff.c), one 64-lane workgroup per (image,
// scan, restart interval) of one level
// ---------------------------------------------------------------------------
// The block procedures are fi_jpeg_prog.h's (shared with the host decoder),
// over the lockstep BitReader.  Only the scan's own tables are staged in LDS
// (one AC table, or up to three DC tables).  Lane z works on coefficient z: a
// first-pass scan writes its band Ss .. Se of a staging block in LDS; a
// refinement scan loads the band into registers (the next block's is in flight
// while this one decodes) and runs on ballots of it.  Every scan stores its
// band only, one 2-byte store per lane -- two scans of one level may share a
// 128-byte block (Y 1-5 and Y 6-63).
struct JpegProgDevOps {
  template <typename TAB>
  static __device__ __forceinline__ int sym(BitReader &br, const TAB *t) {
    return jpeg_decode_sym(br, t);
  }
  // lane z looks up the bit of its own coefficient
  static __device__ __forceinline__ uint64_t deposit(uint64_t bits, int n, uint64_t m) {
    const int z = threadIdx.x & 63;
    const bool in = (m >> z) & 1;
    const int rank = __builtin_popcountll(m & (((uint64_t)1 << z) - 1));
    return __ballot(in && ((bits >> (in ? n - 1 - rank : 0)) & 1));
  }
};

__global__ __launch_bounds__(64) void k_jpeg_prog(const JpegDesc *__restrict__ descs,
                                                  const JpegProgItem *__restrict__ items, int nitems,
                                                  const JpegHuff *__restrict__ huff, uint8_t *__restrict__ work,
                                                  int32_t *__restrict__ handover) {
  __shared__ JpegHuff sh[3];
  __shared__ __attribute__((aligned(16))) int16_t blk[64];
  __shared__ int outside;  // set where corrupt data leaves the scan's band (kept out of the registers: rare)
  typedef __attribute__((address_space(3))) const JpegHuff l_huff;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= nitems) return;
  const JpegProgItem I = items[blockIdx.x];
#pragma unroll
  for (int t = 0; t < 3; t++) {
    if (I.tab[t] < 0) continue;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(huff + I.tab[t]);
    uint32_t *dstw = reinterpret_cast<uint32_t *>(sh + t);
    for (int i = tid; i < (int)sizeof(JpegHuff) / 4; i += 64) dstw[i] = src[i];
  }
  blk[tid] = 0;
  if (tid == 0) outside = 0;
  __syncthreads();
  const JpegDesc *Dp = descs + I.img;
  int hs[3], vs[3], bw[3];
  int64_t co[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const bool on = k < I.ns;
    const int c = on ? I.ci[k] : 0;
    hs[k] = on && I.ns > 1 ? Dp->h[c] : 1;
    vs[k] = on && I.ns > 1 ? Dp->v[c] : 1;
    bw[k] = Dp->bw[c];
    co[k] = Dp->coef[c];
  }
  const bool dc = I.Ss == 0, refine = I.Ah != 0;
  const bool mine = tid >= I.Ss && tid <= I.Se;  // this lane's coefficient is in the scan's band
  const int Ss = I.Ss, Se = I.Se, Al = I.Al;
  // the scan's blocks in decode order: block j of the interval is sub-block
  // j % bpm of MCU mcu0 + j / bpm (bpm = 1 for a single-component scan)
  const int n0 = hs[0] * vs[0], n1 = I.ns > 1 ? hs[1] * vs[1] : 0, n2 = I.ns > 2 ? hs[2] * vs[2] : 0;
  const int bpm = n0 + n1 + n2;
  const int nblk = (I.mcu1 - I.mcu0) * bpm;
  int16_t *const w16 = reinterpret_cast<int16_t *>(work);
  // -> element offset of block j's coefficients; k = its component slot
  auto locate = [&](int j, int &k) -> int64_t {
    const int m = j / bpm;
    int idx = j - m * bpm;
    k = idx < n0 ? 0 : idx < n0 + n1 ? 1 : 2;
    idx -= k == 0 ? 0 : k == 1 ? n0 : n0 + n1;
    const int h = k == 0 ? hs[0] : k == 1 ? hs[1] : hs[2], v = k == 0 ? vs[0] : k == 1 ? vs[1] : vs[2];
    const int by = idx / h, bx = idx - by * h;
    const int64_t base = (k == 0 ? co[0] : k == 1 ? co[1] : co[2]) >> 1;
    return base + jpeg_prog_block(I, I.mcu0 + m, h, v, by, bx, k == 0 ? bw[0] : k == 1 ? bw[1] : bw[2]) * 64;
  };
  BitReader br;
  br.init(Dp->ecs, I.byte0, I.end);
  JpegProgState S{};
  int16_t *b = blk;
  int k = 0;
  // corrupt data that makes libjpeg store outside the scan's band (fi_jpeg_prog.h): handover[image] = 1,
  // and the host decodes that image
  if (!refine) {
    // first pass: the procedure writes the band of the staging block (zero
    // before), the band's lanes store it
    for (int j = 0; j < nblk; j++) {
      // jdphuff.c insufficient_data: the MCU it was raised in is finished, the later ones are left alone
      // (an AC scan's MCU is one block)
      if (br.short_of_data() && (bpm == 1 || j % bpm == 0)) break;
      if (!dc && S.eobrun > 0) {  // the blocks of an end-of-band run stay zero
        const uint32_t left = (uint32_t)(nblk - j), skip = S.eobrun < left ? S.eobrun : left;
        S.eobrun -= skip;
        j += (int)skip - 1;
        continue;
      }
      int16_t *g = w16 + locate(j, k);
      if (dc) {
        if (k == 0)
          jpeg_prog_dc_first<JpegProgDevOps>(br, (l_huff *)(sh + 0), b, S.pred[0], Al);
        else if (k == 1)
          jpeg_prog_dc_first<JpegProgDevOps>(br, (l_huff *)(sh + 1), b, S.pred[1], Al);
        else
          jpeg_prog_dc_first<JpegProgDevOps>(br, (l_huff *)(sh + 2), b, S.pred[2], Al);
      } else {
        if (!jpeg_prog_ac_first<JpegProgDevOps>(br, (l_huff *)(sh + 0), b, S.eobrun, Ss, Se, Al)) outside = 1;
      }
      if (mine) {
        g[tid] = b[tid];
        b[tid] = 0;
      }
    }
    if (outside && tid == 0) handover[items[blockIdx.x].img] = 1;
    return;
  }
  // refinement: lane z holds coefficient z of the block (the next block's is
  // in flight while this one decodes); the procedure works on ballots of them
  int16_t pre = 0;
  if (mine && nblk > 0) pre = w16[locate(0, k) + tid];
  for (int j = 0; j < nblk; j++) {
    if (br.short_of_data() && (bpm == 1 || j % bpm == 0)) break;  // (a DC refinement reads zeros: no change)
    int16_t *g = w16 + locate(j, k);
    const int16_t cur = pre;
    if (mine && j + 1 < nblk) {
      int kn;
      pre = w16[locate(j + 1, kn) + tid];
    }
    int16_t out;
    if (dc) {
      out = jpeg_prog_dc_refine(br) ? (int16_t)(cur | (1 << Al)) : cur;
    } else {
      JpegProgRefine R{};
      R.nz = __ballot(mine && cur != 0);
      R.has = __ballot(mine && (cur & (1 << Al)) != 0);
      if (!jpeg_prog_ac_refine<JpegProgDevOps>(br, (l_huff *)(sh + 0), R, S.eobrun, Ss, Se)) outside = 1;
      out = jpeg_prog_refined(cur, tid, R, Al);
    }
    if (mine && out != cur) g[tid] = out;
  }
  if (outside && tid == 0) handover[items[blockIdx.x].img] = 1;
}

// ---------------------------------------------------------------------------
// device: islow IDCT (jidctint.c), one thread per block
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint8_t jpeg_range_limit(int x) {  // IDCT_range_limit[x & RANGE_MASK]
  const int m = x & 1023;
  const int v = (m >= 512 ? m - 1024 : m) + 128;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// one thread per 8x8 block of the batch; blk0[j] = first block of the j-th
// (image, component) pair (3 pairs per image, empty ones for gray), blk0[3 n] = total
__device__ __forceinline__ void jpeg_idct_block(const JpegDesc *__restrict__ descs, const int64_t *__restrict__ blk0,
                                                int nimg, const uint16_t *__restrict__ qts, uint8_t *__restrict__ work,
                                                int32_t *__restrict__ handover, int64_t i);
// (grid-stride, as k_jpeg_color)
__global__ __launch_bounds__(256) void k_jpeg_idct(const JpegDesc *__restrict__ descs,
                                                   const int64_t *__restrict__ blk0, int nimg,
                                                   const uint16_t *__restrict__ qts, uint8_t *__restrict__ work,
                                                   int32_t *__restrict__ handover) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < blk0[3 * nimg]; i += (int64_t)gridDim.x * 256)
    jpeg_idct_block(descs, blk0, nimg, qts, work, handover, i);
}
__device__ __forceinline__ void jpeg_idct_block(const JpegDesc *__restrict__ descs, const int64_t *__restrict__ blk0,
                                                int nimg, const uint16_t *__restrict__ qts, uint8_t *__restrict__ work,
                                                int32_t *__restrict__ handover, int64_t i) {
  int lo = 0, hi = 3 * nimg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk0[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  struct {
    int img, comp, blk;
  } R = {lo / 3, lo % 3, (int)(i - blk0[lo])};
  const JpegDesc &D = descs[R.img];
  const int c = R.comp;
  const int by = R.blk / D.bw[c], bx = R.blk - by * D.bw[c];
  const int16_t *in = reinterpret_cast<const int16_t *>(work + D.coef[c] + (int64_t)R.blk * 128);
  const uint16_t *q = qts + (int64_t)(D.qt + D.tq[c]) * 64;
  constexpr int CB = 13, P1 = 2;
  constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
  int ws[64];
  int cf[64];
  // coefficient blocks are stored in zigzag order: natural k = jpeg_natural_order[z]
  constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                              12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                              58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
#pragma unroll
  for (int z = 0; z < 64; z++) cf[zz[z]] = (int)in[z] * (int)q[zz[z]];
  // The decoder the output is compared with runs this transform in SIMD: 16-bit
  // products and sums, a first pass saturated to 16 bits, samples saturated
  // instead of looked up in the range-limit table.  It equals jidctint.c (this
  // code) while every dequantised coefficient and first-pass value is within
  // +-16383 (no 16-bit sum of two wraps, no 32-bit sum here overflows) and every
  // sample, before the level shift, within the table's [-512, 511].  Corrupt
  // data leaves that range: such an image is handed to the host decoder
  // (handover[image] = 1, FI_EUNSUPPORTED).
  int dlo = 0, dhi = 0, slo = 0, shi = 0;
#pragma unroll
  for (int k = 0; k < 64; k += 2) {
    dlo = min(dlo, min(cf[k], cf[k + 1]));
    dhi = max(dhi, max(cf[k], cf[k + 1]));
  }
  // pass 1: columns
#pragma unroll
  for (int x = 0; x < 8; x++) {
    int z2 = cf[16 + x], z3 = cf[48 + x];
    int z1 = (z2 + z3) * F0541;
    int tmp2 = z1 + z3 * (-F1847);
    int tmp3 = z1 + z2 * F0765;
    z2 = cf[x];
    z3 = cf[32 + x];
    int tmp0 = (z2 + z3) * (1 << CB);
    int tmp1 = (z2 - z3) * (1 << CB);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = cf[56 + x];
    tmp1 = cf[40 + x];
    tmp2 = cf[24 + x];
    tmp3 = cf[8 + x];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F1175;
    tmp0 *= F0298;
    tmp1 *= F2053;
    tmp2 *= F3072;
    tmp3 *= F1501;
    z1 *= -F0899;
    z2 *= -F2562;
    z3 *= -F1961;
    z4 *= -F0390;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr int S = CB - P1, R1 = 1 << (S - 1);
    ws[x] = (tmp10 + tmp3 + R1) >> S;
    ws[56 + x] = (tmp10 - tmp3 + R1) >> S;
    ws[8 + x] = (tmp11 + tmp2 + R1) >> S;
    ws[48 + x] = (tmp11 - tmp2 + R1) >> S;
    ws[16 + x] = (tmp12 + tmp1 + R1) >> S;
    ws[40 + x] = (tmp12 - tmp1 + R1) >> S;
    ws[24 + x] = (tmp13 + tmp0 + R1) >> S;
    ws[32 + x] = (tmp13 - tmp0 + R1) >> S;
  }
#pragma unroll
  for (int k = 0; k < 64; k += 2) {
    dlo = min(dlo, min(ws[k], ws[k + 1]));
    dhi = max(dhi, max(ws[k], ws[k + 1]));
  }
  // pass 2: rows -> samples
  uint8_t *out = work + D.plane[c] + (int64_t)(by * 8) * (D.bw[c] * 8) + bx * 8;
  const int pitch = D.bw[c] * 8;
  auto limit = [&slo, &shi](int x) {
    slo = min(slo, x);
    shi = max(shi, x);
    return jpeg_range_limit(x);
  };
#pragma unroll
  for (int y = 0; y < 8; y++) {
    const int *w = ws + 8 * y;
    int z2 = w[2], z3 = w[6];
    int z1 = (z2 + z3) * F0541;
    int tmp2 = z1 + z3 * (-F1847);
    int tmp3 = z1 + z2 * F0765;
    int tmp0 = (w[0] + w[4]) * (1 << CB);
    int tmp1 = (w[0] - w[4]) * (1 << CB);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = w[7];
    tmp1 = w[5];
    tmp2 = w[3];
    tmp3 = w[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F1175;
    tmp0 *= F0298;
    tmp1 *= F2053;
    tmp2 *= F3072;
    tmp3 *= F1501;
    z1 *= -F0899;
    z2 *= -F2562;
    z3 *= -F1961;
    z4 *= -F0390;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr int S = CB + P1 + 3, R2 = 1 << (S - 1);
    uint32_t lo = 0, hi = 0;
    lo |= (uint32_t)limit((tmp10 + tmp3 + R2) >> S);
    lo |= (uint32_t)limit((tmp11 + tmp2 + R2) >> S) << 8;
    lo |= (uint32_t)limit((tmp12 + tmp1 + R2) >> S) << 16;
    lo |= (uint32_t)limit((tmp13 + tmp0 + R2) >> S) << 24;
    hi |= (uint32_t)limit((tmp13 - tmp0 + R2) >> S);
    hi |= (uint32_t)limit((tmp12 - tmp1 + R2) >> S) << 8;
    hi |= (uint32_t)limit((tmp11 - tmp2 + R2) >> S) << 16;
    hi |= (uint32_t)limit((tmp10 - tmp3 + R2) >> S) << 24;
    *reinterpret_cast<uint2 *>(out + (int64_t)y * pitch) = uint2{lo, hi};
  }
  if (dlo < -16383 || dhi > 16383 || slo < -512 || shi > 511) handover[R.img] = 1;
}

// ---------------------------------------------------------------------------
// device: fancy upsampling + YCbCr -> RGB (jdsample.c, jdcolor.c)
// ---------------------------------------------------------------------------
// chroma sample of output pixel (x, y) for luma sampling (hs, vs) over 1x1 chroma
__device__ __forceinline__ int jpeg_up(const uint8_t *pl, int pitch, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1 && vs == 1) return pl[(int64_t)y * pitch + x];
  const int cx = x >> 1;
  // jdsample.c jinit_upsampler: the fancy filters only for downsampled_width > 2, else h2v1 / h2v2_upsample (replication)
  if (dw <= 2) return pl[(int64_t)(vs == 1 ? y : y >> 1) * pitch + cx];
  const int cl = cx > 0 ? cx - 1 : 0, cr = cx < dw - 1 ? cx + 1 : dw - 1;
  const bool odd = x & 1;
  if (vs == 1) {  // h2v1_fancy_upsample
    const uint8_t *r = pl + (int64_t)y * pitch;
    return odd ? (3 * r[cx] + r[cr] + 2) >> 2 : (3 * r[cx] + r[cl] + 1) >> 2;
  }
  // h2v2_fancy_upsample: column sums 3 * nearer row + further row (edge rows replicated)
  const int cy = y >> 1;
  const int fy = (y & 1) ? (cy < dh - 1 ? cy + 1 : dh - 1) : (cy > 0 ? cy - 1 : 0);
  const uint8_t *r0 = pl + (int64_t)cy * pitch, *r1 = pl + (int64_t)fy * pitch;
  const int t = 3 * r0[cx] + r1[cx];
  if (odd) return (3 * t + 3 * r0[cr] + r1[cr] + 7) >> 4;
  return (3 * t + 3 * r0[cl] + r1[cl] + 8) >> 4;
}
__device__ __forceinline__ uint8_t jpeg_clamp(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// Pixel (x, y) of a YCbCr image from its luma sample Y: fancy-upsampled chroma
// and jdcolor.c ycc_rgb_convert, as R | G << 8 | B << 16 (both colour kernels)
__device__ __forceinline__ uint32_t jpeg_ycc_rgb(const JpegDesc &D, const uint8_t *__restrict__ work, int Y, int x,
                                                 int y) {
  const int hs = D.h[0], vs = D.v[0];
  const int cb = jpeg_up(work + D.plane[1], D.bw[1] * 8, D.dw[1], D.dh[1], hs, vs, x, y);
  const int cr = jpeg_up(work + D.plane[2], D.bw[2] * 8, D.dw[2], D.dh[2], hs, vs, x, y);
  // build_ycc_rgb_table: FIX(x) = (int)(x * 65536 + 0.5), ONE_HALF = 1 << 15
  const int xr = cr - 128, xb = cb - 128;
  const int r = Y + ((91881 * xr + 32768) >> 16);
  const int g = Y + ((-22554 * xb + 32768 + -46802 * xr) >> 16);
  const int b = Y + ((116130 * xb + 32768) >> 16);
  return (uint32_t)jpeg_clamp(r) | (uint32_t)jpeg_clamp(g) << 8 | (uint32_t)jpeg_clamp(b) << 16;
}

__device__ __forceinline__ void jpeg_color_px(const JpegDesc *__restrict__ descs, const int64_t *__restrict__ px0,
                                              int nimg, const uint8_t *__restrict__ work, int64_t i) {
  // image of pixel i: binary search over the per-image pixel prefix
  int lo = 0, hi = nimg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (px0[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  if (i >= px0[nimg]) return;
  const JpegDesc &D = descs[lo];
  const int64_t k = i - px0[lo];
  const int y = (int)(k / D.W), x = (int)(k - (int64_t)y * D.W);
  const int yp = D.bw[0] * 8;
  const uint8_t Y = work[D.plane[0] + (int64_t)y * yp + x];
  if (D.ncomp == 1) {
    uint8_t *o = D.dst + (int64_t)y * D.dst_stride + x * D.dst_c;
    for (int k = 0; k < D.dst_c; k++) o[k] = Y;
    return;
  }
  const uint32_t p = jpeg_ycc_rgb(D, work, Y, x, y);
  uint8_t *o = D.dst + (int64_t)y * D.dst_stride + 3 * x;
  o[0] = (uint8_t)p;
  o[1] = (uint8_t)(p >> 8);
  o[2] = (uint8_t)(p >> 16);
}

// (grid-stride: a dispatch's work-item count is 32-bit, a batch may hold more pixels)
__global__ __launch_bounds__(256) void k_jpeg_color(const JpegDesc *__restrict__ descs, const int64_t *__restrict__ px0,
                                                    int nimg, const uint8_t *__restrict__ work) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < px0[nimg]; i += (int64_t)gridDim.x * 256)
    jpeg_color_px(descs, px0, nimg, work, i);
}

// The colour stage of the images decoded through a view (fi_jpeg_view.h): the
// same pixels, written where the oriented, extracted image wants them.  One
// 256-thread workgroup per (image, 32x32 tile of the output rectangle); vt0 =
// the per-view tile prefix (binary search, the grid strides over the items as
// k_jpeg_color does over px0).
//   o 1..4  lanes run along the output row: plane reads and dst writes are both
//           row-contiguous (reversed for a flip), no LDS;
//   o 5..8  phase 1: lanes run along the SOURCE row (consecutive lanes read
//           consecutive luma bytes) and write the pixel, one dword, to an LDS
//           tile [source row][source column] of 33-dword rows; one barrier;
//           phase 2: lanes run along the OUTPUT row, reading the tile
//           column-wise (odd pitch: 32 lanes on 32 banks) -- no lane walks a
//           plane column and no wave scatters over 64 rows of dst.
// Chroma neighbours outside the rectangle come from the full planes (edge
// replication at the image edges only); only bytes [0, w * dst_c) of the h
// rows are written.
__device__ __forceinline__ uint32_t jpeg_view_px(const JpegDesc &D, const uint8_t *__restrict__ work, int sx, int sy) {
  const int Y = work[D.plane[0] + (int64_t)sy * (D.bw[0] * 8) + sx];
  if (D.ncomp == 1) return (uint32_t)Y * 0x010101u;
  return jpeg_ycc_rgb(D, work, Y, sx, sy);
}
__device__ __forceinline__ void jpeg_view_store(const JpegDesc &D, const JpegViewDesc &V, int u, int v, uint32_t p) {
  uint8_t *o = D.dst + (int64_t)(v - V.y) * D.dst_stride + (int64_t)(u - V.x) * D.dst_c;
  o[0] = (uint8_t)p;
  if (D.dst_c == 3) {
    o[1] = (uint8_t)(p >> 8);
    o[2] = (uint8_t)(p >> 16);
  }
}
__global__ __launch_bounds__(256) void k_jpeg_color_view(const JpegDesc *__restrict__ descs,
                                                         const JpegViewDesc *__restrict__ views,
                                                         const int64_t *__restrict__ vt0, int nview,
                                                         const uint8_t *__restrict__ work) {
  constexpr int T = kJpegViewTile, P = T + 1;
  __shared__ uint32_t tile[T * P];
  const int cx = threadIdx.x & (T - 1), cy = threadIdx.x / T;  // 8 rows of 32 lanes per pass
  for (int64_t item = blockIdx.x; item < vt0[nview]; item += gridDim.x) {
    int lo = 0, hi = nview;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (vt0[mid] <= item)
        lo = mid;
      else
        hi = mid;
    }
    const JpegViewDesc V = views[lo];
    const JpegDesc &D = descs[V.img];
    const int t = (int)(item - vt0[lo]);
    const int ty = t / V.tiles_x, tx = t - ty * V.tiles_x;
    const int u0 = V.x + tx * T, v0 = V.y + ty * T;  // the tile in the oriented image
    const int tw = min(T, V.x + V.w - u0), th = min(T, V.y + V.h - v0);
    if (!jpeg_view_transposed(V.o)) {
      if (cx < tw)
        for (int r = cy; r < th; r += 256 / T) {
          int sx, sy;
          jpeg_view_map(V.o, D.W, D.H, u0 + cx, v0 + r, &sx, &sy);
          jpeg_view_store(D, V, u0 + cx, v0 + r, jpeg_view_px(D, work, sx, sy));
        }
      continue;
    }
    // phase 1: lane cx along the source row = the output column's direction v, row r of the pass = u
    if (cx < th)
      for (int r = cy; r < tw; r += 256 / T) {
        int sx, sy;
        jpeg_view_map(V.o, D.W, D.H, u0 + r, v0 + cx, &sx, &sy);
        tile[r * P + cx] = jpeg_view_px(D, work, sx, sy);
      }
    __syncthreads();
    // phase 2: lane cx along the output row
    if (cx < tw)
      for (int r = cy; r < th; r += 256 / T) jpeg_view_store(D, V, u0 + cx, v0 + r, tile[cx * P + r]);
    if (item + gridDim.x < vt0[nview]) __syncthreads();  // (the block's next tile overwrites the LDS tile)
  }
}

// ---------------------------------------------------------------------------
// host: batch plan + launches
// ---------------------------------------------------------------------------
// Plans and runs one decode batch.  `alloc(which, bytes)` returns memory that
// stays valid until the stream has run: 0 device upload (compressed data +
// tables), 2 device work (coefficients + planes), 3 pinned host staging.
int jpeg_decode_batch(hipStream_t st, const uint8_t *const *data, const size_t *len, int n, uint8_t *const *dst,
                      const int64_t *dst_stride, int out_channels, uint32_t flags, const fi_jpeg_view *views,
                      int32_t *status, void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *),
                      void *actx, std::string *err) {
  std::vector<JpegHdr> hd(n);
  std::vector<int> ok(n, 0);
  std::map<std::string, int> huff_ix;
  std::vector<JpegHuff> huffs;
  std::vector<uint16_t> qts;
  std::vector<JpegDesc> descs;
  std::vector<int> desc_img;
  std::vector<JpegInterval> ivs;
  std::vector<JpegProgItem> pitems;  // progressive streams: (image, scan, restart interval)
  std::vector<char> desc_prog;
  size_t pcoef_total = 0;            // their coefficient planes: one region at the end of the work buffer, zeroed
  std::vector<int64_t> blk0;  // first block of each (image, component)
  int64_t nblocks = 0;
  std::vector<int64_t> px0(1, 0);     // k_jpeg_color's pixels: the images without a view
  std::vector<JpegViewDesc> vds;      // k_jpeg_color_view's: the others, and their tile prefix
  std::vector<int64_t> vt0(1, 0);
  size_t ecs_total = 0, work_total = 0;
  // header parse (incl. the scan for the end of each entropy-coded segment)
  // and, below, the staging copies run on a few host threads
  const int nthr = (int)std::min<size_t>(8, std::max<size_t>(1, (size_t)n / 16));
  auto parallel = [&](int count, const std::function<void(int)> &fn) {
    if (nthr <= 1 || count < 2) {
      for (int i = 0; i < count; i++) fn(i);
      return;
    }
    std::atomic<int> next(0);
    std::vector<std::thread> th;
    for (int t = 0; t < nthr; t++)
      th.emplace_back([&]() {
        for (int i = next++; i < count; i = next++) fn(i);
      });
    for (auto &t : th) t.join();
  };
  // a view's orientation: given, or (0) the file's; undetermined: that image decodes on the host
  std::vector<int> orient(n, 1);
  parallel(n, [&](int i) {
    status[i] = jpeg_parse(data[i], len[i], &hd[i], flags);
    if (!views) return;
    orient[i] = views[i].orientation;
    if (orient[i] < 0 || orient[i] > 8)
      status[i] = FI_EINVAL;
    else if (orient[i] == 0 && !status[i] && jpeg_orientation(data[i], len[i], &orient[i]) != FI_OK)
      status[i] = FI_EUNSUPPORTED;
  });
  for (int i = 0; i < n; i++) {
    if (status[i]) continue;
    JpegHdr &H = hd[i];
    // the view's rectangle, inside the oriented image (all 0: the whole of it)
    JpegViewDesc V{};
    V.o = orient[i];
    if (views) {
      const fi_jpeg_view &R = views[i];
      const int ow = jpeg_view_transposed(V.o) ? H.H : H.W, oh = jpeg_view_transposed(V.o) ? H.W : H.H;
      const bool whole = R.x == 0 && R.y == 0 && R.w == 0 && R.h == 0;
      if (!whole && (R.x < 0 || R.y < 0 || R.w <= 0 || R.h <= 0 || R.x > ow - R.w || R.y > oh - R.h)) {
        status[i] = FI_EINVAL;
        continue;
      }
      V.x = R.x;
      V.y = R.y;
      V.w = whole ? ow : R.w;
      V.h = whole ? oh : R.h;
      if (whole && V.o == 1) V.w = V.h = 0;  // no view: k_jpeg_color, as without `views`
    }
    JpegDesc D{};
    D.W = H.W;
    D.H = H.H;
    D.ncomp = H.ncomp;
    D.hmax = D.vmax = 1;
    for (int c = 0; c < H.ncomp; c++) {
      D.hmax = std::max(D.hmax, H.h[c]);
      D.vmax = std::max(D.vmax, H.v[c]);
    }
    // a progressive stream's tables: the ones its scans use, deduplicated over the batch as well
    std::vector<int> tabmap(H.ptab.size());
    for (size_t t = 0; t < H.ptab.size() && !status[i]; t++) {
      auto it = huff_ix.find(H.ptab[t]);
      if (it == huff_ix.end()) {
        JpegHuff hf;
        if (!jpeg_build_huff(H.ptab[t].substr(1), H.ptab[t][0] == 'D', &hf)) {
          status[i] = FI_EINVAL;
          break;
        }
        it = huff_ix.emplace(H.ptab[t], (int)huffs.size()).first;
        huffs.push_back(hf);
      }
      tabmap[t] = it->second;
    }
    if (status[i]) continue;
    D.mcux = (H.W + 8 * D.hmax - 1) / (8 * D.hmax);
    D.mcuy = (H.H + 8 * D.vmax - 1) / (8 * D.vmax);
    D.qt = (int)(qts.size() / 64);
    for (int t = 0; t < 4; t++) qts.insert(qts.end(), H.qt[t], H.qt[t] + 64);
    // the image's four table slots, deduplicated over the batch (an encoder's
    // tables are shared by all its images: a few distinct tables, LDS resident)
    for (int t = 0; t < 4; t++) {
      D.ht[t] = -1;
      if (H.dht[t].empty() || H.progressive) continue;
      const std::string key = std::string(1, t < 2 ? 'D' : 'A') + H.dht[t];  // class + table bytes
      auto it = huff_ix.find(key);
      if (it == huff_ix.end()) {
        JpegHuff hf;
        if (!jpeg_build_huff(H.dht[t], t < 2, &hf)) {
          status[i] = FI_EINVAL;
          break;
        }
        it = huff_ix.emplace(key, (int)huffs.size()).first;
        huffs.push_back(hf);
      }
      D.ht[t] = it->second;
    }
    if (status[i]) continue;
    for (int c = 0; c < H.ncomp; c++) {
      D.h[c] = H.h[c];
      D.v[c] = H.v[c];
      D.tq[c] = H.tq[c];
      D.td[c] = H.td[c];
      D.ta[c] = H.ta[c];
      D.bw[c] = D.mcux * H.h[c];
      D.bh[c] = D.mcuy * H.v[c];
      D.dw[c] = (H.W * H.h[c] + D.hmax - 1) / D.hmax;  // jdmaster.c downsampled_width
      D.dh[c] = (H.H * H.v[c] + D.vmax - 1) / D.vmax;
      if (H.progressive) {  // (offset in the zeroed region until placed)
        D.coef[c] = (int64_t)pcoef_total;
        pcoef_total += (size_t)D.bw[c] * D.bh[c] * 128;
      } else {
        D.coef[c] = (int64_t)work_total;
        work_total += (size_t)D.bw[c] * D.bh[c] * 128;
      }
      D.plane[c] = (int64_t)work_total;
      work_total += ((size_t)D.bw[c] * 8 * D.bh[c] * 8 + 255) & ~(size_t)255;
    }
    D.ecs_len = (int32_t)(H.ecs1 - H.ecs0);
    D.ecs = reinterpret_cast<const uint8_t *>(ecs_total);  // offset until placed
    D.dst = dst[i];
    D.dst_stride = dst_stride[i];
    D.dst_c = out_channels == 3 || H.ncomp == 3 ? 3 : 1;
    const int img = (int)descs.size();
    // restart intervals: RSTn markers split the segment
    const int nmcu = D.mcux * D.mcuy;
    if (H.progressive) {
      JpegGeom G;
      jpeg_geom(H, &G);
      jpeg_prog_items(H, G, data[i], img, tabmap.data(), &pitems);
    } else if (H.restart > 0) {
      const uint8_t *e = data[i] + H.ecs0;
      int byte0 = 0, mcu0 = 0;
      for (size_t q = 0; q + 1 < (size_t)D.ecs_len && mcu0 < nmcu; q++) {
        if (e[q] == 0xFF && e[q + 1] >= 0xD0 && e[q + 1] <= 0xD7) {
          ivs.push_back({img, mcu0, std::min(mcu0 + H.restart, nmcu), byte0});
          mcu0 += H.restart;
          byte0 = (int)q + 2;
          q++;
        }
      }
      if (mcu0 < nmcu) ivs.push_back({img, mcu0, nmcu, byte0});
    } else {
      ivs.push_back({img, 0, nmcu, 0});
    }
    for (int c = 0; c < 3; c++) {
      blk0.push_back(nblocks);
      if (c < H.ncomp) nblocks += (int64_t)D.bw[c] * D.bh[c];
    }
    if (V.w > 0) {
      V.img = img;
      V.tiles_x = (V.w + kJpegViewTile - 1) / kJpegViewTile;
      vds.push_back(V);
      vt0.push_back(vt0.back() + (int64_t)V.tiles_x * ((V.h + kJpegViewTile - 1) / kJpegViewTile));
      px0.push_back(px0.back());
    } else {
      px0.push_back(px0.back() + (int64_t)H.W * H.H);
    }
    // zero pad: the reader's window (a progressive scan's reader stops at its scan's end, inside the segment)
    ecs_total += ((size_t)D.ecs_len + 512 + 255) & ~(size_t)255;
    descs.push_back(D);
    desc_prog.push_back(H.progressive);
    desc_img.push_back(i);
  }
  if (descs.empty()) return 0;
  // the progressive images' coefficients: after everything else
  work_total = (work_total + 255) & ~(size_t)255;
  for (size_t k = 0; k < descs.size(); k++)
    if (desc_prog[k])
      for (int c = 0; c < descs[k].ncomp; c++) descs[k].coef[c] += (int64_t)work_total;
  const size_t pcoef0 = work_total;
  // ... and the per-image handover flags (k_jpeg_prog, k_jpeg_idct: corrupt data the host decodes), zeroed with them
  pcoef_total = (pcoef_total + 255) & ~(size_t)255;
  const size_t o_hand = pcoef0 + pcoef_total, hand_bytes = descs.size() * sizeof(int32_t);
  pcoef_total += (hand_bytes + 255) & ~(size_t)255;
  work_total += pcoef_total;
  // scans of one level are independent: one launch per level, in order
  std::stable_sort(pitems.begin(), pitems.end(),
                   [](const JpegProgItem &a, const JpegProgItem &b) { return a.level < b.level; });
  // one upload: compressed data (each segment zero padded for the reader's
  // window) then tables + descriptors, staged in pinned host memory
  const size_t o_desc = 0, o_iv = o_desc + ((descs.size() * sizeof(JpegDesc) + 255) & ~(size_t)255);
  const size_t o_ref = o_iv + ((ivs.size() * sizeof(JpegInterval) + 255) & ~(size_t)255);
  blk0.push_back(nblocks);
  const size_t o_huff = o_ref + ((blk0.size() * 8 + 255) & ~(size_t)255);
  const size_t o_qt = o_huff + ((huffs.size() * sizeof(JpegHuff) + 255) & ~(size_t)255);
  const size_t o_px = o_qt + ((qts.size() * 2 + 255) & ~(size_t)255);
  const size_t o_pit = o_px + ((px0.size() * 8 + 255) & ~(size_t)255);
  const size_t o_view = o_pit + ((pitems.size() * sizeof(JpegProgItem) + 255) & ~(size_t)255);
  const size_t o_vt = o_view + ((vds.size() * sizeof(JpegViewDesc) + 255) & ~(size_t)255);
  const size_t tab0 = (ecs_total + 255) & ~(size_t)255, up_total = tab0 + o_vt + vt0.size() * 8;
  uint8_t *din = (uint8_t *)alloc(actx, 0, up_total);
  uint8_t *hst = (uint8_t *)alloc(actx, 3, up_total + hand_bytes);  // (+ the handover flags, read back)
  uint8_t *dwork = (uint8_t *)alloc(actx, 2, std::max(work_total, (size_t)256));
  if (!din || !hst || !dwork) {
    *err = "memory for the JPEG batch";
    return FI_ENOMEM;
  }
  uint8_t *dtab = din + tab0, *htab = hst + tab0;
  parallel((int)descs.size(), [&](int k) {
    const JpegDesc &D = descs[k];
    const size_t off = (size_t)reinterpret_cast<uintptr_t>(D.ecs);
    memcpy(hst + off, data[desc_img[k]] + hd[desc_img[k]].ecs0, D.ecs_len);
    const size_t pad_end =
        k + 1 < (int)descs.size() ? (size_t)reinterpret_cast<uintptr_t>(descs[k + 1].ecs) : tab0;
    memset(hst + off + D.ecs_len, 0, pad_end - off - D.ecs_len);
  });
  for (JpegDesc &D : descs) D.ecs = din + (size_t)reinterpret_cast<uintptr_t>(D.ecs);
  memcpy(htab + o_desc, descs.data(), descs.size() * sizeof(JpegDesc));
  memcpy(htab + o_iv, ivs.data(), ivs.size() * sizeof(JpegInterval));
  memcpy(htab + o_ref, blk0.data(), blk0.size() * 8);
  memcpy(htab + o_huff, huffs.data(), huffs.size() * sizeof(JpegHuff));
  memcpy(htab + o_qt, qts.data(), qts.size() * 2);
  memcpy(htab + o_px, px0.data(), px0.size() * 8);
  if (!pitems.empty()) memcpy(htab + o_pit, pitems.data(), pitems.size() * sizeof(JpegProgItem));
  if (!vds.empty()) memcpy(htab + o_view, vds.data(), vds.size() * sizeof(JpegViewDesc));
  memcpy(htab + o_vt, vt0.data(), vt0.size() * 8);
  if (hipMemcpyAsync(din, hst, up_total, hipMemcpyHostToDevice, st) != hipSuccess) {
    *err = "JPEG batch upload";
    return FI_EDEVICE;
  }
  const JpegDesc *dd = (const JpegDesc *)(dtab + o_desc);
  // the distinct Huffman tables go to LDS when they are few (kJpegLdsTabs)
  const int nhuff = (int)huffs.size();
  const dim3 g((unsigned)ivs.size());  // one restart interval per 64-lane workgroup
  if (ivs.empty()) {
    // (progressive streams only)
  } else if (nhuff <= kJpegLdsTabs)
    hipLaunchKernelGGL(k_jpeg_huff<true>, g, dim3(64), 0, st, dd, (const JpegInterval *)(dtab + o_iv), (int)ivs.size(),
                       (const JpegHuff *)(dtab + o_huff), nhuff, dwork);
  else
    hipLaunchKernelGGL(k_jpeg_huff<false>, g, dim3(64), 0, st, dd, (const JpegInterval *)(dtab + o_iv),
                       (int)ivs.size(), (const JpegHuff *)(dtab + o_huff), nhuff, dwork);
  if (hipMemsetAsync(dwork + pcoef0, 0, pcoef_total, st) != hipSuccess) {
    *err = "JPEG coefficient clear";
    return FI_EDEVICE;
  }
  if (!pitems.empty()) {
    if (stage) stage(actx, "k_jpeg_prog");
    for (size_t a = 0; a < pitems.size();) {
      size_t z = a;
      while (z < pitems.size() && pitems[z].level == pitems[a].level) z++;
      hipLaunchKernelGGL(k_jpeg_prog, dim3((unsigned)(z - a)), dim3(64), 0, st, dd,
                         (const JpegProgItem *)(dtab + o_pit) + a, (int)(z - a), (const JpegHuff *)(dtab + o_huff),
                         dwork, (int32_t *)(dwork + o_hand));
      a = z;
    }
    if (stage) stage(actx, nullptr);
  }
  hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)std::min<int64_t>((nblocks + 255) / 256, 1 << 20)), dim3(256), 0, st, dd,
                     (const int64_t *)(dtab + o_ref), (int)descs.size(), (const uint16_t *)(dtab + o_qt), dwork,
                     (int32_t *)(dwork + o_hand));
  if (px0.back() > 0) {
    if (stage) stage(actx, "k_jpeg_color");
    hipLaunchKernelGGL(k_jpeg_color, dim3((unsigned)std::min<int64_t>((px0.back() + 255) / 256, 1 << 20)), dim3(256), 0, st, dd,
                       (const int64_t *)(dtab + o_px), (int)descs.size(), dwork);
    if (stage) stage(actx, nullptr);
  }
  if (!vds.empty()) {  // the images with a view: their own colour kernel, one workgroup per output tile
    if (stage) stage(actx, "k_jpeg_color_view");
    hipLaunchKernelGGL(k_jpeg_color_view, dim3((unsigned)std::min<int64_t>(vt0.back(), 1 << 20)), dim3(256), 0, st, dd,
                       (const JpegViewDesc *)(dtab + o_view), (const int64_t *)(dtab + o_vt), (int)vds.size(), dwork);
    if (stage) stage(actx, nullptr);
  }
  // the handover flags come back behind the kernels, into the staging buffer's tail
  const int32_t *hand = reinterpret_cast<const int32_t *>(hst + up_total);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(hst + up_total, dwork + o_hand, hand_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    *err = "JPEG decode kernels";
    return FI_EDEVICE;
  }
  for (size_t k = 0; k < descs.size(); k++)
    if (hand[k]) status[desc_img[k]] = FI_EUNSUPPORTED;
  return 0;
}

}  // namespace fi
