// fi_png_enc.hip -- PNG encode on the GPU for the outputs JPEG cannot carry
// (alpha): lossless, any conforming decoder returns the source pixels.  The
// filtered stream (h rows of a filter-type byte + w * channels bytes) is cut
// into bands of kPngBand bytes; every band is its own deflate block sequence
// in its own IDAT chunk, so bands are independent work:
//
//   k_png_filter  a wave per row: the cost sum min(x, 256 - x) of the five PNG
//            filters against the raw previous row, the cheapest type (ties to
//            the lower type), the type byte and the filtered row -> stream;
//   k_png_lz      a wave per band: the band in LDS beside a 16K-entry u16 hash
//            table of 3-byte prefixes, updated 64 positions at a time (a
//            candidate always lies in an earlier group); lanes extend their
//            matches 4 bytes at a time, the greedy parse walks the group on the
//            scalar unit (take the length at p, advance by it) and the lanes it
//            chose write their symbols and count them with LDS atomics; a match
//            of up to 12 bytes is taken only where it costs less than its
//            literals would (estimated from the band's byte counts); the band's
//            Adler-32 partial sums on the way in;
//   k_png_codes   a wave per band, one lane at work: png_build_block
//            (fi_png_enc.h, the function the CPU tests run) -- length-limited
//            canonical codes, the dynamic header; stored, fixed or dynamic codes,
//            whichever is smallest; where the parse found matches the band is
//            also priced as plain literals and goes out that way if smaller;
//   k_png_emit    a workgroup per band: bits per symbol, prefix sum, codes ORed
//            LSB first into an LDS bit buffer (k_jpeg_henc's pattern); every
//            band but the last ends byte aligned with an empty stored block;
//            the last carries BFINAL and the Adler-32 combined from the band
//            partials; per-thread segment CRCs combined by x^(8 n) mod P; the
//            chunk (for band 0 behind signature + IHDR, for the last before
//            IEND) -> the band's slot;
//   k_png_scan + k_png_pack   exclusive scan of the slot lengths over the batch,
//            a workgroup per band copies its slot into one contiguous stream,
//            which the host fetches with one copy (the scan and the copy of
//            fi_enc_pack.h with a band as the item).
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
#include "fi_png_enc.h"

namespace fi {

struct PngDesc {         // one image of an encode batch
  const uint8_t *src;    // HWC u8, 1..4 channels
  int64_t stride;
  int32_t W, H, C, filter;
  int32_t rowbytes;      // W * C
  int32_t nbands;
  int32_t band0;         // its first band in the batch
  int64_t row0;          // its first row in the batch
  int64_t stream0;       // byte offset of its filtered stream (and index of its first symbol)
  int64_t nbytes;        // bytes of its filtered stream
  uint8_t hdr[48];       // signature + IHDR, then the IEND chunk
};
struct PngBandRef {
  int32_t img, idx;
};

constexpr int kPngHashBits = 14;
constexpr int kPngPayloadMax = 2 + kPngBand + 5 + 4;                  // zlib header, a stored band, Adler-32
constexpr int kPngSlotBytes = (kPngHdrBytes + 12 + kPngPayloadMax + 12 + 15) & ~15;  // + IHDR part, chunk frame, IEND
constexpr int kPngEmitWords = (kPngPayloadMax + 3) / 4 + 8;

__device__ __forceinline__ int png_cost(int v) {  // v = a filtered byte
  v &= 255;
  return v < 128 ? v : 256 - v;
}
__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// (grid-stride over the batch's rows: a wave per row)
__global__ __launch_bounds__(256) void k_png_filter(const PngDesc *__restrict__ descs, int nimg, int64_t nrows,
                                                    uint8_t *__restrict__ stream) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < nrows; r += (int64_t)gridDim.x * 4) {
    const PngDesc &D = descs[enc_find_image(descs, nimg, r, &PngDesc::row0)];
    const int y = (int)(r - D.row0), n = D.rowbytes, bpp = D.C;
    const uint8_t *cur = D.src + (int64_t)y * D.stride;
    const uint8_t *prev = cur - D.stride;  // read for y > 0 only
    int ft = D.filter;
    if (ft < 0) {
      uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
      for (int i = lane; i < n; i += 64) {
        const int x = cur[i], a = i >= bpp ? cur[i - bpp] : 0;
        const int b = y ? prev[i] : 0, c = (y && i >= bpp) ? prev[i - bpp] : 0;
        c0 += png_cost(x);
        c1 += png_cost(x - a);
        c2 += png_cost(x - b);
        c3 += png_cost(x - ((a + b) >> 1));
        c4 += png_cost(x - png_paeth(a, b, c));
      }
      c0 = enc_sum64(c0);
      c1 = enc_sum64(c1);
      c2 = enc_sum64(c2);
      c3 = enc_sum64(c3);
      c4 = enc_sum64(c4);
      ft = 0;
      uint32_t best = c0;
      if (c1 < best) best = c1, ft = 1;
      if (c2 < best) best = c2, ft = 2;
      if (c3 < best) best = c3, ft = 3;
      if (c4 < best) best = c4, ft = 4;
    }
    uint8_t *out = stream + D.stream0 + (int64_t)y * (n + 1);
    if (lane == 0) out[0] = (uint8_t)ft;
    for (int i = lane; i < n; i += 64) {
      const int x = cur[i], a = i >= bpp ? cur[i - bpp] : 0;
      const int b = y ? prev[i] : 0, c = (y && i >= bpp) ? prev[i - bpp] : 0;
      const int p = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
      out[1 + i] = (uint8_t)(x - p);
    }
  }
}

// symbols: a literal is its byte; a match is 1 << 31 | (distance - 1) << 8 | (length - 3)
__global__ __launch_bounds__(64) void k_png_lz(const PngDesc *__restrict__ descs, const PngBandRef *__restrict__ bands,
                                               int nbands, const uint8_t *__restrict__ stream,
                                               uint32_t *__restrict__ syms, int32_t *__restrict__ nsyms,
                                               uint32_t *__restrict__ hists, uint32_t *__restrict__ adler) {
  __shared__ uint32_t dataw[kPngBand / 4 + 4];
  __shared__ uint16_t tab[1 << kPngHashBits];
  __shared__ uint32_t hist[kPngHist2];
  __shared__ uint8_t lcost[256];
  const int band = blockIdx.x, lane = threadIdx.x;
  if (band >= nbands) return;
  const PngBandRef B = bands[band];
  const PngDesc &D = descs[B.img];
  const int64_t off = D.stream0 + (int64_t)B.idx * kPngBand;
  const int n = (int)std::min<int64_t>(kPngBand, D.nbytes - (int64_t)B.idx * kPngBand);
  const uint8_t *bytes = reinterpret_cast<const uint8_t *>(dataw);
  for (int i = lane; i < kPngHist2; i += 64) hist[i] = 0;
  __syncthreads();
  // the band -> LDS (16 bytes per lane; the stream of every image is padded to that), Adler partial sums,
  // byte counts
  uint64_t sa = 0, sb = 0;
  const uint4 *g = reinterpret_cast<const uint4 *>(stream + off);
  for (int i = lane; i * 16 < n; i += 64) {
    const uint4 v = g[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      dataw[4 * i + k] = w[k];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int p = 16 * i + 4 * k + j;
        const uint32_t d = p < n ? (w[k] >> (8 * j)) & 255u : 0u;
        sa += d;
        sb += (uint64_t)d * (uint32_t)(n - p);
        if (p < n) atomicAdd(&hist[kPngHist + d], 1u);
      }
    }
  }
  if (lane < 4) dataw[kPngBand / 4 + lane] = 0;
  for (int i = lane; i < (1 << kPngHashBits) / 2; i += 64) reinterpret_cast<uint32_t *>(tab)[i] = 0xFFFFFFFFu;
  __syncthreads();
  for (int i = lane; i < 256; i += 64) lcost[i] = (uint8_t)enc_literal_cost(hist[kPngHist + i], (uint32_t)n);
  __syncthreads();
  uint32_t *out = syms + off;
  int pos = 0, nsym = 0;  // wave-uniform: the parse position, symbols written
  for (int p0 = 0; p0 < n; p0 += 64) {
    const int p = p0 + lane;
    const bool hv = p + 2 < n;
    uint32_t h = 0;
    int cand = -1;
    if (hv) {
      const uint32_t v = (uint32_t)bytes[p] | ((uint32_t)bytes[p + 1] << 8) | ((uint32_t)bytes[p + 2] << 16);
      h = (v * 0x9E3779B1u) >> (32 - kPngHashBits);
      const int t = tab[h];
      cand = t == 0xFFFF ? -1 : t;
    }
    __syncthreads();  // every lane has its candidate (from an earlier group) before the table moves on
    if (hv) tab[h] = (uint16_t)p;
    __syncthreads();
    if (pos >= p0 + 64) continue;  // the whole group lies inside the last match
    int mlen = 0, mdist = 0;
    if (p >= pos && cand >= 0) {
      const int maxl = std::min(258, n - p);
      int l = 0;
      while (l < maxl) {
        uint32_t x, y;
        __builtin_memcpy(&x, bytes + p + l, 4);
        __builtin_memcpy(&y, bytes + cand + l, 4);
        x ^= y;
        if (x) {
          l += __builtin_ctz(x) >> 3;
          break;
        }
        l += 4;
      }
      l = std::min(l, maxl);
      if (l >= 3) {
        // a short match must cost less than the literals it stands for (in 1/16 bit: a length
        // code of about 7 bits, a distance code of about 5 and the distance's extra bits)
        bool pays = true;
        if (l <= 12) {
          int eb, ev, lit = 0;
          (void)enc_prefix_sym(p - cand, &eb, &ev);
          for (int k = 0; k < l; k++) lit += lcost[bytes[p + k]];
          pays = 16 * (12 + eb) < lit;
        }
        if (pays) {
          mlen = l;
          mdist = p - cand;
        }
      }
    }
    uint64_t mask = 0;  // the positions the greedy parse lands on
    const int end = std::min(p0 + 64, n);
    while (pos < end) {
      const int k = __builtin_amdgcn_readfirstlane(pos - p0);
      const int l = __builtin_amdgcn_readlane(mlen, k);
      mask |= 1ull << k;
      pos += l ? l : 1;
    }
    if ((mask >> lane) & 1ull) {
      const int at = nsym + __popcll(mask & ((1ull << lane) - 1ull));
      if (mlen) {
        out[at] = 0x80000000u | ((uint32_t)(mdist - 1) << 8) | (uint32_t)(mlen - 3);
        int eb, ev;
        atomicAdd(&hist[png_len_sym(mlen, &eb, &ev)], 1u);
        atomicAdd(&hist[kPngLL + enc_prefix_sym(mdist, &eb, &ev)], 1u);
      } else {
        const uint32_t b = bytes[p];
        out[at] = b;
        atomicAdd(&hist[b], 1u);
      }
    }
    nsym += __popcll(mask);
  }
  __syncthreads();
  for (int i = lane; i < kPngHist2; i += 64) hists[(int64_t)band * kPngHist2 + i] = hist[i];
  const uint32_t ta = enc_sum64((uint32_t)(sa % 65521u)), tb = enc_sum64((uint32_t)(sb % 65521u));
  if (lane == 0) {
    nsyms[band] = nsym;
    adler[2 * band] = ta % 65521u;
    adler[2 * band + 1] = tb % 65521u;
  }
}

__global__ __launch_bounds__(64) void k_png_codes(const PngDesc *__restrict__ descs,
                                                  const PngBandRef *__restrict__ bands, int nbands,
                                                  const uint32_t *__restrict__ hists, const int32_t *__restrict__ nsyms,
                                                  PngBandCode *__restrict__ codes) {
  __shared__ uint32_t hist[kPngHist2];
  __shared__ PngCodeWork work;
  __shared__ PngBandCode code, alt;
  const int band = blockIdx.x, lane = threadIdx.x;
  if (band >= nbands) return;
  const PngBandRef B = bands[band];
  const PngDesc &D = descs[B.img];
  const int n = (int)std::min<int64_t>(kPngBand, D.nbytes - (int64_t)B.idx * kPngBand);
  for (int i = lane; i < kPngHist2; i += 64) hist[i] = hists[(int64_t)band * kPngHist2 + i];
  __syncthreads();
  // the parse's symbols, and -- where it found matches -- the band as plain literals: the smaller block
  const bool both = nsyms[band] != n;
  const bool last = B.idx == D.nbands - 1;
  if (lane == 0) png_build_block(hist, n, last, &code, &work);
  __syncthreads();
  if (both) {
    for (int i = lane; i < kPngHist; i += 64) hist[i] = i < 256 ? hist[kPngHist + i] : 0;
    __syncthreads();
    if (lane == 0) {
      png_build_block(hist, n, last, &alt, &work);
      alt.literal = 1;
    }
    __syncthreads();
  }
  const bool use_alt = both && alt.block_bits < code.block_bits;
  const uint32_t *s = reinterpret_cast<const uint32_t *>(use_alt ? &alt : &code);
  uint32_t *d = reinterpret_cast<uint32_t *>(&codes[band]);
  for (int i = lane; i < (int)(sizeof(PngBandCode) / 4); i += 64) d[i] = s[i];
}

// k_png_emit's bit buffer (enc_or_bits)
__device__ __forceinline__ bool png_put(uint32_t *buf, int bit, uint64_t v, int nb) {
  return enc_or_bits(buf, kPngEmitWords, bit, v, nb);
}

__global__ __launch_bounds__(256) void k_png_emit(const PngDesc *__restrict__ descs,
                                                  const PngBandRef *__restrict__ bands, int nbands,
                                                  const uint8_t *__restrict__ stream, const uint32_t *__restrict__ syms,
                                                  const int32_t *__restrict__ nsyms,
                                                  const PngBandCode *__restrict__ codes,
                                                  const uint32_t *__restrict__ adler, uint8_t *__restrict__ slots,
                                                  int32_t *__restrict__ bandlen, int32_t *__restrict__ fault) {
  __shared__ uint32_t buf[kPngEmitWords];
  __shared__ uint32_t lltab[kPngLL], dtab[kPngD], crctab[256];
  __shared__ int wsum[4];
  __shared__ uint32_t wcrc[4];
  const int band = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (band >= nbands) return;
  const PngBandRef B = bands[band];
  const PngDesc &D = descs[B.img];
  const PngBandCode &K = codes[band];
  const int64_t off = D.stream0 + (int64_t)B.idx * kPngBand;
  const int n = (int)std::min<int64_t>(kPngBand, D.nbytes - (int64_t)B.idx * kPngBand);
  const bool first = B.idx == 0, last = B.idx == D.nbands - 1, stored = K.stored != 0;
  uint8_t *bb = reinterpret_cast<uint8_t *>(buf);
  for (int i = t; i < kPngEmitWords; i += 256) buf[i] = 0;
  for (int i = t; i < kPngLL; i += 256) lltab[i] = K.ll[i];
  if (t < kPngD) dtab[t] = K.dist[t];
  crctab[t] = png_crc_byte((uint32_t)t);
  __syncthreads();
  int pb = 0;  // payload bytes (uniform)
  bool ok = true;  // every bit found its place, and the block has the size k_png_codes decided on
  if (first) {
    if (t == 0) {
      bb[0] = 0x78;  // deflate, 32 KiB window
      bb[1] = 0x01;  // FCHECK, no dictionary, fastest level
    }
    pb = 2;
  }
  if (stored) {
    if (t == 0) {
      bb[pb] = last ? 1 : 0;
      bb[pb + 1] = (uint8_t)n;
      bb[pb + 2] = (uint8_t)(n >> 8);
      bb[pb + 3] = (uint8_t)~n;
      bb[pb + 4] = (uint8_t)(~n >> 8);
    }
    const uint8_t *g = stream + off;
    for (int i = t; i < n; i += 256) bb[pb + 5 + i] = g[i];
    pb += 5 + n;
  } else {
    int bit = pb * 8;
    const int bit0 = bit;
    if (t == 0) ok &= png_put(buf, bit, (last ? 1u : 0u) | ((uint32_t)K.btype << 1), 3);
    bit += 3;
    const int hb = K.hdr_bits;
    for (int w = t; w * 32 < hb; w += 256) ok &= png_put(buf, bit + 32 * w, K.hdr[w], std::min(32, hb - 32 * w));
    bit += hb;
    const uint32_t *sy = syms + off;
    const uint8_t *raw = stream + off;
    const bool literal = K.literal != 0;
    const int ns = literal ? n : nsyms[band];
    for (int base = 0; base < ns; base += 256) {
      const int i = base + t;
      uint64_t val = 0;
      int nb = 0;
      if (i < ns) {
        const uint32_t s = literal ? raw[i] : sy[i];
        if (s & 0x80000000u) {
          int eb, ev;
          const int ls = png_len_sym((int)(s & 255u) + 3, &eb, &ev);
          uint32_t e = lltab[ls];
          val = e & 0xFFFFu;
          nb = (int)(e >> 16);
          val |= (uint64_t)ev << nb;
          nb += eb;
          const int ds = enc_prefix_sym((int)((s >> 8) & 0x7FFFu) + 1, &eb, &ev);
          e = dtab[ds];
          val |= (uint64_t)(e & 0xFFFFu) << nb;
          nb += (int)(e >> 16);
          val |= (uint64_t)ev << nb;
          nb += eb;
        } else {
          const uint32_t e = lltab[s & 255u];
          val = e & 0xFFFFu;
          nb = (int)(e >> 16);
        }
      }
      int total;
      const int before = enc_offset256(nb, wsum, &total);
      ok &= png_put(buf, bit + before, val, nb);
      bit += total;
      __syncthreads();
    }
    if (t == 0) ok &= png_put(buf, bit, lltab[256] & 0xFFFFu, (int)(lltab[256] >> 16));
    bit += (int)(lltab[256] >> 16);
    ok &= bit - bit0 == K.block_bits;
    if (!last) bit += 3;  // the empty stored block's header: BFINAL 0, BTYPE 00
    pb = (bit + 7) >> 3;
    __syncthreads();
    if (!last) {
      if (t == 0 && pb + 4 <= kPngPayloadMax) {  // LEN 0, NLEN 0xFFFF
        bb[pb + 2] = 0xFF;
        bb[pb + 3] = 0xFF;
      }
      pb += 4;
    }
  }
  // png_build_block chose the form that fits; should its accounting ever disagree with this kernel's,
  // the call fails (FI_EDEVICE) instead of handing out a damaged file
  if (pb > kPngPayloadMax - (last ? 4 : 0)) {
    pb = kPngPayloadMax - (last ? 4 : 0);
    ok = false;
  }
  if (!ok) *fault = 1;
  __syncthreads();
  if (last) {
    if (t == 0) {  // the stream's Adler-32 from the band partials
      uint32_t a = 1, b = 0;
      for (int j = 0; j < D.nbands; j++) {
        const uint32_t nj = (uint32_t)std::min<int64_t>(kPngBand, D.nbytes - (int64_t)j * kPngBand);
        png_adler_append(&a, &b, adler[2 * (D.band0 + j)], adler[2 * (D.band0 + j) + 1], nj);
      }
      bb[pb] = (uint8_t)(b >> 8);
      bb[pb + 1] = (uint8_t)b;
      bb[pb + 2] = (uint8_t)(a >> 8);
      bb[pb + 3] = (uint8_t)a;
    }
    pb += 4;
    __syncthreads();
  }
  // CRC-32 of "IDAT" + payload: a segment per thread, combined by x^(8 * bytes behind it)
  const int seg = (pb + 255) >> 8, s0 = std::min(pb, t * seg), s1 = std::min(pb, s0 + seg);
  uint32_t c = 0;
  if (t == 0) {
    c = 0xFFFFFFFFu;
    const uint8_t ty[4] = {'I', 'D', 'A', 'T'};
    for (int k = 0; k < 4; k++) c = crctab[(c ^ ty[k]) & 255u] ^ (c >> 8);
  }
  for (int k = s0; k < s1; k++) c = crctab[(c ^ bb[k]) & 255u] ^ (c >> 8);
  if (c && s1 < pb) c = png_crc_mulmod(c, png_crc_xpow8((uint64_t)(pb - s1)));
#pragma unroll
  for (int d = 32; d; d >>= 1) c ^= __shfl_xor(c, d, 64);
  if (lane == 0) wcrc[wave] = c;
  __syncthreads();
  const uint32_t crc = ~(wcrc[0] ^ wcrc[1] ^ wcrc[2] ^ wcrc[3]);
  // header (band 0), chunk, IEND (last band) -> slot
  uint8_t *o = slots + (int64_t)band * kPngSlotBytes;
  int total = 0;
  if (first) {
    if (t < kPngHdrBytes) o[t] = D.hdr[t];
    o += kPngHdrBytes;
    total += kPngHdrBytes;
  }
  if (t == 0) {
    o[0] = (uint8_t)((uint32_t)pb >> 24);
    o[1] = (uint8_t)(pb >> 16);
    o[2] = (uint8_t)(pb >> 8);
    o[3] = (uint8_t)pb;
    o[4] = 'I';
    o[5] = 'D';
    o[6] = 'A';
    o[7] = 'T';
    o[8 + pb] = (uint8_t)(crc >> 24);
    o[9 + pb] = (uint8_t)(crc >> 16);
    o[10 + pb] = (uint8_t)(crc >> 8);
    o[11 + pb] = (uint8_t)crc;
  }
  for (int i = t; i < pb; i += 256) o[8 + i] = bb[i];
  total += 12 + pb;
  if (last) {
    if (t < 12) o[12 + pb + t] = D.hdr[kPngHdrBytes + t];
    total += 12;
  }
  if (t == 0) bandlen[band] = total;
}

// Exclusive scan of the slot lengths over the batch's bands (one workgroup):
// banddst[b] = where band b's bytes start in the packed stream; imgpos[2 i] /
// [2 i + 1] = start / end of image i.
__global__ __launch_bounds__(256) void k_png_scan(const PngDesc *__restrict__ descs,
                                                  const PngBandRef *__restrict__ bands, int nbands,
                                                  const int32_t *__restrict__ bandlen, int64_t *__restrict__ banddst,
                                                  int64_t *__restrict__ imgpos) {
  enc_scan_items(
      nbands,
      [=](int b) {
        const PngBandRef B = bands[b];
        return EncItem{bandlen[b], B.img, B.idx == 0, B.idx == descs[B.img].nbands - 1};
      },
      banddst, imgpos);
}

// a workgroup per band: slot -> packed (dword stores once the destination is aligned)
__global__ __launch_bounds__(256) void k_png_pack(int nbands, const int32_t *__restrict__ bandlen,
                                                  const int64_t *__restrict__ banddst,
                                                  const uint8_t *__restrict__ slots, uint8_t *__restrict__ packed) {
  const int band = blockIdx.x;
  if (band >= nbands) return;
  enc_copy_aligned(packed + banddst[band], slots + (int64_t)band * kPngSlotBytes, bandlen[band], threadIdx.x, 256);
}

// ---------------------------------------------------------------------------
// host: batch plan + launches (`alloc` / `stage` as in jpeg_encode_batch)
// ---------------------------------------------------------------------------
int png_encode_batch(hipStream_t st, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                     const int32_t *channels, const int64_t *src_stride, const int32_t *filter, int n,
                     uint8_t *const *out, const size_t *out_cap, size_t *out_len, int32_t *status,
                     void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *), void *actx,
                     std::string *err) {
  std::vector<PngDesc> descs;
  std::vector<int> desc_img;
  std::vector<PngBandRef> bands;
  int64_t nrows = 0;
  size_t stream_total = 0, bound_total = 0;
  auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  for (int i = 0; i < n; i++) {
    out_len[i] = 0;
    const int f = filter ? filter[i] : -1;
    status[i] = enc_io_status(png_enc_check(w[i], h[i], channels[i], f), src[i], src_stride[i], w[i], channels[i], out[i],
                              out_cap[i]);
    if (status[i]) continue;
    PngDesc D{};
    D.src = src[i];
    D.stride = src_stride[i];
    D.W = w[i];
    D.H = h[i];
    D.C = channels[i];
    D.filter = f;
    D.rowbytes = w[i] * channels[i];
    D.nbytes = png_enc_stream_bytes(D.W, D.H, D.C);
    D.nbands = (int32_t)((D.nbytes + kPngBand - 1) / kPngBand);
    D.band0 = (int32_t)bands.size();
    D.row0 = nrows;
    D.stream0 = (int64_t)stream_total;
    png_enc_write_header(D.W, D.H, D.C, D.hdr);
    png_enc_write_iend(D.hdr + kPngHdrBytes);
    if (bands.size() + (size_t)D.nbands > (size_t)1 << 24) {
      *err = "PNG encode batch too large";
      return FI_EINVAL;
    }
    for (int b = 0; b < D.nbands; b++) bands.push_back({(int32_t)descs.size(), b});
    nrows += D.H;
    stream_total += up256((size_t)D.nbytes + 16);
    size_t bnd = 0;
    (void)png_enc_bound(D.W, D.H, D.C, &bnd);
    bound_total += bnd;
    descs.push_back(D);
    desc_img.push_back(i);
  }
  if (descs.empty()) return 0;
  const int nd = (int)descs.size(), nb = (int)bands.size();
  // upload: descriptors, bands
  EncArena up, work;
  const size_t o_desc = up.add(descs.size() * sizeof(PngDesc));
  const size_t o_band = up.add(bands.size() * sizeof(PngBandRef));
  const size_t up_total = up.total();
  // work: filtered streams, symbols, symbol counts, histograms, Adler partials, codes, lengths, destinations,
  // image positions, slots
  const size_t k_stream = work.add(stream_total);
  const size_t k_syms = work.add(stream_total * 4);
  const size_t k_nsym = work.add((size_t)nb * 4);
  const size_t k_hist = work.add((size_t)nb * kPngHist2 * 4);
  const size_t k_adler = work.add((size_t)nb * 8);
  const size_t k_codes = work.add((size_t)nb * sizeof(PngBandCode));
  const size_t k_len = work.add((size_t)nb * 4);
  const size_t k_dst = work.add((size_t)nb * 8);
  const size_t k_pos = work.add((size_t)nd * 16 + 16);  // (+ the fault word behind the positions)
  const size_t k_slots = work.add((size_t)nb * kPngSlotBytes);
  const size_t work_total = work.total();
  uint8_t *dup = (uint8_t *)alloc(actx, 0, up_total);
  uint8_t *hst = (uint8_t *)alloc(actx, 3, std::max(up_total, (size_t)nd * 16 + 16));
  uint8_t *dwork = (uint8_t *)alloc(actx, 1, work_total);
  uint8_t *dpack = (uint8_t *)alloc(actx, 2, bound_total + (size_t)nb * 16);  // (slack: a slot's clamp is per band)
  if (!dup || !hst || !dwork || !dpack) {
    *err = "memory for the PNG encode batch";
    return FI_ENOMEM;
  }
  memcpy(hst + o_desc, descs.data(), descs.size() * sizeof(PngDesc));
  memcpy(hst + o_band, bands.data(), bands.size() * sizeof(PngBandRef));
  if (hipMemcpyAsync(dup, hst, up_total, hipMemcpyHostToDevice, st) != hipSuccess) {
    *err = "PNG encode batch upload";
    return FI_EDEVICE;
  }
  const PngDesc *dd = (const PngDesc *)(dup + o_desc);
  const PngBandRef *db = (const PngBandRef *)(dup + o_band);
  uint8_t *dstream = dwork + k_stream;
  uint32_t *dsyms = (uint32_t *)(dwork + k_syms);
  int32_t *dnsym = (int32_t *)(dwork + k_nsym);
  uint32_t *dhist = (uint32_t *)(dwork + k_hist);
  uint32_t *dadler = (uint32_t *)(dwork + k_adler);
  PngBandCode *dcodes = (PngBandCode *)(dwork + k_codes);
  int32_t *dlen = (int32_t *)(dwork + k_len);
  int64_t *ddst = (int64_t *)(dwork + k_dst);
  int64_t *dpos = (int64_t *)(dwork + k_pos);
  int32_t *dfault = (int32_t *)(dpos + 2 * (size_t)nd);
  uint8_t *dslots = dwork + k_slots;
  if (hipMemsetAsync(dfault, 0, 16, st) != hipSuccess) {
    *err = "PNG encode batch setup";
    return FI_EDEVICE;
  }
  stage(actx, "k_png_filter");
  hipLaunchKernelGGL(k_png_filter, dim3((unsigned)std::min<int64_t>((nrows + 3) / 4, 1 << 20)), dim3(256), 0, st, dd, nd,
                     nrows, dstream);
  stage(actx, "k_png_lz");
  hipLaunchKernelGGL(k_png_lz, dim3((unsigned)nb), dim3(64), 0, st, dd, db, nb, dstream, dsyms, dnsym, dhist, dadler);
  stage(actx, "k_png_codes");
  hipLaunchKernelGGL(k_png_codes, dim3((unsigned)nb), dim3(64), 0, st, dd, db, nb, dhist, dnsym, dcodes);
  stage(actx, "k_png_emit");
  hipLaunchKernelGGL(k_png_emit, dim3((unsigned)nb), dim3(256), 0, st, dd, db, nb, dstream, dsyms, dnsym, dcodes, dadler,
                     dslots, dlen, dfault);
  stage(actx, "k_png_pack");
  hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(256), 0, st, dd, db, nb, dlen, ddst, dpos);
  hipLaunchKernelGGL(k_png_pack, dim3((unsigned)nb), dim3(256), 0, st, nb, dlen, ddst, dslots, dpack);
  stage(actx, nullptr);
  return enc_finish(st, alloc, actx, hst, dpos, nd,
                    "PNG encode: a band's block did not have the size its codes were chosen for", dpack, bound_total,
                    "PNG", desc_img, out, out_cap, out_len, status, true, err);
}
}  // namespace fi
