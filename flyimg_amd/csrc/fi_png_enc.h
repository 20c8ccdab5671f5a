// fi_png_enc.h -- what the GPU PNG encoder's device half (fi_png_enc.hip) and
// host half (fi_png_write.cpp) share: the band geometry, the size bound, the
// file's fixed chunks, and -- as plain inline functions that compile for the
// host and the device alike -- the deflate symbol mapping, the CRC-32 and
// Adler-32 combination and the per-band code construction (length-limited
// canonical Huffman codes + the dynamic block header).  No HIP header is
// needed: the host half and this header build and run under ASan/UBSan on
// their own (tests/native/png_write_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define FI_PNG_HD __host__ __device__ inline
#else
#define FI_PNG_HD inline
#endif

namespace fi {

constexpr int kPngBand = 32768;      // bytes of the filtered stream per band (one deflate block sequence, one IDAT)
constexpr int kPngHdrBytes = 33;     // signature + IHDR chunk
constexpr int kPngLL = 288, kPngD = 32;  // histogram / table strides of the lit/len and distance alphabets
constexpr int kPngHist = kPngLL + kPngD;
constexpr int kPngHist2 = kPngHist + 256;  // a band's record: the parse's histograms, then the plain byte counts
constexpr int kPngShortBand = 4096;  // bands up to this size try shorter code-length limits (png_build_block)
constexpr int kPngHdrWords = 160;    // dynamic block header: 14 + 19 * 3 + 316 * 14 bits at most

// 0, or FI_EINVAL / FI_EUNSUPPORTED as fi_png_encode_device documents them
int png_enc_check(int w, int h, int channels, int filter);
// bytes of the filtered stream h * (w * channels + 1) and its bands
int64_t png_enc_stream_bytes(int w, int h, int channels);
// upper bound of the whole file (every band stored); 0 = OK
int png_enc_bound(int w, int h, int channels, size_t *bytes);
// signature + IHDR (33 bytes) / the IEND chunk (12 bytes)
void png_enc_write_header(int w, int h, int channels, uint8_t out[kPngHdrBytes]);
void png_enc_write_iend(uint8_t out[12]);
uint32_t png_crc32(uint32_t crc, const uint8_t *p, size_t n);  // zlib's crc32()

// bytes a band of n filtered bytes takes as stored blocks
FI_PNG_HD int png_stored_bytes(int n) { return n + 5 * ((n + 65534) / 65535); }

// ---- deflate symbols ---------------------------------------------------------
FI_PNG_HD int png_ilog2(uint32_t v) { return 31 - __builtin_clz(v); }
// length 3..258 -> lit/len symbol 257..285, its extra bits and their value
FI_PNG_HD int png_len_sym(int len, int *ebits, int *eval) {
  const int l = len - 3;
  if (l < 8 || len == 258) {
    *ebits = 0;
    *eval = 0;
    return len == 258 ? 285 : 257 + l;
  }
  const int e = png_ilog2((uint32_t)l) - 2;
  *ebits = e;
  *eval = l & ((1 << e) - 1);
  return 261 + 4 * e + ((l - (4 << e)) >> e);
}
// distance 1..32768 -> distance symbol 0..29
FI_PNG_HD int png_dist_sym(int dist, int *ebits, int *eval) {
  const int d = dist - 1;
  if (d < 4) {
    *ebits = 0;
    *eval = 0;
    return d;
  }
  const int e = png_ilog2((uint32_t)d) - 1;
  *ebits = e;
  *eval = d & ((1 << e) - 1);
  return 2 * e + 2 + ((d >> e) & 1);
}
FI_PNG_HD int png_len_extra(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
FI_PNG_HD int png_dist_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// What a literal costs in a band of n bytes where its value occurs `count`
// times, in 1/16 bit: the matcher's estimate (the codes do not exist yet).
FI_PNG_HD int png_literal_cost(uint32_t count, uint32_t n) {
  if (!count) return 240;
  int c = 0;  // 16 * log2(n / count), by the integer part and four squarings
  uint64_t q = ((uint64_t)n << 16) / count;  // >= 1.0 in 16.16
  const int ip = png_ilog2((uint32_t)(q >> 16));
  c = 16 * ip;
  uint64_t f = q >> ip;  // [1, 2) in 16.16
  for (int k = 8; k; k >>= 1) {
    f = (f * f) >> 16;
    if (f >= (2u << 16)) {
      f >>= 1;
      c += k;
    }
  }
  return c < 16 ? 16 : c > 240 ? 240 : c;
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320) ---------------------------------
// One byte through the register, bit by bit (the kernels build their 256-entry
// table from it).
FI_PNG_HD uint32_t png_crc_byte(uint32_t c) {
  for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  return c;
}
// a * b mod P in the reflected representation (bit 31 = x^0)
FI_PNG_HD uint32_t png_crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int k = 0; k < 32; k++) {
    r ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return r;
}
// x^(8 n) mod P
FI_PNG_HD uint32_t png_crc_xpow8(uint64_t n) {
  uint32_t r = 0x80000000u;  // x^0
  uint32_t sq = 0x00800000u; // x^8
  for (; n; n >>= 1) {
    if (n & 1) r = png_crc_mulmod(r, sq);
    sq = png_crc_mulmod(sq, sq);
  }
  return r;
}
// crc32(A || B) from crc32(A), crc32(B) and B's length
FI_PNG_HD uint32_t png_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return png_crc_mulmod(crc_a, png_crc_xpow8(len_b)) ^ crc_b;
}

// ---- Adler-32 ------------------------------------------------------------------
// A band of n bytes d[0..n-1] contributes sa = sum d[i] and sb = sum (n - i) d[i],
// both mod 65521; (a, b) is the running checksum (1, 0 before the first byte).
FI_PNG_HD void png_adler_append(uint32_t *a, uint32_t *b, uint32_t sa, uint32_t sb, uint32_t n) {
  *b = (uint32_t)((*b + (uint64_t)(n % 65521u) * *a + sb) % 65521u);
  *a = (*a + sa) % 65521u;
}

// ---- code construction -----------------------------------------------------------
struct PngHuffWork {  // scratch of png_huff_lengths: alphabets of at most 288 symbols
  uint16_t order[2][288];
  uint32_t weight[288];  // internal nodes
  uint16_t iparent[288], lparent[288];
  uint16_t count[256];
  uint16_t blcount[34];
};

// Length-limited Huffman code lengths of freq[0..n-1] (n <= 288, the sum below
// 2^32): len[s] = 0 for unused symbols, 1..maxbits otherwise; one used symbol
// gets one bit.  Symbols are sorted by (frequency, index) with a byte-wise
// counting sort, the tree comes from the two-queue merge, and lengths beyond
// maxbits are folded back by moving the Kraft excess down from the longest
// codes; the shortest lengths then go to the most frequent symbols.
FI_PNG_HD void png_huff_lengths(const uint32_t *freq, int n, int maxbits, uint8_t *len, PngHuffWork *ws) {
  int m = 0;
  uint32_t fmax = 0;
  for (int s = 0; s < n; s++) {
    len[s] = 0;
    if (freq[s]) {
      ws->order[0][m++] = (uint16_t)s;
      if (freq[s] > fmax) fmax = freq[s];
    }
  }
  if (m == 0) return;
  if (m == 1) {
    len[ws->order[0][0]] = 1;
    return;
  }
  int cur = 0;
  for (int shift = 0; shift < 32 && (fmax >> shift); shift += 8) {
    for (int i = 0; i < 256; i++) ws->count[i] = 0;
    for (int i = 0; i < m; i++) ws->count[(freq[ws->order[cur][i]] >> shift) & 255u]++;
    int acc = 0;
    for (int i = 0; i < 256; i++) {
      const int c = ws->count[i];
      ws->count[i] = (uint16_t)acc;
      acc += c;
    }
    for (int i = 0; i < m; i++) {
      const uint16_t s = ws->order[cur][i];
      ws->order[cur ^ 1][ws->count[(freq[s] >> shift) & 255u]++] = s;
    }
    cur ^= 1;
  }
  const uint16_t *ord = ws->order[cur];
  // two queues: leaves ord[leaf..], internal nodes weight[node..made)
  int leaf = 0, node = 0;
  for (int made = 0; made < m - 1; made++) {
    uint32_t wsum = 0;
    for (int k = 0; k < 2; k++) {
      if (leaf < m && (node >= made || freq[ord[leaf]] <= ws->weight[node])) {
        wsum += freq[ord[leaf]];
        ws->lparent[leaf++] = (uint16_t)made;
      } else {
        wsum += ws->weight[node];
        ws->iparent[node++] = (uint16_t)made;
      }
    }
    ws->weight[made] = wsum;
  }
  // depths: the root is node m - 2; a parent has a higher index than its children
  ws->iparent[m - 2] = 0;  // (its depth)
  for (int k = m - 3; k >= 0; k--) ws->iparent[k] = (uint16_t)(ws->iparent[ws->iparent[k]] + 1);
  for (int i = 0; i <= 32; i++) ws->blcount[i] = 0;
  for (int i = 0; i < m; i++) {
    int d = ws->iparent[ws->lparent[i]] + 1;
    if (d > maxbits) d = maxbits;
    ws->blcount[d]++;
  }
  uint32_t total = 0;
  for (int l = 1; l <= maxbits; l++) total += (uint32_t)ws->blcount[l] << (maxbits - l);
  while (total > (1u << maxbits)) {
    ws->blcount[maxbits]--;
    for (int l = maxbits - 1; l >= 1; l--)
      if (ws->blcount[l]) {
        ws->blcount[l]--;
        ws->blcount[l + 1] += 2;
        break;
      }
    total--;
  }
  int i = 0;
  for (int l = maxbits; l >= 1; l--)
    for (int k = ws->blcount[l]; k > 0; k--) len[ord[i++]] = (uint8_t)l;
}

// canonical codes (RFC 1951 3.2.2) of len[0..n-1], bit-reversed for the
// LSB-first stream: tab[s] = (len << 16) | reversed code; work: 34 words
FI_PNG_HD void png_huff_codes(const uint8_t *len, int n, int maxbits, uint32_t *tab, uint32_t *work) {
  uint32_t *next = work, *cnt = work + 17;
  for (int l = 0; l <= 16; l++) cnt[l] = 0;
  for (int s = 0; s < n; s++) cnt[len[s]]++;
  cnt[0] = 0;
  uint32_t code = 0;
  next[0] = 0;
  for (int l = 1; l <= maxbits; l++) {
    code = (code + cnt[l - 1]) << 1;
    next[l] = code;
  }
  for (int s = 0; s < n; s++) {
    const int l = len[s];
    uint32_t r = 0;
    if (l) {
      const uint32_t c = next[l]++;
      for (int k = 0; k < l; k++) r |= ((c >> k) & 1u) << (l - 1 - k);
    }
    tab[s] = ((uint32_t)l << 16) | r;
  }
}

struct PngBandCode {         // what k_png_emit needs of a band's dynamic block
  uint32_t ll[kPngLL];       // (len << 16) | reversed code
  uint32_t dist[kPngD];
  uint32_t hdr[kPngHdrWords];  // HLIT .. the coded code lengths, LSB first
  int32_t hdr_bits;
  int32_t block_bits;        // BFINAL + BTYPE + header + symbols + end of block
  int32_t stored;            // 1: the band goes out as stored blocks
  int32_t btype;             // otherwise 2: dynamic codes, 1: the fixed codes (no header; short bands)
  int32_t literal;           // 1: the band's bytes go out as literals (the parse's matches did not pay)
};
struct PngCodeWork {  // scratch of png_build_block
  PngHuffWork huff;
  uint32_t freq[kPngLL];
  uint8_t lens[kPngLL + kPngD];  // lit/len lengths, then distance lengths
  uint8_t cl_len[19];
  uint32_t cl_tab[19];
  uint32_t codes_work[34];  // png_huff_codes
  uint16_t rle[kPngLL + kPngD];  // code-length symbols: sym | extra << 8
  int32_t nrle;
};

// The dynamic codes and header of a band with lit/len codes of at most llmax
// bits (the used symbols must number at most 2^llmax): fills out->ll, dist,
// hdr, hdr_bits; returns the bits of the whole block.
FI_PNG_HD int64_t png_build_dynamic(const uint32_t *hist, int llmax, PngBandCode *out, PngCodeWork *ws) {
  constexpr uint8_t clord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint8_t *ll_len = ws->lens, *d_len = ws->lens + kPngLL;
  for (int s = 0; s < kPngLL; s++) ws->freq[s] = s < 286 ? hist[s] : 0;
  ws->freq[256] = 1;
  png_huff_lengths(ws->freq, 286, llmax, ll_len, &ws->huff);
  // at least two distance codes, as zlib writes them: every inflater accepts that
  int dused = 0;
  for (int s = 0; s < kPngD; s++) {
    ws->freq[s] = s < 30 ? hist[kPngLL + s] : 0;
    dused += ws->freq[s] != 0;
  }
  for (int s = 0; s < 2 && dused < 2; s++)
    if (!ws->freq[s]) {
      ws->freq[s] = 1;
      dused++;
    }
  png_huff_lengths(ws->freq, 30, 15, d_len, &ws->huff);
  png_huff_codes(ll_len, 286, 15, out->ll, ws->codes_work);
  png_huff_codes(d_len, 30, 15, out->dist, ws->codes_work);
  int hlit = 286, hdist = 30;
  while (hlit > 257 && !ll_len[hlit - 1]) hlit--;
  while (hdist > 1 && !d_len[hdist - 1]) hdist--;
  // the lengths as one sequence, run-length coded with 16 / 17 / 18
  for (int s = 0; s < hdist; s++) ws->lens[hlit + s] = d_len[s];  // (hlit <= kPngLL: moves down or stays)
  const int nl = hlit + hdist;
  int nr = 0;
  for (int i = 0; i < 19; i++) ws->freq[i] = 0;
  for (int i = 0; i < nl;) {
    const int v = ws->lens[i];
    int run = 1;
    while (i + run < nl && ws->lens[i + run] == v) run++;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        ws->rle[nr++] = (uint16_t)(18 | ((r - 11) << 8));
        ws->freq[18]++;
        run -= r;
      }
      if (run >= 3) {
        ws->rle[nr++] = (uint16_t)(17 | ((run - 3) << 8));
        ws->freq[17]++;
        run = 0;
      }
    } else {
      ws->rle[nr++] = (uint16_t)v;
      ws->freq[v]++;
      run--;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        ws->rle[nr++] = (uint16_t)(16 | ((r - 3) << 8));
        ws->freq[16]++;
        run -= r;
      }
    }
    for (; run > 0; run--) {
      ws->rle[nr++] = (uint16_t)v;
      ws->freq[v]++;
    }
  }
  ws->nrle = nr;
  int clused = 0;
  for (int i = 0; i < 19; i++) clused += ws->freq[i] != 0;
  if (clused < 2) ws->freq[ws->freq[0] ? 1 : 0] = 1;  // never a one-symbol code-length code
  png_huff_lengths(ws->freq, 19, 7, ws->cl_len, &ws->huff);
  png_huff_codes(ws->cl_len, 19, 7, ws->cl_tab, ws->codes_work);
  int hclen = 19;
  while (hclen > 4 && !ws->cl_len[clord[hclen - 1]]) hclen--;
  // header bits, LSB first
  for (int i = 0; i < kPngHdrWords; i++) out->hdr[i] = 0;
  int pos = 0;
  bool over = false;  // (kPngHdrWords holds the longest header there is)
  auto put = [&](uint32_t v, int nb) {
    if (!nb) return;
    if (pos + nb > kPngHdrWords * 32) {
      over = true;
      return;
    }
    out->hdr[pos >> 5] |= v << (pos & 31);
    if ((pos & 31) + nb > 32) out->hdr[(pos >> 5) + 1] |= v >> (32 - (pos & 31));
    pos += nb;
  };
  put((uint32_t)(hlit - 257), 5);
  put((uint32_t)(hdist - 1), 5);
  put((uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; i++) put(ws->cl_len[clord[i]], 3);
  for (int i = 0; i < nr; i++) {
    const int s = ws->rle[i] & 255, ex = ws->rle[i] >> 8;
    put(ws->cl_tab[s] & 0xFFFFu, (int)(ws->cl_tab[s] >> 16));
    if (s == 16) put((uint32_t)ex, 2);
    if (s == 17) put((uint32_t)ex, 3);
    if (s == 18) put((uint32_t)ex, 7);
  }
  out->hdr_bits = pos;
  if (over) return (int64_t)1 << 40;  // not a block: the caller takes the fixed codes or stored blocks
  int64_t bits = 3 + pos + (out->ll[256] >> 16);
  for (int s = 0; s < 286; s++)
    if (s != 256) bits += (int64_t)hist[s] * ((out->ll[s] >> 16) + (uint32_t)png_len_extra(s));
  for (int s = 0; s < 30; s++) bits += (int64_t)hist[kPngLL + s] * ((out->dist[s] >> 16) + (uint32_t)png_dist_extra(s));
  return bits;
}

// The block of a band from its histograms hist[0..kPngHist) (lit/len at 0,
// distances at kPngLL; the end-of-block symbol is counted here).  Fills *out
// and decides between stored, fixed and dynamic codes, whichever is smallest:
// n = the band's bytes, last = it ends the stream (no alignment block after
// it).  In a band of a few hundred bytes the header is a tenth of the block
// and every distinct code length costs there, so short bands also try codes
// limited to 10, 9, 8 and 7 bits and keep the smallest block.
FI_PNG_HD void png_build_block(const uint32_t *hist, int n, bool last, PngBandCode *out, PngCodeWork *ws) {
  int best = 15;
  int64_t bits = png_build_dynamic(hist, 15, out, ws);
  if (n <= kPngShortBand) {
    int used = 1;
    for (int s = 0; s < 286; s++) used += s != 256 && hist[s] != 0;
    int built = 15;
    for (int lim = 10; lim >= 7 && used <= (1 << lim); lim--) {
      const int64_t b = png_build_dynamic(hist, lim, out, ws);
      built = lim;
      if (b < bits) {
        bits = b;
        best = lim;
      }
    }
    if (built != best) bits = png_build_dynamic(hist, best, out, ws);
  }
  out->btype = 2;
  // the fixed codes (RFC 1951 3.2.6) carry no header: the better form of a band of a few bytes
  int64_t fbits = 3 + 7;
  for (int s = 0; s < 286; s++)
    if (s != 256) fbits += (int64_t)hist[s] * ((s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8) + png_len_extra(s));
  for (int s = 0; s < 30; s++) fbits += (int64_t)hist[kPngLL + s] * (5 + png_dist_extra(s));
  if (fbits < bits) {
    for (int s = 0; s < kPngLL; s++) ws->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < kPngD; s++) ws->lens[kPngLL + s] = 5;
    png_huff_codes(ws->lens, kPngLL, 15, out->ll, ws->codes_work);
    png_huff_codes(ws->lens + kPngLL, kPngD, 15, out->dist, ws->codes_work);
    out->hdr_bits = 0;
    out->btype = 1;
    bits = fbits;
  }
  out->block_bits = (int32_t)bits;
  // behind a dynamic block that does not end the stream: an empty stored block
  // (3 header bits, padding, LEN, NLEN) brings the next band to a byte boundary
  const int64_t dyn_bytes = last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
  out->stored = dyn_bytes >= png_stored_bytes(n) ? 1 : 0;
  out->literal = 0;
}

}  // namespace fi
