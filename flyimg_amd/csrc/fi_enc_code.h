// fi_enc_code.h -- the prefix-code and bit-emit layer the GPU PNG encoder
// (fi_png_enc.h) and the GPU lossless WebP encoder (fi_webp_enc.h) share, as
// plain inline functions that compile for the host and the device alike:
// length-limited canonical Huffman codes, the prefix symbols of deflate
// distances and VP8L lengths / distance codes, the run-length coding of a
// code's lengths with its 19-symbol code (deflate's and VP8L's are the same
// but for the order the 19 lengths are sent in), and an LSB-first bit writer.
// What a format frames around them -- HLIT / HDIST / HCLEN, VP8L's form bits
// -- stays with the format.  No HIP header is needed: this header and its
// users build and run under ASan/UBSan on their own
// (tests/native/png_write_driver.cpp, webp_write_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define FI_ENC_HD __host__ __device__ inline
#else
#define FI_ENC_HD inline
#endif

namespace fi {

FI_ENC_HD int enc_ilog2(uint32_t v) { return 31 - __builtin_clz(v); }

// v >= 1 -> its prefix symbol 2 * ilog2(v - 1) + the next bit, the extra bits
// and their value: a deflate distance 1..32768 (symbols 0..29), a VP8L length
// or distance code
FI_ENC_HD int enc_prefix_sym(int v, int *ebits, int *eval) {
  const int d = v - 1;
  if (d < 4) {
    *ebits = 0;
    *eval = 0;
    return d;
  }
  const int e = enc_ilog2((uint32_t)d) - 1;
  *ebits = e;
  *eval = d & ((1 << e) - 1);
  return 2 * e + 2 + ((d >> e) & 1);
}
FI_ENC_HD int enc_prefix_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// What a literal costs in a band of n bytes where its value occurs `count`
// times, in 1/16 bit: the matcher's estimate (the codes do not exist yet).
FI_ENC_HD int enc_literal_cost(uint32_t count, uint32_t n) {
  if (!count) return 240;
  int c = 0;  // 16 * log2(n / count), by the integer part and four squarings
  uint64_t q = ((uint64_t)n << 16) / count;  // >= 1.0 in 16.16
  const int ip = enc_ilog2((uint32_t)(q >> 16));
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

// ---- bits ------------------------------------------------------------------------
struct EncBits {  // LSB-first writer into zeroed words; out == nullptr: only counts
  uint32_t *out;
  int64_t pos, cap;  // bits
  int32_t over;      // a write would have passed cap: nothing of it was written
};
FI_ENC_HD void enc_put(EncBits *b, uint32_t v, int nb) {  // nb <= 32, v below 2^nb
  if (!nb) return;
  if (b->out) {
    if (b->pos + nb > b->cap) {
      b->over = 1;
    } else {
      const int64_t w = b->pos >> 5;
      const int s = (int)(b->pos & 31);
      b->out[w] |= v << s;
      if (s + nb > 32) b->out[w + 1] |= v >> (32 - s);
    }
  }
  b->pos += nb;
}

// ---- code construction -----------------------------------------------------------
struct EncHuffWork {  // scratch of enc_huff_lengths: alphabets of at most 288 symbols
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
FI_ENC_HD void enc_huff_lengths(const uint32_t *freq, int n, int maxbits, uint8_t *len, EncHuffWork *ws) {
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
FI_ENC_HD void enc_huff_codes(const uint8_t *len, int n, int maxbits, uint32_t *tab, uint32_t *work) {
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

// ---- a code's lengths, as deflate and VP8L carry them ------------------------------
// lens[0..n) run-length coded into rle[] (at most n entries: sym | extra << 8):
// 16 repeats the previous length 3..6 times, 17 / 18 are runs of 3..10 /
// 11..138 zeros.  freq[0..19) counts the symbols; returns their number.
FI_ENC_HD int enc_rle_lengths(const uint8_t *lens, int n, uint16_t *rle, uint32_t *freq) {
  int nr = 0;
  for (int i = 0; i < 19; i++) freq[i] = 0;
  for (int i = 0; i < n;) {
    const int v = lens[i];
    int run = 1;
    while (i + run < n && lens[i + run] == v) run++;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        rle[nr++] = (uint16_t)(18 | ((r - 11) << 8));
        freq[18]++;
        run -= r;
      }
      if (run >= 3) {
        rle[nr++] = (uint16_t)(17 | ((run - 3) << 8));
        freq[17]++;
        run = 0;
      }
    } else {
      rle[nr++] = (uint16_t)v;
      freq[v]++;
      run--;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        rle[nr++] = (uint16_t)(16 | ((r - 3) << 8));
        freq[16]++;
        run -= r;
      }
    }
    for (; run > 0; run--) {
      rle[nr++] = (uint16_t)v;
      freq[v]++;
    }
  }
  return nr;
}

// The code of the 19 code-length symbols counted in freq (which it may touch),
// limited to 7 bits: cl_len, cl_tab[s] = (len << 16) | reversed code; work: 34
// words.  Returns how many of the lengths, in the format's order clord, are
// sent: at least 4, up to the last non-zero one.
FI_ENC_HD int enc_cl_code(uint32_t *freq, const uint8_t *clord, uint8_t *cl_len, uint32_t *cl_tab, EncHuffWork *huff,
                          uint32_t *work) {
  int clused = 0;
  for (int i = 0; i < 19; i++) clused += freq[i] != 0;
  if (clused < 2) freq[freq[0] ? 1 : 0] = 1;  // never a one-symbol code-length code
  enc_huff_lengths(freq, 19, 7, cl_len, huff);
  enc_huff_codes(cl_len, 19, 7, cl_tab, work);
  int ncl = 19;
  while (ncl > 4 && !cl_len[clord[ncl - 1]]) ncl--;
  return ncl;
}

// the coded lengths: every symbol of rle[0..nr) in the code cl_tab, 16 / 17 / 18 with their 2 / 3 / 7 extra bits
FI_ENC_HD void enc_put_rle(EncBits *b, const uint16_t *rle, int nr, const uint32_t *cl_tab) {
  for (int i = 0; i < nr; i++) {
    const int s = rle[i] & 255, ex = rle[i] >> 8;
    enc_put(b, cl_tab[s] & 0xFFFFu, (int)(cl_tab[s] >> 16));
    if (s == 16) enc_put(b, (uint32_t)ex, 2);
    if (s == 17) enc_put(b, (uint32_t)ex, 3);
    if (s == 18) enc_put(b, (uint32_t)ex, 7);
  }
}

}  // namespace fi
