// fi_webp_enc.h -- the GPU lossless WebP (VP8L) encoder's algorithm, shared by
// its device half (fi_webp_enc.hip) and its host half (fi_webp_write.cpp) as
// plain inline functions over (lane, nlanes): the kernels run them with
// (threadIdx.x, 64) in a workgroup of one wave, the host with (0, 1).  Every
// choice is defined on 64-position groups, per-block sums and maxima, never on
// the lane count, so both produce the same bytes: the host file
// (fi_debug_webp_encode_host) is the specification of the device's file.  No
// HIP header is needed: the host half and this header build and run under
// ASan/UBSan on their own (tests/native/webp_write_driver.cpp).
//
// The file: RIFF / WEBP / VP8L, subtract-green, a predictor transform with one
// mode per 16 x 16 block, backward references inside bands of kWebpBand pixels
// (distance codes d + 120 only), one Huffman group, no colour cache.  The
// fallback form -- no predictor, no references, flat 8-bit codes for every
// channel that varies -- costs exactly w * h * channels bytes plus a constant
// header and is the size bound; the encoder prices both forms and writes the
// smaller.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fi_enc_code.h"

// (fi_webp_enc.hip defines FI_WEBP_DEVICE behind hip_runtime.h: only there do the functions run on the device)
#if defined(FI_WEBP_DEVICE) && defined(__HIP_DEVICE_COMPILE__)
#define FI_WEBP_SYNC() __syncthreads()
#define FI_WEBP_ADD(p, v) atomicAdd((p), (v))
#define FI_WEBP_MAX(p, v) atomicMax((p), (v))
#else
#define FI_WEBP_SYNC() ((void)0)
#define FI_WEBP_ADD(p, v) (*(p) += (v))
#define FI_WEBP_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#endif

namespace fi {

constexpr int kWebpBand = 8192;      // residual pixels per band: references stay inside it
constexpr int kWebpMaxLen = 4096;    // longest copy
constexpr int kWebpHashBits = 12;
constexpr int kWebpBlockBits = 4;    // 16 x 16 predictor blocks
constexpr int kWebpG = 280, kWebpD = 40;  // green + length symbols; distance symbols
constexpr int kWebpOffG = 0, kWebpOffR = 280, kWebpOffB = 536, kWebpOffA = 792, kWebpOffD = 1048;
constexpr int kWebpHist = 1088;      // the five histograms / code tables of an image, back to back
constexpr int kWebpRiffBytes = 20;   // RIFF size WEBP VP8L length
constexpr int kWebpMaxSide = 16384;

struct WebpImg {         // one image of an encode batch
  const uint8_t *src;    // HWC u8, 1..4 channels
  int64_t stride;
  int32_t W, H, C, pred;  // pred: -1 adaptive, 0..13 that mode on every block
  int32_t bw, bh;        // predictor blocks across / down
  int32_t npix, nbands;
  int32_t band0;         // its first band in the batch
  int32_t fb_hdr;        // payload bits before the first token in the fallback form (webp_fallback_hdr_bits)
  int64_t block0;        // its first predictor block in the batch (and its offset in the mode array)
  int64_t px0;           // its first pixel in the batch (residuals, tokens)
  int64_t slot0;         // byte offset of its output slot (16-byte aligned)
  int64_t slot_bytes;    // multiple of 16, above the bound
};
struct WebpImgOut {      // what webp_build_image decides
  int32_t fallback;      // 1: the fallback form
  int32_t hdr_bits;      // payload bits before the first token
  int64_t total_bits;    // payload bits
  int64_t file_bytes;
};
struct WebpBandRef {
  int32_t img, idx;
};

// 0, or FI_EINVAL / FI_EUNSUPPORTED as fi_webp_encode_device documents them
int webp_enc_check(int w, int h, int channels, int predictor);
// the fallback form's payload bits before the first token: a function of the channel count alone
int webp_fallback_hdr_bits(int channels);
// upper bound of the whole file (the fallback form); 0 = OK
int webp_enc_bound(int w, int h, int channels, size_t *bytes);
// the host form: the device's file.  0, FI_EINVAL, FI_EUNSUPPORTED, FI_ENOMEM
// (out_len = the size needed, nothing written) or FI_EDEVICE if what was
// emitted differs from what was priced
int webp_encode_host(const uint8_t *src, int w, int h, int channels, int64_t stride, int predictor, uint8_t *out,
                     size_t out_cap, size_t *out_len);

FI_ENC_HD int webp_min(int a, int b) { return a < b ? a : b; }

// ---- pixels -------------------------------------------------------------------
// (A, R, G, B) of pixel (x, y): gray replicates, alpha 255 where the source has none; sg: subtract green
FI_ENC_HD uint32_t webp_px(const WebpImg &I, int x, int y, bool sg) {
  const uint8_t *p = I.src + (int64_t)y * I.stride + (int64_t)x * I.C;
  uint32_t a = 255, r, g, b;
  if (I.C <= 2) {
    r = g = b = p[0];
    if (I.C == 2) a = p[1];
  } else {
    r = p[0];
    g = p[1];
    b = p[2];
    if (I.C == 4) a = p[3];
  }
  if (sg) {
    r = (r - g) & 255u;
    b = (b - g) & 255u;
  }
  return (a << 24) | (r << 16) | (g << 8) | b;
}
FI_ENC_HD uint32_t webp_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
FI_ENC_HD uint32_t webp_sub(uint32_t a, uint32_t b) {  // per channel mod 256
  const uint32_t ag = 0x00FF00FFu + (a & 0xFF00FF00u) - (b & 0xFF00FF00u);
  const uint32_t rb = 0xFF00FF00u + (a & 0x00FF00FFu) - (b & 0x00FF00FFu);
  return (ag & 0xFF00FF00u) | (rb & 0x00FF00FFu);
}
FI_ENC_HD int webp_clip(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
FI_ENC_HD int webp_abs(int v) { return v < 0 ? -v : v; }
// sum over the four residual bytes of min(x, 256 - x)
FI_ENC_HD uint32_t webp_cost4(uint32_t v) {
  uint32_t c = 0;
  for (int s = 0; s < 32; s += 8) {
    const uint32_t x = (v >> s) & 255u;
    c += x < 128 ? x : 256 - x;
  }
  return c;
}
FI_ENC_HD uint32_t webp_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (mode) {
    case 0: return 0xFF000000u;
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return webp_avg2(webp_avg2(L, TR), T);
    case 6: return webp_avg2(L, TL);
    case 7: return webp_avg2(L, T);
    case 8: return webp_avg2(TL, T);
    case 9: return webp_avg2(T, TR);
    case 10: return webp_avg2(webp_avg2(L, TL), webp_avg2(T, TR));
    case 11: {
      int st = 0, sl = 0;  // sum |T - TL|, sum |L - TL|
      for (int s = 0; s < 32; s += 8) {
        const int l = (L >> s) & 255, t = (T >> s) & 255, c = (TL >> s) & 255;
        st += webp_abs(t - c);
        sl += webp_abs(l - c);
      }
      return st < sl ? L : T;
    }
    case 12: {
      uint32_t r = 0;
      for (int s = 0; s < 32; s += 8)
        r |= (uint32_t)webp_clip((int)((L >> s) & 255) + (int)((T >> s) & 255) - (int)((TL >> s) & 255)) << s;
      return r;
    }
    default: {
      const uint32_t A = webp_avg2(L, T);
      uint32_t r = 0;
      for (int s = 0; s < 32; s += 8) {
        const int a = (A >> s) & 255, c = (TL >> s) & 255;
        r |= (uint32_t)webp_clip(a + (a - c) / 2) << s;
      }
      return r;
    }
  }
}
// the prediction of pixel (x, y) under `mode`, borders included
FI_ENC_HD uint32_t webp_pred_at(const WebpImg &I, int mode, int x, int y) {
  if (y == 0) return x == 0 ? 0xFF000000u : webp_px(I, x - 1, 0, true);
  if (x == 0) return webp_px(I, 0, y - 1, true);
  const uint32_t L = webp_px(I, x - 1, y, true), T = webp_px(I, x, y - 1, true), TL = webp_px(I, x - 1, y - 1, true);
  const uint32_t TR = x == I.W - 1 ? webp_px(I, 0, y, true) : webp_px(I, x + 1, y - 1, true);
  return webp_predict(mode, L, T, TL, TR);
}

// One predictor block: the mode (the cheapest of the 14 by the sum of
// min(x, 256 - x) over the block's residual bytes, ties to the lower mode; the
// border pixels, whose prediction no mode changes, do not count), the mode
// image entry and the block's residuals.  cost: 16 words all lanes share.
FI_ENC_HD void webp_pred_block(const WebpImg &I, int blk, int lane, int nlanes, uint32_t *cost, uint32_t *resid,
                               uint8_t *modes) {
  const int bx = blk % I.bw, by = blk / I.bw, x0 = bx << kWebpBlockBits, y0 = by << kWebpBlockBits;
  const int bwid = webp_min(16, I.W - x0), bhei = webp_min(16, I.H - y0);
  int mode = I.pred;
  if (mode < 0) {
    for (int m = lane; m < 16; m += nlanes) cost[m] = 0;
    FI_WEBP_SYNC();
    uint32_t c[14];
    for (int m = 0; m < 14; m++) c[m] = 0;
    for (int i = lane; i < 256; i += nlanes) {
      const int x = x0 + (i & 15), y = y0 + (i >> 4);
      if ((i & 15) >= bwid || (i >> 4) >= bhei || x == 0 || y == 0) continue;
      const uint32_t cur = webp_px(I, x, y, true);
      const uint32_t L = webp_px(I, x - 1, y, true), T = webp_px(I, x, y - 1, true), TL = webp_px(I, x - 1, y - 1, true);
      const uint32_t TR = x == I.W - 1 ? webp_px(I, 0, y, true) : webp_px(I, x + 1, y - 1, true);
      for (int m = 0; m < 14; m++) c[m] += webp_cost4(webp_sub(cur, webp_predict(m, L, T, TL, TR)));
    }
    for (int m = 0; m < 14; m++)
      if (c[m]) FI_WEBP_ADD(&cost[m], c[m]);
    FI_WEBP_SYNC();
    mode = 0;
    for (int m = 1; m < 14; m++)
      if (cost[m] < cost[mode]) mode = m;
  }
  for (int i = lane; i < 256; i += nlanes) {
    const int x = x0 + (i & 15), y = y0 + (i >> 4);
    if ((i & 15) >= bwid || (i >> 4) >= bhei) continue;
    resid[(int64_t)y * I.W + x] = webp_sub(webp_px(I, x, y, true), webp_pred_at(I, mode, x, y));
  }
  if (lane == 0) modes[blk] = (uint8_t)mode;
}

// ---- backward references (lengths and distance codes: enc_prefix_sym) ------------
struct WebpLzWork {  // a band's working set (LDS on the device)
  uint32_t px[kWebpBand];
  uint32_t tab[1 << kWebpHashBits];  // position + 1 of the last two-pixel prefix with this hash; 0: none
  uint32_t hist[kWebpHist];
  uint32_t cnt[4 * 256];  // byte counts per channel: A, R, G, B
  uint8_t lcost[4 * 256];  // what a literal byte costs, in 1/16 bit (enc_literal_cost; 0 for a constant channel)
  int32_t gcand[64], ghash[64], glen[64], gdist[64];  // the current group of 64 positions
};

FI_ENC_HD int webp_match_len(const uint32_t *px, int p, int cand, int maxl) {
  int l = 0;
  while (l < maxl && px[p + l] == px[cand + l]) l++;
  return l;
}

// A token is a literal's position in the band, or 1 << 31 | (distance - 1) <<
// 12 | (length - 1).  The hash table moves 64 positions at a time, so a hash
// candidate lies in an earlier group; the pixel before is a candidate too (runs).
// The parse is greedy: take the match at the position, advance by its length.
// A match of up to 8 pixels is taken only where it costs less than its literals
// would by the band's byte counts.
FI_ENC_HD void webp_lz_band(const uint32_t *src, int n, int lane, int nlanes, WebpLzWork *S, uint32_t *tok,
                            int32_t *ntok, uint32_t *bandhist, uint32_t *imghist) {
  for (int i = lane; i < kWebpHist; i += nlanes) S->hist[i] = 0;
  for (int i = lane; i < 4 * 256; i += nlanes) S->cnt[i] = 0;
  for (int i = lane; i < (1 << kWebpHashBits); i += nlanes) S->tab[i] = 0;
  FI_WEBP_SYNC();
  for (int i = lane; i < n; i += nlanes) {
    const uint32_t v = src[i];
    S->px[i] = v;
    FI_WEBP_ADD(&S->cnt[v >> 24], 1u);
    FI_WEBP_ADD(&S->cnt[256 + ((v >> 16) & 255u)], 1u);
    FI_WEBP_ADD(&S->cnt[512 + ((v >> 8) & 255u)], 1u);
    FI_WEBP_ADD(&S->cnt[768 + (v & 255u)], 1u);
  }
  FI_WEBP_SYNC();
  for (int i = lane; i < 4 * 256; i += nlanes)
    S->lcost[i] = S->cnt[i] == (uint32_t)n ? 0 : (uint8_t)enc_literal_cost(S->cnt[i], (uint32_t)n);
  FI_WEBP_SYNC();
  int pos = 0, nt = 0;  // the same in every lane: the parse position, tokens written
  for (int p0 = 0; p0 < n; p0 += 64) {
    for (int k = lane; k < 64; k += nlanes) {
      const int p = p0 + k;
      int h = -1, cand = -1;
      if (p + 1 < n) {
        h = (int)(((S->px[p] * 0x9E3779B1u + S->px[p + 1]) * 0x85EBCA6Bu) >> (32 - kWebpHashBits));
        cand = (int)S->tab[h] - 1;
      }
      S->ghash[k] = h;
      S->gcand[k] = cand;
    }
    FI_WEBP_SYNC();  // every position has its candidate (from an earlier group) before the table moves on
    for (int k = lane; k < 64; k += nlanes)
      if (S->ghash[k] >= 0) FI_WEBP_MAX(&S->tab[S->ghash[k]], (uint32_t)(p0 + k + 1));
    FI_WEBP_SYNC();
    if (pos >= p0 + 64) continue;  // the whole group lies inside the last match
    for (int k = lane; k < 64; k += nlanes) {
      const int p = p0 + k;
      int mlen = 0, mdist = 0;
      if (p >= pos && p < n && p > 0) {
        const int maxl = webp_min(kWebpMaxLen, n - p);
        const int cand = S->gcand[k];
        int l = webp_match_len(S->px, p, p - 1, maxl), d = 1;
        if (cand >= 0 && cand != p - 1) {
          const int l2 = webp_match_len(S->px, p, cand, maxl);
          if (l2 > l) {
            l = l2;
            d = p - cand;
          }
        }
        if (l >= 1) {
          bool pays = true;
          if (l <= 8) {
            int eb, ev, el, lit = 0;
            (void)enc_prefix_sym(d + 120, &eb, &ev);
            (void)enc_prefix_sym(l, &el, &ev);
            for (int j = 0; j < l; j++) {
              const uint32_t v = S->px[p + j];
              lit += S->lcost[v >> 24] + S->lcost[256 + ((v >> 16) & 255u)] + S->lcost[512 + ((v >> 8) & 255u)] +
                     S->lcost[768 + (v & 255u)];
            }
            pays = 16 * (12 + eb + el) < lit;
          }
          if (pays) {
            mlen = l;
            mdist = d;
          }
        }
      }
      S->glen[k] = mlen;
      S->gdist[k] = mdist;
    }
    FI_WEBP_SYNC();
    uint64_t mask = 0;  // the positions the greedy parse lands on
    const int end = webp_min(p0 + 64, n);
    while (pos < end) {
      const int k = pos - p0, l = S->glen[k];
      mask |= 1ull << k;
      pos += l ? l : 1;
    }
    for (int k = lane; k < 64; k += nlanes) {
      if (!((mask >> k) & 1ull)) continue;
      const int at = nt + __builtin_popcountll(mask & ((1ull << k) - 1ull));
      const int l = S->glen[k];
      if (l) {
        tok[at] = 0x80000000u | ((uint32_t)(S->gdist[k] - 1) << 12) | (uint32_t)(l - 1);
        int eb, ev;
        FI_WEBP_ADD(&S->hist[256 + enc_prefix_sym(l, &eb, &ev)], 1u);
        FI_WEBP_ADD(&S->hist[kWebpOffD + enc_prefix_sym(S->gdist[k] + 120, &eb, &ev)], 1u);
      } else {
        const uint32_t v = S->px[p0 + k];
        tok[at] = (uint32_t)(p0 + k);
        FI_WEBP_ADD(&S->hist[kWebpOffG + ((v >> 8) & 255u)], 1u);
        FI_WEBP_ADD(&S->hist[kWebpOffR + ((v >> 16) & 255u)], 1u);
        FI_WEBP_ADD(&S->hist[kWebpOffB + (v & 255u)], 1u);
        FI_WEBP_ADD(&S->hist[kWebpOffA + (v >> 24)], 1u);
      }
    }
    nt += __builtin_popcountll(mask);
    FI_WEBP_SYNC();  // the group's lengths are read before the next group writes its own
  }
  FI_WEBP_SYNC();
  for (int i = lane; i < kWebpHist; i += nlanes) {
    const uint32_t v = S->hist[i];
    bandhist[i] = v;
    if (v) FI_WEBP_ADD(&imghist[i], v);
  }
  if (lane == 0) *ntok = nt;
}

// ---- bits, codes, header ---------------------------------------------------------
using WebpBits = EncBits;  // the payload's bit writer (fi_enc_code.h)

struct WebpCodeWork {  // scratch of webp_write_code
  EncHuffWork huff;
  uint32_t freq[19];
  uint8_t lens[kWebpG];
  uint8_t cl_len[19];
  uint32_t cl_tab[19];
  uint32_t codes_work[34];
  uint16_t rle[kWebpG];  // code-length symbols: sym | extra << 8
};

// The prefix code of hist[0..n) (n <= 280): tab[s] = (len << 16) | reversed
// code, and the code as the stream carries it.  Up to two used symbols below
// 256: the simple form (one symbol: zero bits per occurrence); otherwise the
// normal form, lengths limited to 15, complete.
FI_ENC_HD void webp_write_code(const uint32_t *hist, int n, uint32_t *tab, WebpBits *bw, WebpCodeWork *ws) {
  constexpr uint8_t clord[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
  int used = 0, s0 = 0, s1 = 0;
  for (int s = 0; s < n; s++) {
    tab[s] = 0;
    if (hist[s]) {
      if (used == 0) s0 = s;
      if (used == 1) s1 = s;
      used++;
    }
  }
  if (used == 0) used = 1;  // (symbol 0, never read)
  if (used <= 2 && (used == 1 ? s0 : s1) < 256) {
    enc_put(bw, 1, 1);
    enc_put(bw, (uint32_t)(used - 1), 1);
    if (s0 < 2) {
      enc_put(bw, 0, 1);
      enc_put(bw, (uint32_t)s0, 1);
    } else {
      enc_put(bw, 1, 1);
      enc_put(bw, (uint32_t)s0, 8);
    }
    if (used == 2) {
      enc_put(bw, (uint32_t)s1, 8);
      tab[s0] = (1u << 16) | 0u;
      tab[s1] = (1u << 16) | 1u;
    }
    return;
  }
  enc_huff_lengths(hist, n, 15, ws->lens, &ws->huff);
  enc_huff_codes(ws->lens, n, 15, tab, ws->codes_work);
  if (used == 1) tab[s0] = 0;  // a decoder reads no bits for the only symbol
  // the lengths run-length coded, in a code of their own
  const int nr = enc_rle_lengths(ws->lens, n, ws->rle, ws->freq);
  const int ncl = enc_cl_code(ws->freq, clord, ws->cl_len, ws->cl_tab, &ws->huff, ws->codes_work);
  enc_put(bw, 0, 1);
  enc_put(bw, (uint32_t)(ncl - 4), 4);
  for (int i = 0; i < ncl; i++) enc_put(bw, ws->cl_len[clord[i]], 3);
  enc_put(bw, 0, 1);  // every symbol's length follows
  enc_put_rle(bw, ws->rle, nr, ws->cl_tab);
}

struct WebpBuildWork {  // scratch of webp_build_image (LDS on the device)
  WebpCodeWork code;
  uint32_t hist[kWebpHist];  // the mode image's green histogram / the fallback's histograms
  uint32_t mtab[kWebpG];     // the mode image's green code
  uint32_t zero[256];        // a histogram of nothing, and its table
  uint32_t ztab[256];
  int64_t coded_bits, fb_bits;
  int32_t coded_hdr, fb_hdr;
};

// Everything of the payload before the first token: the VP8L header, the
// transforms (the mode image with them) and the five codes, whose tables go
// to tabs[0..kWebpHist).  coded = false: the fallback form.
FI_ENC_HD void webp_write_head(const WebpImg &I, bool coded, const uint8_t *modes, const uint32_t *imghist,
                               uint32_t *tabs, WebpBits *bw, WebpBuildWork *ws) {
  enc_put(bw, 0x2F, 8);
  enc_put(bw, (uint32_t)(I.W - 1), 14);
  enc_put(bw, (uint32_t)(I.H - 1), 14);
  enc_put(bw, I.C == 2 || I.C == 4 ? 1u : 0u, 1);
  enc_put(bw, 0, 3);
  const uint32_t *h = imghist;
  if (coded) {
    enc_put(bw, 1, 1);
    enc_put(bw, 2, 2);  // subtract green
    enc_put(bw, 1, 1);
    enc_put(bw, 0, 2);  // predictor
    enc_put(bw, (uint32_t)(kWebpBlockBits - 2), 3);
    enc_put(bw, 0, 1);  // the mode image: no colour cache; the mode in green, zeros elsewhere
    const int64_t nblk = (int64_t)I.bw * I.bh;
    for (int s = 0; s < kWebpG; s++) ws->hist[s] = 0;
    for (int s = 0; s < 256; s++) ws->zero[s] = 0;
    for (int64_t i = 0; i < nblk; i++) ws->hist[modes[i]]++;
    webp_write_code(ws->hist, kWebpG, ws->mtab, bw, &ws->code);
    for (int k = 0; k < 3; k++) webp_write_code(ws->zero, 256, ws->ztab, bw, &ws->code);
    webp_write_code(ws->zero, kWebpD, ws->ztab, bw, &ws->code);
    for (int64_t i = 0; i < nblk; i++) enc_put(bw, ws->mtab[modes[i]] & 0xFFFFu, (int)(ws->mtab[modes[i]] >> 16));
    enc_put(bw, 0, 1);  // no further transform
  } else {
    if (I.C <= 2) {  // subtract green makes red and blue constant
      enc_put(bw, 1, 1);
      enc_put(bw, 2, 2);
    }
    enc_put(bw, 0, 1);
    for (int s = 0; s < kWebpHist; s++) ws->hist[s] = 0;
    for (int s = 0; s < 256; s++) {
      ws->hist[kWebpOffG + s] = 1;
      if (I.C >= 3) ws->hist[kWebpOffR + s] = ws->hist[kWebpOffB + s] = 1;
      if (I.C == 2 || I.C == 4) ws->hist[kWebpOffA + s] = 1;
    }
    if (I.C <= 2) ws->hist[kWebpOffR] = ws->hist[kWebpOffB] = 1;
    if (I.C == 1 || I.C == 3) ws->hist[kWebpOffA + 255] = 1;
    h = ws->hist;
  }
  enc_put(bw, 0, 1);  // no colour cache
  enc_put(bw, 0, 1);  // no meta prefix image: one Huffman group
  webp_write_code(h + kWebpOffG, kWebpG, tabs + kWebpOffG, bw, &ws->code);
  webp_write_code(h + kWebpOffR, 256, tabs + kWebpOffR, bw, &ws->code);
  webp_write_code(h + kWebpOffB, 256, tabs + kWebpOffB, bw, &ws->code);
  webp_write_code(h + kWebpOffA, 256, tabs + kWebpOffA, bw, &ws->code);
  webp_write_code(h + kWebpOffD, kWebpD, tabs + kWebpOffD, bw, &ws->code);
}

// the bits a token takes and, LSB first, their value: a literal is G, R, B, A
FI_ENC_HD int webp_token_bits(uint32_t tok, uint32_t argb, const uint32_t *tabs, uint64_t *val) {
  uint64_t v = 0;
  int nb = 0;
  if (tok & 0x80000000u) {
    int eb, ev;
    const int ls = enc_prefix_sym((int)(tok & 0xFFFu) + 1, &eb, &ev);
    uint32_t e = tabs[256 + ls];
    v = e & 0xFFFFu;
    nb = (int)(e >> 16);
    v |= (uint64_t)(uint32_t)ev << nb;
    nb += eb;
    const int ds = enc_prefix_sym((int)((tok >> 12) & 0x1FFFu) + 1 + 120, &eb, &ev);
    e = tabs[kWebpOffD + ds];
    v |= (uint64_t)(e & 0xFFFFu) << nb;
    nb += (int)(e >> 16);
    v |= (uint64_t)(uint32_t)ev << nb;
    nb += eb;
  } else {
    const uint32_t eg = tabs[kWebpOffG + ((argb >> 8) & 255u)], er = tabs[kWebpOffR + ((argb >> 16) & 255u)];
    const uint32_t eb = tabs[kWebpOffB + (argb & 255u)], ea = tabs[kWebpOffA + (argb >> 24)];
    v = eg & 0xFFFFu;
    nb = (int)(eg >> 16);
    v |= (uint64_t)(er & 0xFFFFu) << nb;
    nb += (int)(er >> 16);
    v |= (uint64_t)(eb & 0xFFFFu) << nb;
    nb += (int)(eb >> 16);
    v |= (uint64_t)(ea & 0xFFFFu) << nb;
    nb += (int)(ea >> 16);
  }
  *val = v;
  return nb;
}

// The image's codes, header and form.  imghist: its five histograms; bandhists:
// kWebpHist words per band; bandoff[b]: payload bit where band b starts (out).
// slot: the zeroed output slot; lane 0 writes RIFF header and payload head.
// Prices the coded and the fallback form and takes the smaller.  The coded
// head is built once, straight into the slot (the fallback's head has
// I.fb_hdr bits whatever the image holds); only where the fallback wins is it
// wiped and the fallback's written in its place.
FI_ENC_HD void webp_build_image(const WebpImg &I, const uint32_t *imghist, const uint8_t *modes,
                                const uint32_t *bandhists, int lane, int nlanes, WebpBuildWork *ws, uint32_t *tabs,
                                int64_t *bandoff, uint32_t *slot, WebpImgOut *out, int32_t *fault) {
  uint32_t *pay = slot + kWebpRiffBytes / 4;
  const int64_t cap = (I.slot_bytes - kWebpRiffBytes) * 8;
  if (lane == 0) {
    ws->fb_hdr = I.fb_hdr;
    ws->fb_bits = I.fb_hdr + (int64_t)I.npix * 8 * I.C;
    WebpBits bw{pay, 0, cap, 0};
    webp_write_head(I, true, modes, imghist, tabs, &bw, ws);  // (past the slot it only counts: the fallback is smaller then)
    ws->coded_hdr = (int32_t)bw.pos;
  }
  FI_WEBP_SYNC();
  for (int b = lane; b < I.nbands; b += nlanes) {
    const uint32_t *hb = bandhists + (int64_t)b * kWebpHist;
    int64_t bits = 0;
    for (int s = 0; s < kWebpHist; s++) {
      const int extra = s >= 256 && s < kWebpG ? enc_prefix_extra(s - 256) : s >= kWebpOffD ? enc_prefix_extra(s - kWebpOffD) : 0;
      bits += (int64_t)hb[s] * ((tabs[s] >> 16) + (uint32_t)extra);
    }
    bandoff[b] = bits;
  }
  FI_WEBP_SYNC();
  if (lane == 0) {
    int64_t acc = ws->coded_hdr;
    for (int b = 0; b < I.nbands; b++) {
      const int64_t t = bandoff[b];
      bandoff[b] = acc;
      acc += t;
    }
    ws->coded_bits = acc;
    const bool fb = ws->fb_bits < ws->coded_bits;
    const int64_t total = fb ? ws->fb_bits : ws->coded_bits;
    const int64_t payload = (total + 7) >> 3, file = kWebpRiffBytes + payload + (payload & 1);
    int64_t hdr = ws->coded_hdr;
    if (fb) {
      for (int b = 0; b < I.nbands; b++) bandoff[b] = ws->fb_hdr + (int64_t)b * kWebpBand * 8 * I.C;
      const int64_t used = ws->coded_hdr < cap ? ws->coded_hdr : cap;
      for (int64_t w = 0; w < (used + 31) >> 5; w++) pay[w] = 0;
      WebpBits bw{pay, 0, cap, 0};
      webp_write_head(I, false, modes, imghist, tabs, &bw, ws);
      if (bw.over || bw.pos != ws->fb_hdr) *fault = 1;
      hdr = bw.pos;
    }
    if (file > I.slot_bytes) *fault = 1;
    slot[0] = 0x46464952u;  // "RIFF"
    slot[1] = (uint32_t)(file - 8);
    slot[2] = 0x50424557u;  // "WEBP"
    slot[3] = 0x4C385056u;  // "VP8L"
    slot[4] = (uint32_t)payload;
    out->fallback = fb ? 1 : 0;
    out->hdr_bits = (int32_t)hdr;
    out->total_bits = total;
    out->file_bytes = file;
  }
  FI_WEBP_SYNC();
}

}  // namespace fi
