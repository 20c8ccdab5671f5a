// fi_png_enc.h -- what the GPU PNG encoder's device half (fi_png_enc.hip) and
// host half (fi_png_write.cpp) share: the band geometry, the size bound, the
// file's fixed chunks, and -- as plain inline functions that compile for the
// host and the device alike -- deflate's length symbols and the per-band block
// construction: the dynamic block header around the codes, run-length coder
// and bit writer of fi_enc_code.h, and the choice between stored, fixed and
// dynamic codes.  (The checksums are fi_png_sum.h's.)  No HIP header is
// needed: the host half and this header build and run under ASan/UBSan on
// their own (tests/native/png_write_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fi_enc_code.h"
#include "fi_png_sum.h"

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

// bytes a band of n filtered bytes takes as stored blocks
FI_ENC_HD int png_stored_bytes(int n) { return n + 5 * ((n + 65534) / 65535); }

// ---- deflate symbols ---------------------------------------------------------
// length 3..258 -> lit/len symbol 257..285, its extra bits and their value
FI_ENC_HD int png_len_sym(int len, int *ebits, int *eval) {
  const int l = len - 3;
  if (l < 8 || len == 258) {
    *ebits = 0;
    *eval = 0;
    return len == 258 ? 285 : 257 + l;
  }
  const int e = enc_ilog2((uint32_t)l) - 2;
  *ebits = e;
  *eval = l & ((1 << e) - 1);
  return 261 + 4 * e + ((l - (4 << e)) >> e);
}
FI_ENC_HD int png_len_extra(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }

// ---- code construction -----------------------------------------------------------
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
  EncHuffWork huff;
  uint32_t freq[kPngLL];
  uint8_t lens[kPngLL + kPngD];  // lit/len lengths, then distance lengths
  uint8_t cl_len[19];
  uint32_t cl_tab[19];
  uint32_t codes_work[34];  // enc_huff_codes
  uint16_t rle[kPngLL + kPngD];  // code-length symbols: sym | extra << 8
  int32_t nrle;
};

// The dynamic codes and header of a band with lit/len codes of at most llmax
// bits (the used symbols must number at most 2^llmax): fills out->ll, dist,
// hdr, hdr_bits; returns the bits of the whole block.
FI_ENC_HD int64_t png_build_dynamic(const uint32_t *hist, int llmax, PngBandCode *out, PngCodeWork *ws) {
  constexpr uint8_t clord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint8_t *ll_len = ws->lens, *d_len = ws->lens + kPngLL;
  for (int s = 0; s < kPngLL; s++) ws->freq[s] = s < 286 ? hist[s] : 0;
  ws->freq[256] = 1;
  enc_huff_lengths(ws->freq, 286, llmax, ll_len, &ws->huff);
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
  enc_huff_lengths(ws->freq, 30, 15, d_len, &ws->huff);
  enc_huff_codes(ll_len, 286, 15, out->ll, ws->codes_work);
  enc_huff_codes(d_len, 30, 15, out->dist, ws->codes_work);
  int hlit = 286, hdist = 30;
  while (hlit > 257 && !ll_len[hlit - 1]) hlit--;
  while (hdist > 1 && !d_len[hdist - 1]) hdist--;
  // the lengths as one sequence, run-length coded with 16 / 17 / 18
  for (int s = 0; s < hdist; s++) ws->lens[hlit + s] = d_len[s];  // (hlit <= kPngLL: moves down or stays)
  const int nr = enc_rle_lengths(ws->lens, hlit + hdist, ws->rle, ws->freq);
  ws->nrle = nr;
  const int hclen = enc_cl_code(ws->freq, clord, ws->cl_len, ws->cl_tab, &ws->huff, ws->codes_work);
  // header bits, LSB first
  for (int i = 0; i < kPngHdrWords; i++) out->hdr[i] = 0;
  EncBits bw{out->hdr, 0, kPngHdrWords * 32, 0};  // (kPngHdrWords holds the longest header there is)
  enc_put(&bw, (uint32_t)(hlit - 257), 5);
  enc_put(&bw, (uint32_t)(hdist - 1), 5);
  enc_put(&bw, (uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; i++) enc_put(&bw, ws->cl_len[clord[i]], 3);
  enc_put_rle(&bw, ws->rle, nr, ws->cl_tab);
  const int pos = (int)bw.pos;
  out->hdr_bits = pos;
  if (bw.over) return (int64_t)1 << 40;  // not a block: the caller takes the fixed codes or stored blocks
  int64_t bits = 3 + pos + (out->ll[256] >> 16);
  for (int s = 0; s < 286; s++)
    if (s != 256) bits += (int64_t)hist[s] * ((out->ll[s] >> 16) + (uint32_t)png_len_extra(s));
  for (int s = 0; s < 30; s++) bits += (int64_t)hist[kPngLL + s] * ((out->dist[s] >> 16) + (uint32_t)enc_prefix_extra(s));
  return bits;
}

// The block of a band from its histograms hist[0..kPngHist) (lit/len at 0,
// distances at kPngLL; the end-of-block symbol is counted here).  Fills *out
// and decides between stored, fixed and dynamic codes, whichever is smallest:
// n = the band's bytes, last = it ends the stream (no alignment block after
// it).  In a band of a few hundred bytes the header is a tenth of the block
// and every distinct code length costs there, so short bands also try codes
// limited to 10, 9, 8 and 7 bits and keep the smallest block.
FI_ENC_HD void png_build_block(const uint32_t *hist, int n, bool last, PngBandCode *out, PngCodeWork *ws) {
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
  for (int s = 0; s < 30; s++) fbits += (int64_t)hist[kPngLL + s] * (5 + enc_prefix_extra(s));
  if (fbits < bits) {
    for (int s = 0; s < kPngLL; s++) ws->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < kPngD; s++) ws->lens[kPngLL + s] = 5;
    enc_huff_codes(ws->lens, kPngLL, 15, out->ll, ws->codes_work);
    enc_huff_codes(ws->lens + kPngLL, kPngD, 15, out->dist, ws->codes_work);
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
