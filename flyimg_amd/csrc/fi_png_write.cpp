// fi_png_write.cpp -- host side of the GPU PNG encoder (fi_png_enc.hip): the
// argument check, the size bound and the file's fixed chunks (signature + IHDR,
// IEND).  Host C++ only.
#include "fi_png_enc.h"

#include "../../include/flyimg_hip.h"

namespace fi {

// Eight bytes per step (slicing by 8): the decoder's chunk walk checks the CRC
// of every IDAT byte of a batch on one host thread.
struct CrcTables {
  uint32_t t[8][256];
  CrcTables() {
    for (uint32_t i = 0; i < 256; i++) t[0][i] = png_crc_byte(i);
    for (int k = 1; k < 8; k++)
      for (uint32_t i = 0; i < 256; i++) t[k][i] = t[0][t[k - 1][i] & 255u] ^ (t[k - 1][i] >> 8);
  }
};

uint32_t png_crc32(uint32_t crc, const uint8_t *p, size_t n) {
  static const CrcTables T;
  uint32_t c = ~crc;
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    const uint32_t lo = c ^ ((uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) |
                             ((uint32_t)p[i + 3] << 24));
    c = T.t[7][lo & 255u] ^ T.t[6][(lo >> 8) & 255u] ^ T.t[5][(lo >> 16) & 255u] ^ T.t[4][lo >> 24] ^
        T.t[3][p[i + 4]] ^ T.t[2][p[i + 5]] ^ T.t[1][p[i + 6]] ^ T.t[0][p[i + 7]];
  }
  for (; i < n; i++) c = T.t[0][(c ^ p[i]) & 255u] ^ (c >> 8);
  return ~c;
}

int png_enc_check(int w, int h, int channels, int filter) {
  if (channels < 1 || channels > 4 || w < 1 || h < 1 || w > 65535 || h > 65535 || filter < -1 || filter > 4)
    return FI_EINVAL;
  if (png_enc_stream_bytes(w, h, channels) > 0x7FFFFFFFll) return FI_EUNSUPPORTED;
  return 0;
}

int64_t png_enc_stream_bytes(int w, int h, int channels) { return (int64_t)h * ((int64_t)w * channels + 1); }

// Signature and IHDR, the zlib header and the Adler-32, IEND, and per band of
// the filtered stream one IDAT chunk (length, type, CRC) around the band as
// stored blocks: the encoder writes a band that way whenever its dynamic block
// (with the alignment block behind it) would not be smaller.
int png_enc_bound(int w, int h, int channels, size_t *bytes) {
  const int rc = png_enc_check(w, h, channels, -1);
  if (rc) return rc;
  const int64_t s = png_enc_stream_bytes(w, h, channels);
  const int64_t full = s / kPngBand, rest = s % kPngBand;
  int64_t b = kPngHdrBytes + 12 + 2 + 4;
  b += full * (12 + png_stored_bytes(kPngBand));
  if (rest) b += 12 + png_stored_bytes((int)rest);
  *bytes = (size_t)b;
  return 0;
}

static void be32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

void png_enc_write_header(int w, int h, int channels, uint8_t out[kPngHdrBytes]) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  static const uint8_t ctype[5] = {0, 0, 4, 2, 6};  // gray, gray + alpha, RGB, RGBA
  for (int i = 0; i < 8; i++) out[i] = sig[i];
  be32(out + 8, 13);
  out[12] = 'I';
  out[13] = 'H';
  out[14] = 'D';
  out[15] = 'R';
  be32(out + 16, (uint32_t)w);
  be32(out + 20, (uint32_t)h);
  out[24] = 8;  // bit depth
  out[25] = ctype[channels];
  out[26] = 0;  // deflate
  out[27] = 0;  // adaptive filtering
  out[28] = 0;  // no interlace
  be32(out + 29, png_crc32(0, out + 12, 17));
}

void png_enc_write_iend(uint8_t out[12]) {
  be32(out, 0);
  out[4] = 'I';
  out[5] = 'E';
  out[6] = 'N';
  out[7] = 'D';
  be32(out + 8, png_crc32(0, out + 4, 4));
}

}  // namespace fi
