// fi_jpeg_write.cpp -- host side of the GPU JPEG encoder (fi_jpeg_enc.hip):
// the tables, the header bytes and the size bound, as libjpeg-turbo produces
// them for Pillow's Image.save(..., "JPEG", quality=q, subsampling=s,
// restart_marker_rows=1).  Host C++ only.
#include "fi_jpeg_enc.h"

#include "../../include/flyimg_hip.h"

namespace fi {

namespace {
// Annex K.1 / K.2, natural order
const uint8_t kBaseLum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                              14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                              18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                              99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3 (jstdhuff.c): code counts per length 1..16, then the symbols
const uint8_t kBitsDcLum[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kBitsDcChr[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kValDc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kBitsAcLum[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kValAcLum[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kBitsAcChr[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kValAcChr[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct HuffSpec {
  const uint8_t *bits, *vals;
  int nvals;
};
// slot 2 * chroma + ac
const HuffSpec kHuff[4] = {{kBitsDcLum, kValDc, 12},
                           {kBitsAcLum, kValAcLum, 162},
                           {kBitsDcChr, kValDc, 12},
                           {kBitsAcChr, kValAcChr, 162}};

void put16(std::vector<uint8_t> *o, int v) {
  o->push_back((uint8_t)(v >> 8));
  o->push_back((uint8_t)(v & 255));
}
void put_dht(std::vector<uint8_t> *o, int slot) {
  const HuffSpec &s = kHuff[slot];
  o->push_back(0xFF);
  o->push_back(0xC4);
  put16(o, 2 + 1 + 16 + s.nvals);
  o->push_back((uint8_t)(((slot & 1) << 4) | (slot >> 1)));  // Tc (0 DC, 1 AC) | Th
  o->insert(o->end(), s.bits, s.bits + 16);
  o->insert(o->end(), s.vals, s.vals + s.nvals);
}
// header bytes: SOI 2, APP0 18, DQT 69 each, SOF0 10 + 3 nc, DHT 33 / 183
// (luminance) + 33 / 183 (chrominance), DRI 6, SOS 8 + 2 nc
size_t header_bytes(int nc) { return nc == 1 ? 2 + 18 + 69 + 13 + 216 + 6 + 10 : 2 + 18 + 138 + 19 + 432 + 6 + 14; }
}  // namespace

void jpeg_enc_quant_tables(int quality, uint16_t t[2][64]) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int k = 0; k < 64; k++) {
    const int base[2] = {kBaseLum[k], kBaseChr[k]};
    for (int c = 0; c < 2; c++) {
      int v = (base[c] * scale + 50) / 100;
      t[c][k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
  }
}

void jpeg_enc_huff_tables(uint32_t tab[1024]) {
  for (int i = 0; i < 1024; i++) tab[i] = 0;
  for (int slot = 0; slot < 4; slot++) {
    const HuffSpec &s = kHuff[slot];
    uint32_t code = 0;
    int p = 0;
    for (int l = 1; l <= 16; l++) {  // jpeg_make_c_derived_tbl: canonical codes in order of length
      for (int i = 0; i < s.bits[l - 1] && p < s.nvals; i++) tab[256 * slot + s.vals[p++]] = ((uint32_t)l << 16) | code++;
      code <<= 1;
    }
  }
}

int jpeg_enc_check(int w, int h, int channels, int quality, int subsampling) {
  if (channels != 1 && channels != 3) return channels == 2 || channels == 4 ? FI_EUNSUPPORTED : FI_EINVAL;
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || quality < 1 || quality > 100) return FI_EINVAL;
  if (channels == 3 && subsampling != 0 && subsampling != 2) return FI_EUNSUPPORTED;
  return 0;
}

void jpeg_enc_grid(int w, int h, int channels, int subsampling, int *bpm, int *mcux, int *mcuy) {
  const int m = channels == 3 && subsampling == 2 ? 16 : 8;
  *bpm = channels == 1 ? 1 : m == 16 ? 6 : 3;
  *mcux = (w + m - 1) / m;
  *mcuy = (h + m - 1) / m;
}

void jpeg_enc_write_header(int w, int h, int channels, int quality, int subsampling, std::vector<uint8_t> *o) {
  const int nc = channels == 3 ? 3 : 1;
  int bpm, mcux, mcuy;
  jpeg_enc_grid(w, h, channels, subsampling, &bpm, &mcux, &mcuy);
  uint16_t qt[2][64];
  jpeg_enc_quant_tables(quality, qt);
  static const uint8_t soi_app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  o->insert(o->end(), soi_app0, soi_app0 + 20);
  for (int t = 0; t < (nc == 3 ? 2 : 1); t++) {
    o->push_back(0xFF);
    o->push_back(0xDB);
    put16(o, 67);
    o->push_back((uint8_t)t);
    for (int z = 0; z < 64; z++) o->push_back((uint8_t)qt[t][kZigzag[z]]);
  }
  o->push_back(0xFF);
  o->push_back(0xC0);
  put16(o, 8 + 3 * nc);
  o->push_back(8);
  put16(o, h);
  put16(o, w);
  o->push_back((uint8_t)nc);
  for (int c = 0; c < nc; c++) {
    o->push_back((uint8_t)(c + 1));
    o->push_back((uint8_t)(c == 0 && bpm == 6 ? 0x22 : 0x11));
    o->push_back((uint8_t)(c ? 1 : 0));
  }
  for (int slot = 0; slot < (nc == 3 ? 4 : 2); slot++) put_dht(o, slot);  // DC0, AC0, DC1, AC1
  o->push_back(0xFF);
  o->push_back(0xDD);
  put16(o, 4);
  put16(o, mcux);  // one restart interval per MCU row
  o->push_back(0xFF);
  o->push_back(0xDA);
  put16(o, 6 + 2 * nc);
  o->push_back((uint8_t)nc);
  for (int c = 0; c < nc; c++) {
    o->push_back((uint8_t)(c + 1));
    o->push_back((uint8_t)(c ? 0x11 : 0x00));
  }
  o->push_back(0);
  o->push_back(63);
  o->push_back(0);
}

// One restart interval holds bpm * mcux blocks.  A block codes into at most
// 1660 bits (kJpegEncBlockBytes: a DC code of <= 11 bits with 11 value bits,
// 63 AC symbols of 16 + 10 bits; no ZRL or EOB can add to a block whose 63 AC
// coefficients are all coded), so the interval's bits, padded to a whole byte,
// fit blocks * 208 bytes (207.5 per block, and the padding is < 1 byte).  Every
// one of those bytes may be 0xFF and gain a stuffed zero byte: * 2.  The RSTn
// marker after the interval adds 2.
size_t jpeg_enc_slot_bytes(int bpm, int mcux) { return (size_t)bpm * mcux * kJpegEncBlockBytes * 2 + 2; }

// The file: the header (fixed for a component count: header_bytes), mcuy
// restart intervals of at most jpeg_enc_slot_bytes each (the last carries no
// RSTn: its 2 bytes pay for EOI).  Nothing here is fitted to samples; typical
// files are tens of times smaller.
int jpeg_enc_bound(int w, int h, int channels, int quality, int subsampling, size_t *bytes) {
  const int rc = jpeg_enc_check(w, h, channels, quality, subsampling);
  if (rc) return rc;
  int bpm, mcux, mcuy;
  jpeg_enc_grid(w, h, channels, subsampling, &bpm, &mcux, &mcuy);
  *bytes = header_bytes(channels == 3 ? 3 : 1) + (size_t)mcuy * jpeg_enc_slot_bytes(bpm, mcux);
  return 0;
}

}  // namespace fi
