// fi_jpeg_enc.h -- host side of the GPU JPEG encoder (fi_jpeg_write.cpp): the
// quantisation tables, the standard Huffman tables, the file header and the
// size bound.  Plain host C++ (no HIP header), so the writer builds and runs
// under ASan/UBSan on its own (tests/native/jpeg_write_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace fi {

// worst-case entropy-coded bytes of one 8x8 block before 0xFF stuffing: a DC
// symbol (code <= 11 bits + 11 value bits) and 63 AC symbols of the longest
// code with the largest value (16 + 10 bits) = 22 + 63 * 26 = 1660 bits
constexpr int kJpegEncBlockBytes = 208;

// jpeg_quality_scaling + jpeg_add_quant_table (force_baseline) of the Annex K
// tables: t[0] luminance, t[1] chrominance, natural order
void jpeg_enc_quant_tables(int quality, uint16_t t[2][64]);
// the four Annex K Huffman tables (jstdhuff.c) as jchuff.c's derived encoding
// tables: tab[256 * (2 * chroma + ac) + symbol] = (code length << 16) | code
void jpeg_enc_huff_tables(uint32_t tab[1024]);
// 0, or FI_EINVAL / FI_EUNSUPPORTED as fi_jpeg_encode_device documents them
int jpeg_enc_check(int w, int h, int channels, int quality, int subsampling);
// blocks per MCU (1 gray, 3 4:4:4, 6 4:2:0) and the MCU grid
void jpeg_enc_grid(int w, int h, int channels, int subsampling, int *bpm, int *mcux, int *mcuy);
// SOI ... SOS as libjpeg-turbo writes them for these settings (one restart
// interval per MCU row), appended to `out`
void jpeg_enc_write_header(int w, int h, int channels, int quality, int subsampling, std::vector<uint8_t> *out);
// worst-case bytes of one restart interval (stuffed, with its RSTn)
size_t jpeg_enc_slot_bytes(int bpm, int mcux);
// upper bound of the whole file; 0 = OK
int jpeg_enc_bound(int w, int h, int channels, int quality, int subsampling, size_t *bytes);

}  // namespace fi
