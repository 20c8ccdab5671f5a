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

// Progressive files with per-scan optimal tables (fi_jpeg_pwrite.cpp; the
// entropy coder itself is fi_jpeg_pcore.h, shared with the kernels), as
// libjpeg-turbo writes them for progressive=True, restart_marker_rows=1.
// SOI, APP0, DQT, SOF2: everything before the first scan's tables
void jpeg_penc_write_head(int w, int h, int channels, int quality, int subsampling, std::vector<uint8_t> *out);
// what follows scan s's DHT segments: DRI where the scan's interval differs
// from *last_interval (updated), then SOS
void jpeg_penc_write_scan_tail(int w, int h, int channels, int subsampling, int s, int *last_interval,
                               std::vector<uint8_t> *out);
// upper bound of the whole progressive file; 0 = OK (the statuses of jpeg_enc_check)
int jpeg_penc_bound(int w, int h, int channels, int quality, int subsampling, size_t *bytes);
// The host model: the file of the quantised coefficients `coefs` (zigzag int16
// blocks, a plane per component padded to whole MCUs: what
// fi_debug_jpeg_coefs_host hands out; ncoefs of them).  *flushes = the
// correction-buffer flushes inside EOB runs.  0, a status of jpeg_enc_check,
// or FI_EINVAL for a coefficient count that does not fit the geometry.
int jpeg_penc_write(const int16_t *coefs, size_t ncoefs, int w, int h, int channels, int quality, int subsampling,
                    std::vector<uint8_t> *out, int *flushes);

}  // namespace fi
