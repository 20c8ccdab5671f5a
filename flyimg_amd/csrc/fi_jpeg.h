// fi_jpeg.h -- host side of the GPU JPEG decoder (fi_jpeg_parse.cpp): the
// header summary the batch planner in fi_jpeg.hip works from.  Host C++ only,
// so the parser can be built and fuzzed under ASan/UBSan on its own
// (tests/native/jpeg_fuzz_driver.cpp, tests/native/jpeg_prog_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "fi_internal.h"

namespace fi {

constexpr int kJpegMaxScans = 64;

struct JpegScan {  // one SOS of a progressive stream
  int ns = 0, ci[3] = {}, td[3] = {}, ta[3] = {};
  int Ss = 0, Se = 0, Ah = 0, Al = 0;
  int tab[3] = {-1, -1, -1};  // JpegHdr::ptab index in force at this SOS: the DC table of each
                              // component (DC first scan) or tab[0] = the AC table; -1: none needed
  int restart = 0;            // DRI in force (MCUs of this scan)
  int level = 0;              // 1 + the highest level of the earlier scans it overlaps, else 0
  size_t ecs0 = 0, ecs1 = 0;  // its entropy-coded segment [ecs0, ecs1)
};

struct JpegHdr {
  int W = 0, H = 0, ncomp = 0, restart = 0;
  int id[3] = {}, h[3] = {}, v[3] = {}, tq[3] = {}, td[3] = {}, ta[3] = {};
  uint16_t qt[4][64] = {};  // natural order
  bool qt_ok[4] = {};
  std::string dht[4];       // DC0, DC1, AC0, AC1: bits[16] + huffval
  size_t ecs0 = 0, ecs1 = 0;  // entropy-coded segment [ecs0, ecs1); progressive: first SOS data .. EOI
  // progressive (SOF2) streams, FI_JPEG_PROGRESSIVE only
  bool progressive = false;
  std::vector<JpegScan> scans;
  std::vector<std::string> ptab;  // every table a scan uses: 'D' / 'A' + bits[16] + huffval
  int nlevels = 0;
};

struct JpegGeom {  // block grids of a parsed stream
  int hmax, vmax, mcux, mcuy;
  int bw[3], bh[3];  // component block grid (whole MCUs)
  int dw[3], dh[3];  // downsampled width / height (jdmaster.c)
};

// 0 = OK; FI_EUNSUPPORTED for streams the GPU decoder does not handle;
// FI_EINVAL for malformed data
int jpeg_parse(const uint8_t *d, size_t n, JpegHdr *o, uint32_t flags = 0);
// jdhuff.c jpeg_make_d_derived_tbl (+ the fast-AC entries); false when the
// code lengths are over-subscribed, the value count does not match, or (dc) a
// DC symbol exceeds 15 -- the tables libjpeg rejects with JERR_BAD_HUFF_TABLE
bool jpeg_build_huff(const std::string &dht, bool dc, JpegHuff *t);
// dimensions and output channels of a stream the GPU decoder takes
int jpeg_info(const uint8_t *data, size_t len, int *w, int *h, int *c);
int jpeg_info_ex(const uint8_t *data, size_t len, uint32_t flags, int *w, int *h, int *c, int *nscans, int *nlevels);
// EXIF orientation of a JPEG as Pillow's Image.getexif().get(0x0112, 1) reads
// it, from the marker segments up to the first SOS (whether or not the GPU
// decoder takes the stream): FI_OK with *orientation in 1..8 (values
// exif_transpose ignores are 1); FI_EUNSUPPORTED where Pillow's answer takes
// more than an IFD0 lookup (several Exif segments, XMP, odd types, malformed
// TIFF): the host decides; FI_EINVAL without SOI
int jpeg_orientation(const uint8_t *d, size_t n, int *orientation);
void jpeg_geom(const JpegHdr &H, JpegGeom *G);
// The work items of a progressive stream: per scan, one per restart interval
// (located by the RSTn markers of the scan's segment).  tabmap[i] = the batch
// table index of H.ptab[i]; byte offsets are relative to H.ecs0.
void jpeg_prog_items(const JpegHdr &H, const JpegGeom &G, const uint8_t *data, int img, const int *tabmap,
                     std::vector<JpegProgItem> *out);
// Host entropy decode of a progressive stream (fi_jpeg_prog_host.cpp): the
// block procedures of fi_jpeg_prog.h -- the ones k_jpeg_prog runs -- on the
// CPU.  coefs: the int16 zigzag blocks of component 0, 1, 2 one after the
// other, [bh][bw][64] each.
int jpeg_prog_coefs_host(const uint8_t *data, size_t len, uint32_t flags, JpegHdr *H, JpegGeom *G,
                         std::vector<int16_t> *coefs);

}  // namespace fi
