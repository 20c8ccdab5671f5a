// fi_jpeg_pwrite.cpp -- host model and writer of the progressive GPU JPEG
// encoder (fi_jpeg_penc.hip): the file libjpeg-turbo produces for Pillow's
// Image.save(..., "JPEG", quality=q, subsampling=s, progressive=True,
// restart_marker_rows=1), from quantised coefficients.  The entropy coder, the
// table builder and the scan script are fi_jpeg_pcore.h, which the kernels
// compile too; here are the file layout, the size bound and the model that
// runs the coder serially.  Host C++ only.
#include <assert.h>

#include "fi_jpeg_enc.h"
#include "fi_jpeg_pcore.h"

#include "../../include/flyimg_hip.h"

namespace fi {

namespace {
struct CountSink {  // the statistics pass (jcphuff.c with gather_statistics)
  uint32_t *cnt;    // [2][kPencHist]
  void sym(int t, int s) { cnt[kPencHist * t + s]++; }
  void bits(uint32_t, int) {}
};
}  // namespace

void jpeg_penc_write_head(int w, int h, int channels, int quality, int subsampling, std::vector<uint8_t> *o) {
  // the baseline header up to its frame header, which becomes SOF2
  std::vector<uint8_t> b;
  jpeg_enc_write_header(w, h, channels, quality, subsampling, &b);
  const int nc = channels == 3 ? 3 : 1;
  const size_t sof = 20 + 69 * (size_t)(nc == 3 ? 2 : 1);
  b[sof + 1] = 0xC2;
  o->insert(o->end(), b.begin(), b.begin() + sof + 10 + 3 * nc);
}

void jpeg_penc_write_scan_tail(int w, int h, int channels, int subsampling, int s, int *last_interval,
                               std::vector<uint8_t> *o) {
  PencGeom G;
  penc_geom(w, h, channels, subsampling, &G);
  const PencScan S = penc_scan(G.nc, s);
  const int iv = penc_scan_interval(G, S);
  if (iv != *last_interval) {  // jcmarker.c write_scan_header
    const uint8_t dri[6] = {0xFF, 0xDD, 0, 4, (uint8_t)(iv >> 8), (uint8_t)(iv & 255)};
    o->insert(o->end(), dri, dri + 6);
    *last_interval = iv;
  }
  const int n = S.ss == 0 ? G.nc : 1;
  o->push_back(0xFF);
  o->push_back(0xDA);
  o->push_back(0);
  o->push_back((uint8_t)(6 + 2 * n));
  o->push_back((uint8_t)n);
  for (int i = 0; i < n; i++) {
    const int c = S.ss == 0 ? i : S.comp;
    const int td = S.ss == 0 && S.ah == 0 && c ? 1 : 0, ta = S.se && c ? 1 : 0;
    o->push_back((uint8_t)(c + 1));
    o->push_back((uint8_t)((td << 4) | ta));
  }
  o->push_back(S.ss);
  o->push_back(S.se);
  o->push_back((uint8_t)((S.ah << 4) | S.al));
}

// The file: the head (SOI 2, APP0 18, DQT 69 each, SOF2 10 + 3 nc), per scan
// its DHT segments (kPencDhtMax each), DRI 6, SOS 8 + 2 components, and one
// slot of penc_slot_bytes per block row (the last row's RSTn pays for nothing;
// EOI is added).  Nothing is fitted to samples.
int jpeg_penc_bound(int w, int h, int channels, int quality, int subsampling, size_t *bytes) {
  const int rc = jpeg_enc_check(w, h, channels, quality, subsampling);
  if (rc) return rc;
  PencGeom G;
  penc_geom(w, h, channels, subsampling, &G);
  size_t t = 20 + 69 * (size_t)(G.nc == 3 ? 2 : 1) + 10 + 3 * G.nc + 2;
  for (int s = 0; s < penc_nscans(G.nc); s++) {
    const PencScan S = penc_scan(G.nc, s);
    int tc[2];
    t += (size_t)penc_scan_tables(S, tc) * kPencDhtMax + 6 + 8 + 2 * (S.ss == 0 ? G.nc : 1);
    t += (size_t)penc_scan_rows(G, S) * penc_slot_bytes(S, penc_scan_blocks(G, S));
  }
  *bytes = t;
  return 0;
}

int jpeg_penc_write(const int16_t *coefs, size_t ncoefs, int w, int h, int channels, int quality, int subsampling,
                    std::vector<uint8_t> *out, int *flushes) {
  const int rc = jpeg_enc_check(w, h, channels, quality, subsampling);
  if (rc) return rc;
  PencGeom G;
  penc_geom(w, h, channels, subsampling, &G);
  PencLayout L{};
  L.base = coefs;
  L.planar = 1;
  L.bpm = G.bpm;
  L.mcux = G.mcux;
  size_t total = 0;
  for (int c = 0; c < G.nc; c++) {
    const int hs = c == 0 && G.bpm == 6 ? 2 : 1;
    L.plane[c] = (int64_t)total;
    L.pw[c] = G.mcux * hs;
    total += (size_t)G.mcux * hs * G.mcuy * hs * 64;
  }
  if (!coefs || ncoefs != total) return FI_EINVAL;
  *flushes = 0;
  jpeg_penc_write_head(w, h, channels, quality, subsampling, out);
  int last_interval = 0;
  std::vector<uint8_t> slot;
  for (int s = 0; s < penc_nscans(G.nc); s++) {
    const PencScan S = penc_scan(G.nc, s);
    const int rows = penc_scan_rows(G, S), nblk = penc_scan_blocks(G, S);
    assert(nblk < 0x7FFF);  // an EOB run cannot reach jcphuff.c's cap within one block row
    // statistics, as the scan will be coded: every interval flushes its run
    uint32_t cnt[2 * kPencHist] = {0};
    CountSink cs{cnt};
    for (int r = 0; r < rows; r++) (void)penc_interval(G, S, L, r, cs);
    uint32_t code[2 * 256] = {0};
    int tc[2];
    const int nt = penc_scan_tables(S, tc);
    for (int t = 0; t < nt; t++) {
      uint8_t bits[17], vals[256], dht[kPencDhtMax];
      const int nv = penc_gen_table(cnt + kPencHist * t, bits, vals, code + 256 * t);
      const int len = penc_write_dht(dht, tc[t], bits, vals, nv);
      out->insert(out->end(), dht, dht + len);
    }
    jpeg_penc_write_scan_tail(w, h, channels, subsampling, s, &last_interval, out);
    slot.resize(penc_slot_bytes(S, nblk));
    for (int r = 0; r < rows; r++) {
      PencByteSink bs;
      bs.init(slot.data(), (int64_t)slot.size() - 2, code);
      *flushes += penc_interval(G, S, L, r, bs);
      bs.finish();
      if (bs.n > bs.cap) return FI_EINVAL;  // (the bound holds by construction)
      out->insert(out->end(), slot.data(), slot.data() + bs.n);
      if (r != rows - 1) {
        out->push_back(0xFF);
        out->push_back((uint8_t)(0xD0 + (r & 7)));
      }
    }
  }
  out->push_back(0xFF);
  out->push_back(0xD9);
  return 0;
}

}  // namespace fi
