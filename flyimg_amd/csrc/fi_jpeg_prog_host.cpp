// fi_jpeg_prog_host.cpp -- progressive JPEG entropy decode on the CPU: the
// parser, the scan scheduler and the block procedures of fi_jpeg_prog.h that
// k_jpeg_prog runs on the device, over a plain byte reader.  Host C++ only
// (tests/native/jpeg_prog_driver.cpp runs it under ASan/UBSan; the
// fi_debug_jpeg_coefs_host export lets a test compare its coefficients,
// through an IDCT, with libjpeg's pixels).
#include <string.h>

#include <algorithm>

#include "fi_jpeg.h"
#include "fi_jpeg_prog.h"

namespace fi {

namespace {

// jdhuff.c jpeg_fill_bit_buffer over [pos, end): stuffed 0xFF00 -> 0xFF; a
// marker or the end of the scan feeds zero bits, counted in `fake` as
// fi_jpeg.hip's BitReader counts them
struct HostBitReader {
  const uint8_t *p;
  int pos, end;
  uint64_t buf;
  int nbits, fake;
  bool marker;
  bool short_of_data() const { return nbits < fake; }
  void init(const uint8_t *seg, int byte0, int end_) {
    p = seg;
    pos = byte0;
    end = end_;
    buf = 0;
    nbits = 0;
    fake = 0;
    marker = false;
  }
  void fill() {
    while (nbits < 32) {
      uint32_t b = 0;
      if (!marker && pos < end) {
        b = p[pos];
        if (b == 0xFFu) {
          if (pos + 1 < end && p[pos + 1] == 0u) {
            pos += 2;
          } else {
            marker = true;
            b = 0;
            fake += 8;
          }
        } else {
          pos++;
        }
      } else {
        fake += 8;
      }
      buf = (buf << 8) | b;
      nbits += 8;
    }
  }
  uint32_t peek(int n) const { return (uint32_t)(buf >> (nbits - n)) & ((1u << n) - 1u); }
  void skip(int n) { nbits -= n; }
};

struct HostOps {  // jpeg_decode_sym of fi_jpeg.hip
  static int sym(HostBitReader &br, const JpegHuff *t) {
    br.fill();
    const uint32_t lk = t->look[br.peek(9)];
    if (lk) {
      br.skip(lk >> 8);
      return lk & 255;
    }
    int l = 10;
    int32_t code = (int32_t)br.peek(10);
    while (l <= 16 && code > t->maxcode[l]) {
      l++;
      code = (int32_t)br.peek(l);
    }
    if (l > 16) {  // corrupt data: jdhuff.c warns and returns 0, the 17 bits it tried consumed
      br.skip(17);
      return 0;
    }
    br.skip(l);
    return t->huffval[(code + t->valoff[l]) & 255];
  }
  static uint64_t deposit(uint64_t bits, int n, uint64_t m) {
    uint64_t o = 0;
    for (int i = n - 1; m; m &= m - 1, i--)
      if ((bits >> i) & 1) o |= m & (~m + 1);
    return o;
  }
};

}  // namespace

int jpeg_prog_coefs_host(const uint8_t *data, size_t len, uint32_t flags, JpegHdr *H, JpegGeom *G,
                         std::vector<int16_t> *coefs) {
  const int rc = jpeg_parse(data, len, H, flags);
  if (rc) return rc;
  if (!H->progressive) return FI_EUNSUPPORTED;
  std::vector<JpegHuff> huffs(H->ptab.size());
  std::vector<int> tabmap(H->ptab.size());
  for (size_t t = 0; t < H->ptab.size(); t++) {
    if (!jpeg_build_huff(H->ptab[t].substr(1), H->ptab[t][0] == 'D', &huffs[t])) return FI_EINVAL;
    tabmap[t] = (int)t;
  }
  jpeg_geom(*H, G);
  size_t co[3], total = 0;
  for (int c = 0; c < 3; c++) {
    co[c] = total;
    total += (size_t)G->bw[c] * G->bh[c] * 64;
  }
  coefs->assign(total, 0);
  std::vector<JpegProgItem> items;
  jpeg_prog_items(*H, *G, data, 0, tabmap.data(), &items);
  std::stable_sort(items.begin(), items.end(),
                   [](const JpegProgItem &a, const JpegProgItem &b) { return a.level < b.level; });
  // the segment, at its exact size (the reader is bounded by each scan's end)
  const std::vector<uint8_t> seg(data + H->ecs0, data + H->ecs1);
  for (const JpegProgItem &I : items) {
    HostBitReader br;
    br.init(seg.data(), I.byte0, I.end);
    JpegProgState S{};
    const JpegHuff *tab[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; k++)
      if (I.tab[k] >= 0) tab[k] = &huffs[I.tab[k]];
    // (jdphuff.c insufficient_data: the MCU it was raised in is finished, the later ones are left alone)
    for (int mcu = I.mcu0; mcu < I.mcu1 && !br.short_of_data(); mcu++) {
      if (I.Ss != 0 && I.Ah == 0 && S.eobrun > 0) {  // a first-pass run leaves its blocks zero
        const uint32_t skip = std::min<uint32_t>(S.eobrun, (uint32_t)(I.mcu1 - mcu));
        S.eobrun -= skip;
        mcu += (int)skip - 1;
        continue;
      }
      for (int k = 0; k < I.ns; k++) {
        const int c = I.ci[k];
        const int hs = I.ns == 1 ? 1 : H->h[c], vs = I.ns == 1 ? 1 : H->v[c];
        for (int by = 0; by < vs; by++)
          for (int bx = 0; bx < hs; bx++) {
            int16_t *b = coefs->data() + co[c] + jpeg_prog_block(I, mcu, hs, vs, by, bx, G->bw[c]) * 64;
            if (I.Ss == 0) {
              if (I.Ah == 0)
                jpeg_prog_dc_first<HostOps>(br, tab[k], b, S.pred[k], I.Al);
              else if (jpeg_prog_dc_refine(br))
                b[0] = (int16_t)(b[0] | (1 << I.Al));
            } else if (I.Ah == 0) {
              if (!jpeg_prog_ac_first<HostOps>(br, tab[0], b, S.eobrun, I.Ss, I.Se, I.Al)) return FI_EUNSUPPORTED;
            } else {
              JpegProgRefine R{};
              for (int z = I.Ss; z <= I.Se; z++) {
                R.nz |= (uint64_t)(b[z] != 0) << z;
                R.has |= (uint64_t)((b[z] & (1 << I.Al)) != 0) << z;
              }
              if (!jpeg_prog_ac_refine<HostOps>(br, tab[0], R, S.eobrun, I.Ss, I.Se)) return FI_EUNSUPPORTED;
              for (int z = I.Ss; z <= I.Se; z++) b[z] = jpeg_prog_refined(b[z], z, R, I.Al);
            }
          }
      }
    }
  }
  return 0;
}

}  // namespace fi
