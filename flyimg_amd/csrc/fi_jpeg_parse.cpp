// fi_jpeg_parse.cpp -- the GPU JPEG decoder's host-side header parser and
// Huffman table builder (restating libjpeg-turbo jdmarker.c / jdhuff.c for
// the streams fi_jpeg.hip decodes).  Host C++ only: no HIP calls.
#include <string.h>

#include "fi_jpeg.h"

namespace fi {

static int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

// ---- progressive streams (SOF2): the scan list ----------------------------
struct ProgParse {
  std::vector<std::string> defs;  // every DHT definition so far, 'D' / 'A' + bits + huffval
  std::vector<int> def_ix;        // its JpegHdr::ptab index once a scan uses it
  int cur[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};  // [class][id] -> defs index in force
  bool high_id = false;           // a table id 2 or 3 was defined (progressive only)
  int coef_bits[3][64];           // jdphuff.c coef_bits: last Al sent per coefficient, -1 = never
  ProgParse() {
    for (auto &c : coef_bits)
      for (int &b : c) b = -1;
  }
};

// end of an entropy-coded segment: the first marker other than RSTn (stuffed
// 0xFF00 and fill bytes skipped), or n
static size_t scan_end(const uint8_t *d, size_t n, size_t q) {
  while (q < n) {
    const void *f = memchr(d + q, 0xFF, n - q);
    if (!f) return n;
    q = (size_t)((const uint8_t *)f - d);
    if (q + 1 >= n) return n;
    const int b = d[q + 1];
    if (b == 0x00 || b == 0xFF || (b >= 0xD0 && b <= 0xD7)) {
      q += b == 0xFF ? 1 : 2;
      continue;
    }
    return q;
  }
  return n;
}

// The restart markers of a scan of nmcu MCUs, segment e[0, len): libjpeg reads
// one after every `restart` MCUs and expects them numbered 0, 1, ... mod 8
// (jdmarker.c read_restart_marker); for a skipped, repeated or missing one
// jpeg_resync_to_restart drops or invents intervals.  Only the regular
// sequence is decoded here (the intervals are located by their markers); the
// markers after the last MCU are never read.
static bool restarts_regular(const uint8_t *e, size_t len, int restart, int nmcu) {
  if (restart <= 0) return true;
  const int need = (nmcu + restart - 1) / restart - 1;
  int seen = 0;
  for (size_t q = 0; q + 1 < len && seen < need; q++) {
    if (e[q] == 0xFF && e[q + 1] >= 0xD0 && e[q + 1] <= 0xD7) {
      if (e[q + 1] - 0xD0 != (seen & 7)) return false;
      seen++;
      q++;
    }
  }
  return seen == need;
}

// One SOS of a progressive stream (s .. e = the marker's payload of length L - 2):
// jdmarker.c get_sos and jdphuff.c start_pass_phuff_decoder
static int prog_sos(const uint8_t *d, size_t n, const uint8_t *s, size_t L, const uint8_t *e, bool jfif, bool adobe,
                    int adobe_transform, JpegHdr *o, ProgParse *pp) {
  if (o->scans.empty()) {
    // colour space and sampling: the rules of the baseline path
    if (o->ncomp == 3 && !jfif) {
      if (adobe && adobe_transform == 0) return FI_EUNSUPPORTED;
      if (!adobe && o->id[0] == 82 && o->id[1] == 71 && o->id[2] == 66) return FI_EUNSUPPORTED;
    }
    for (int c = 0; c < o->ncomp; c++)
      if (!o->qt_ok[o->tq[c]]) return FI_EINVAL;
    if (o->ncomp == 1) {
      o->h[0] = o->v[0] = 1;
    } else {
      if (o->h[1] != 1 || o->v[1] != 1 || o->h[2] != 1 || o->v[2] != 1) return FI_EUNSUPPORTED;
      const int hv = o->h[0] * 10 + o->v[0];
      if (hv != 11 && hv != 21 && hv != 22) return FI_EUNSUPPORTED;
    }
    o->ecs0 = (size_t)(e - d);
  }
  if ((int)o->scans.size() >= kJpegMaxScans) return FI_EUNSUPPORTED;
  JpegScan S;
  S.ns = s[0];
  if (S.ns < 1 || S.ns > 4 || L != 6 + 2 * (size_t)S.ns) return FI_EINVAL;
  if (S.ns > o->ncomp) return FI_EINVAL;
  for (int k = 0; k < S.ns; k++) {
    const int cs = s[1 + 2 * k];
    int c = -1;
    for (int j = 0; j < o->ncomp; j++)
      if (o->id[j] == cs) c = j;
    if (c < 0) return FI_EINVAL;
    for (int j = 0; j < k; j++)
      if (S.ci[j] == c) return FI_EINVAL;
    // (libjpeg takes the components of a scan in any order; the MCU layout
    // follows the scan's order: leave other orders to the host)
    if (k > 0 && c < S.ci[k - 1]) return FI_EUNSUPPORTED;
    S.ci[k] = c;
    S.td[k] = s[2 + 2 * k] >> 4;
    S.ta[k] = s[2 + 2 * k] & 15;
    if (S.td[k] > 3 || S.ta[k] > 3) return FI_EINVAL;
  }
  const uint8_t *t = s + 1 + 2 * S.ns;
  S.Ss = t[0];
  S.Se = t[1];
  S.Ah = t[2] >> 4;
  S.Al = t[2] & 15;
  // JERR_BAD_PROGRESSION
  if (S.Ss > S.Se || S.Se > 63) return FI_EINVAL;
  if (S.Ss == 0 && S.Se != 0) return FI_EINVAL;
  if (S.Ss != 0 && S.ns != 1) return FI_EINVAL;
  if (S.Ah != 0 && S.Al != S.Ah - 1) return FI_EINVAL;
  if (S.Al > 13) return FI_EINVAL;
  // coef_bits: where libjpeg warns (JWRN_BOGUS_PROGRESSION) the host decodes;
  // so it does for a coefficient sent twice from scratch
  for (int k = 0; k < S.ns; k++) {
    int *cb = pp->coef_bits[S.ci[k]];
    if (S.Ss != 0 && cb[0] < 0) return FI_EUNSUPPORTED;  // AC before DC
    for (int z = S.Ss; z <= S.Se; z++) {
      if (S.Ah != (cb[z] < 0 ? 0 : cb[z]) || (S.Ah == 0 && cb[z] >= 0)) return FI_EUNSUPPORTED;
      cb[z] = S.Al;
    }
  }
  // the tables in force (JERR_NO_HUFF_TABLE)
  auto use = [&](int tc, int th) {
    const int di = pp->cur[tc][th];
    if (di < 0) return -1;
    if (pp->def_ix[di] < 0) {
      pp->def_ix[di] = (int)o->ptab.size();
      o->ptab.push_back(pp->defs[di]);
    }
    return pp->def_ix[di];
  };
  if (S.Ss == 0) {
    if (S.Ah == 0)
      for (int k = 0; k < S.ns; k++)
        if ((S.tab[k] = use(0, S.td[k])) < 0) return FI_EINVAL;
  } else if ((S.tab[0] = use(1, S.ta[0])) < 0) {
    return FI_EINVAL;
  }
  S.restart = o->restart;
  S.ecs0 = (size_t)(e - d);
  S.ecs1 = scan_end(d, n, S.ecs0);
  // level: 1 + the highest level of an earlier scan that shares a component
  // over an overlapping band
  for (const JpegScan &P : o->scans) {
    if (P.Ss > S.Se || S.Ss > P.Se) continue;
    bool share = false;
    for (int a = 0; a < S.ns; a++)
      for (int b = 0; b < P.ns; b++) share |= S.ci[a] == P.ci[b];
    if (share && P.level + 1 > S.level) S.level = P.level + 1;
  }
  o->scans.push_back(S);
  return 0;
}

// at EOI: every coefficient of every component sent and refined to Al = 0
// (libjpeg smooths the blocks of an incomplete file: jdcoefct.c)
static int prog_finish(const uint8_t *d, JpegHdr *o, const ProgParse &pp) {
  for (int c = 0; c < o->ncomp; c++)
    for (int z = 0; z < 64; z++)
      if (pp.coef_bits[c][z] != 0) return FI_EUNSUPPORTED;
  JpegGeom G;
  jpeg_geom(*o, &G);
  for (const JpegScan &S : o->scans) {  // (the MCU counts of jpeg_prog_items)
    const int c = S.ci[0];
    const int nmcu = S.ns == 1 ? ((G.dw[c] + 7) / 8) * ((G.dh[c] + 7) / 8) : G.mcux * G.mcuy;
    if (!restarts_regular(d + S.ecs0, S.ecs1 - S.ecs0, S.restart, nmcu)) return FI_EUNSUPPORTED;
  }
  o->nlevels = 0;
  for (const JpegScan &S : o->scans) o->nlevels = S.level + 1 > o->nlevels ? S.level + 1 : o->nlevels;
  o->ecs1 = o->scans.back().ecs1;
  if (o->ecs1 - o->ecs0 > 0x7FFFF000u) return FI_EUNSUPPORTED;  // 32-bit offsets on the device
  return 0;
}

// 0 = OK; FI_EUNSUPPORTED for streams the GPU decoder does not handle;
// FI_EINVAL for malformed data
int jpeg_parse(const uint8_t *d, size_t n, JpegHdr *o, uint32_t flags) {
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return FI_EINVAL;
  const bool prog_ok = (flags & FI_JPEG_PROGRESSIVE) != 0;
  ProgParse pp;
  static const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  size_t p = 2;
  bool sof = false;
  // jdmarker.c examine_app0 / examine_app14: what default_decompress_parms
  // (jdapimin.c) reads to pick the colour space of a 3-component stream
  bool jfif = false, adobe = false;
  int adobe_transform = 0;
  while (p + 4 <= n) {
    if (d[p] != 0xFF) return FI_EINVAL;
    const int m = d[p + 1];
    if (m == 0xFF) {  // fill byte
      p++;
      continue;
    }
    if (o->progressive && !o->scans.empty() && (m == 0xD9 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01))
      return FI_EUNSUPPORTED;  // data after EOI, or a stray marker between the scans
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) {
      p += 2;
      continue;
    }
    const size_t L = (size_t)be16(d + p + 2);
    // (a progressive stream cut off between its scans: truncated, as one cut off inside a scan)
    if (L >= 2 && p + 2 + L > n && o->progressive && !o->scans.empty()) return FI_EUNSUPPORTED;
    if (L < 2 || p + 2 + L > n) return FI_EINVAL;
    const uint8_t *s = d + p + 4, *e = d + p + 2 + L;
    switch (m) {
      case 0xC2:  // progressive, Huffman (FI_JPEG_PROGRESSIVE)
        if (!prog_ok) return FI_EUNSUPPORTED;
        [[fallthrough]];
      case 0xC0:
      case 0xC1: {  // baseline / extended sequential, Huffman
        if (sof || L < 8 || s[0] != 8) return FI_EUNSUPPORTED;
        sof = true;
        o->progressive = m == 0xC2;
        o->H = be16(s + 1);
        o->W = be16(s + 3);
        o->ncomp = s[5];
        if (o->W <= 0 || o->H <= 0) return FI_EUNSUPPORTED;  // DNL-defined height
        if (o->ncomp != 1 && o->ncomp != 3) return FI_EUNSUPPORTED;
        if (L != 8 + 3 * (size_t)o->ncomp) return FI_EINVAL;
        for (int c = 0; c < o->ncomp; c++) {
          o->id[c] = s[6 + 3 * c];
          o->h[c] = s[7 + 3 * c] >> 4;
          o->v[c] = s[7 + 3 * c] & 15;
          o->tq[c] = s[8 + 3 * c];
          if (o->tq[c] > 3 || o->h[c] < 1 || o->v[c] < 1) return FI_EINVAL;
        }
        break;
      }
      case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB:
      case 0xCD: case 0xCE: case 0xCF:
        return FI_EUNSUPPORTED;  // progressive, lossless, hierarchical, arithmetic
      case 0xDB: {  // DQT
        if (!o->scans.empty()) return FI_EUNSUPPORTED;  // redefined between scans (libjpeg latches per component)
        for (const uint8_t *q = s; q < e;) {
          const int pq = q[0] >> 4, tq = q[0] & 15;
          if (tq > 3 || pq > 1 || q + 1 + 64 * (pq + 1) > e) return FI_EINVAL;
          for (int k = 0; k < 64; k++)
            o->qt[tq][zz[k]] = (uint16_t)(pq ? be16(q + 1 + 2 * k) : q[1 + k]);
          o->qt_ok[tq] = true;
          q += 1 + 64 * (pq + 1);
        }
        break;
      }
      case 0xC4: {  // DHT
        for (const uint8_t *q = s; q < e;) {
          if (q + 17 > e) return FI_EINVAL;
          const int tc = q[0] >> 4, th = q[0] & 15;
          if (tc > 1 || th > (prog_ok ? 3 : 1)) return FI_EUNSUPPORTED;  // baseline: two tables per class
          int cnt = 0;
          for (int l = 0; l < 16; l++) cnt += q[1 + l];
          if (cnt > 256 || q + 17 + cnt > e) return FI_EINVAL;
          if (th > 1)
            pp.high_id = true;
          else
            o->dht[2 * tc + th].assign((const char *)q + 1, 16 + cnt);
          if (prog_ok) {  // progressive: the table in force at each SOS
            pp.cur[tc][th] = (int)pp.defs.size();
            pp.defs.push_back(std::string(1, tc ? 'A' : 'D') + std::string((const char *)q + 1, 16 + cnt));
            pp.def_ix.push_back(-1);
          }
          q += 17 + cnt;
        }
        break;
      }
      case 0xDD:  // DRI
        if (L != 4) return FI_EINVAL;
        o->restart = be16(s);
        break;
      case 0xDA: {  // SOS: the one scan, then the entropy-coded data up to EOI
        if (!sof || L < 3) return FI_EINVAL;
        if (o->progressive) {
          const int rc = prog_sos(d, n, s, L, e, jfif, adobe, adobe_transform, o, &pp);
          if (rc) return rc;
          p = o->scans.back().ecs1;
          continue;
        }
        if (pp.high_id) return FI_EUNSUPPORTED;  // baseline: two tables per class
        const int ns = s[0];
        if (ns != o->ncomp || L != 6 + 2 * (size_t)ns) return FI_EUNSUPPORTED;  // one interleaved scan
        for (int k = 0; k < ns; k++) {
          const int cs = s[1 + 2 * k];
          if (cs != o->id[k]) return FI_EUNSUPPORTED;
          o->td[k] = s[2 + 2 * k] >> 4;
          o->ta[k] = s[2 + 2 * k] & 15;
          if (o->td[k] > 1 || o->ta[k] > 1) return FI_EUNSUPPORTED;
        }
        const uint8_t *t = s + 1 + 2 * ns;
        if (t[0] != 0 || t[1] != 63 || t[2] != 0) return FI_EUNSUPPORTED;
        o->ecs0 = (size_t)(e - d);
        // end of the scan: the first marker other than RSTn (stuffed 0xFF00 and fill bytes skipped)
        size_t q = o->ecs0;
        for (;;) {
          const void *f = memchr(d + q, 0xFF, n - q);
          if (!f) {
            q = n;
            break;
          }
          q = (size_t)((const uint8_t *)f - d);
          if (q + 1 >= n) {
            q = n;
            break;
          }
          const int b = d[q + 1];
          if (b == 0x00 || b == 0xFF || (b >= 0xD0 && b <= 0xD7)) {
            q += b == 0xFF ? 1 : 2;
            continue;
          }
          break;
        }
        o->ecs1 = q;
        // the scan must end at EOI: a truncated stream (no marker before the
        // end of the data) or one with markers after the scan goes to the host
        // decoder, which reports truncation as libjpeg / Pillow do
        if (q + 1 >= n || d[q + 1] != 0xD9) return FI_EUNSUPPORTED;
        // libjpeg decodes a 3-component stream as RGB (no colour conversion) when
        // it has no JFIF marker and either an Adobe marker with transform 0 or,
        // with no Adobe marker, the component ids 'R', 'G', 'B'; the GPU path
        // converts YCbCr only
        if (o->ncomp == 3 && !jfif) {
          if (adobe && adobe_transform == 0) return FI_EUNSUPPORTED;
          if (!adobe && o->id[0] == 82 && o->id[1] == 71 && o->id[2] == 66) return FI_EUNSUPPORTED;
        }
        for (int c = 0; c < o->ncomp; c++) {
          if (!o->qt_ok[o->tq[c]] || o->dht[o->td[c]].empty() || o->dht[2 + o->ta[c]].empty()) return FI_EINVAL;
        }
        if (o->ncomp == 1) {
          o->h[0] = o->v[0] = 1;  // non-interleaved scan: one block per MCU
        } else {
          // YCbCr with luma 1x1 / 2x1 / 2x2 over 1x1 chroma (jdsample.c fullsize / h2v1 / h2v2)
          if (o->h[1] != 1 || o->v[1] != 1 || o->h[2] != 1 || o->v[2] != 1) return FI_EUNSUPPORTED;
          const int hv = o->h[0] * 10 + o->v[0];
          if (hv != 11 && hv != 21 && hv != 22) return FI_EUNSUPPORTED;
        }
        JpegGeom G;
        jpeg_geom(*o, &G);
        if (!restarts_regular(d + o->ecs0, o->ecs1 - o->ecs0, o->restart, G.mcux * G.mcuy)) return FI_EUNSUPPORTED;
        return 0;
      }
      case 0xE0:  // APP0 "JFIF\0" (examine_app0: at least 14 data bytes)
        if (L >= 16 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
        break;
      case 0xEE:  // APP14 "Adobe" (examine_app14: at least 12 data bytes); it may precede SOF
        if (L >= 14 && memcmp(s, "Adobe", 5) == 0) {
          adobe = true;
          adobe_transform = s[11];
        }
        break;
      default:
        break;  // APPn, COM, ...
    }
    p += 2 + L;
  }
  if (o->progressive && !o->scans.empty()) {
    // the last scan must end at EOI, the last two bytes of the data
    if (p + 2 != n || d[p] != 0xFF || d[p + 1] != 0xD9) return FI_EUNSUPPORTED;
    return prog_finish(d, o, pp);
  }
  return FI_EINVAL;
}

// jdhuff.c jpeg_make_d_derived_tbl: canonical codes, maxcode / valoffset,
// 9-bit lookahead
bool jpeg_build_huff(const std::string &dht, bool dc, JpegHuff *t) {
  memset(t, 0, sizeof(*t));
  if (dht.size() < 16 || dht.size() > 16 + 256) return false;
  const uint8_t *bits = (const uint8_t *)dht.data();
  const int nv = (int)dht.size() - 16;
  int cnt = 0;
  for (int l = 0; l < 16; l++) cnt += bits[l];
  if (cnt != nv) return false;
  memcpy(t->huffval, bits + 16, nv);
  // jdhuff.c: DC symbols are coefficient sizes, 0..15 (JERR_BAD_HUFF_TABLE)
  if (dc)
    for (int k = 0; k < nv; k++)
      if (t->huffval[k] > 15) return false;
  int p = 0;
  uint32_t code = 0;
  for (int l = 1; l <= 16; l++) {
    // jdhuff.c: the codes of length l, and the next code after them, must fit
    // in l bits (no code is all ones); checked before any lookahead entry is
    // written, so an over-subscribed table never writes past look[]
    if ((uint64_t)code + bits[l - 1] >= ((uint64_t)1 << l)) return false;
    if (bits[l - 1]) {
      t->valoff[l] = p - (int)code;
      for (int i = 0; i < bits[l - 1]; i++, p++, code++) {
        if (l <= 9) {
          const uint32_t lo = code << (9 - l), cnt = 1u << (9 - l);
          for (uint32_t k = 0; k < cnt; k++) t->look[lo + k] = (uint16_t)((l << 8) | t->huffval[p]);
        }
      }
      t->maxcode[l] = (int32_t)code - 1;
    } else {
      t->maxcode[l] = -1;
    }
    code <<= 1;
  }
  t->maxcode[17] = 0x7FFFFFFF;
  // fast AC entries (as stb_image's fast_ac): run/size symbols whose code and
  // value bits both fit the 9-bit lookahead and whose value fits a signed byte
  for (int l = 0; l < 512; l++) {
    const int lk = t->look[l];
    if (!lk) continue;
    const int len = lk >> 8, rs = lk & 255, run = rs >> 4, sz = rs & 15;
    if (sz == 0 || len + sz > 9) continue;
    const int v = (l >> (9 - len - sz)) & ((1 << sz) - 1);
    const int val = v < (1 << (sz - 1)) ? v - (1 << sz) + 1 : v;  // HUFF_EXTEND
    if (val < -128 || val > 127) continue;
    t->fast_ac[l] = (int16_t)((val * 256) | (run << 4) | (len + sz));
  }
  return p == nv;
}


int jpeg_info_ex(const uint8_t *data, size_t len, uint32_t flags, int *w, int *h, int *c, int *nscans, int *nlevels) {
  JpegHdr hd;
  const int rc = jpeg_parse(data, len, &hd, flags);
  if (rc) return rc;
  JpegHuff hf;
  if (hd.progressive) {  // (the tables its scans use)
    for (const std::string &t : hd.ptab)
      if (!jpeg_build_huff(t.substr(1), t[0] == 'D', &hf)) return FI_EINVAL;
  } else {
    for (int t = 0; t < 4; t++)  // the Huffman tables must build (jdhuff.c rejects bad ones too)
      if (!hd.dht[t].empty() && !jpeg_build_huff(hd.dht[t], t < 2, &hf)) return FI_EINVAL;
  }
  *w = hd.W;
  *h = hd.H;
  *c = hd.ncomp == 1 ? 1 : 3;
  if (nscans) *nscans = hd.progressive ? (int)hd.scans.size() : 1;
  if (nlevels) *nlevels = hd.progressive ? hd.nlevels : 1;
  return 0;
}
int jpeg_info(const uint8_t *data, size_t len, int *w, int *h, int *c) {
  return jpeg_info_ex(data, len, 0, w, h, c, nullptr, nullptr);
}

// ---- EXIF orientation ------------------------------------------------------
// Tag 0x0112 of IFD0 of one TIFF structure (the payload of an Exif APP1 after
// its "Exif\0\0"): 0 = absent, 1..8 / other = its SHORT value (*val), -1 = the
// host decides (malformed, another type or count, the tag twice)
static int exif_ifd0_orientation(const uint8_t *t, size_t n, int *val) {
  if (n < 8) return -1;
  bool le;
  if (t[0] == 'I' && t[1] == 'I' && t[2] == 0x2A && t[3] == 0)
    le = true;
  else if (t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 0x2A)
    le = false;
  else
    return -1;
  auto u16 = [&](const uint8_t *p) -> uint32_t { return le ? p[0] | (p[1] << 8) : (p[0] << 8) | p[1]; };
  auto u32 = [&](const uint8_t *p) -> uint32_t { return le ? u16(p) | (u16(p + 2) << 16) : (u16(p) << 16) | u16(p + 2); };
  const size_t off = u32(t + 4);
  if (off > n || n - off < 2) return -1;
  const size_t cnt = u16(t + off);
  if ((n - off - 2) / 12 < cnt) return -1;
  int found = 0;
  for (size_t k = 0; k < cnt; k++) {
    const uint8_t *e = t + off + 2 + 12 * k;
    if (u16(e) != 0x0112) continue;
    if (found++ || u16(e + 2) != 3 || u32(e + 4) != 1) return -1;
    *val = (int)u16(e + 8);
  }
  return found;
}

// The orientation Pillow's Image.getexif().get(0x0112, 1) yields (markers up to
// the first SOS: JpegImagePlugin.APP collects them, Image.getexif reads IFD0
// and falls back to tiff:Orientation of an XMP packet), or FI_EUNSUPPORTED
// wherever that takes more than an IFD0 lookup -- never another orientation.
int jpeg_orientation(const uint8_t *d, size_t n, int *orientation) {
  if (!d || !orientation || n < 2 || d[0] != 0xFF || d[1] != 0xD8) return FI_EINVAL;
  static const char kExif[] = "Exif\0\0", kXmp[] = "http://ns.adobe.com/xap/1.0/";  // (+ its NUL: 29 bytes)
  int nexif = 0, found = 0, val = 1;
  bool xmp = false;
  size_t p = 2;
  for (;;) {
    if (p + 2 > n || d[p] != 0xFF) return FI_EUNSUPPORTED;  // no SOS, or bytes between the segments
    const int m = d[p + 1];
    if (m == 0xFF) {  // fill byte
      p++;
      continue;
    }
    if (m == 0xDA) break;
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) {
      p += 2;
      continue;
    }
    if (m == 0xD9 || m == 0x00 || p + 4 > n) return FI_EUNSUPPORTED;
    const size_t L = (size_t)be16(d + p + 2);
    if (L < 2 || L > n - p - 2) return FI_EUNSUPPORTED;  // the segment runs past the data
    const uint8_t *s = d + p + 4;
    const size_t sl = L - 2;
    if (m == 0xE1 && sl >= 6 && memcmp(s, kExif, 6) == 0) {
      if (++nexif > 1) return FI_EUNSUPPORTED;  // Pillow concatenates them
      found = exif_ifd0_orientation(s + 6, sl - 6, &val);
      if (found < 0) return FI_EUNSUPPORTED;
    } else if (m == 0xE1 && sl >= 29 && memcmp(s, kXmp, 29) == 0) {
      xmp = true;
    }
    p += 2 + L;
  }
  if (!found && xmp) return FI_EUNSUPPORTED;  // tiff:Orientation of the XMP packet applies
  *orientation = found && val >= 2 && val <= 8 ? val : 1;  // (exif_transpose does nothing for 0, 1, 9..)
  return FI_OK;
}

void jpeg_geom(const JpegHdr &H, JpegGeom *G) {
  G->hmax = G->vmax = 1;
  for (int c = 0; c < H.ncomp; c++) {
    G->hmax = H.h[c] > G->hmax ? H.h[c] : G->hmax;
    G->vmax = H.v[c] > G->vmax ? H.v[c] : G->vmax;
  }
  G->mcux = (H.W + 8 * G->hmax - 1) / (8 * G->hmax);
  G->mcuy = (H.H + 8 * G->vmax - 1) / (8 * G->vmax);
  for (int c = 0; c < 3; c++) {
    const bool on = c < H.ncomp;
    G->bw[c] = on ? G->mcux * H.h[c] : 0;
    G->bh[c] = on ? G->mcuy * H.v[c] : 0;
    G->dw[c] = on ? (H.W * H.h[c] + G->hmax - 1) / G->hmax : 0;  // jdmaster.c downsampled_width
    G->dh[c] = on ? (H.H * H.v[c] + G->vmax - 1) / G->vmax : 0;
  }
}

// jdinput.c per_scan_setup: a single-component scan's MCU is one block of the
// component's own raster, ceil(dw / 8) x ceil(dh / 8); an interleaved scan
// walks the image's MCU grid
void jpeg_prog_items(const JpegHdr &H, const JpegGeom &G, const uint8_t *data, int img, const int *tabmap,
                     std::vector<JpegProgItem> *out) {
  for (const JpegScan &S : H.scans) {
    JpegProgItem I{};
    I.img = img;
    I.level = S.level;
    I.ns = S.ns;
    for (int k = 0; k < 3; k++) {
      I.ci[k] = k < S.ns ? S.ci[k] : 0;
      I.tab[k] = S.tab[k] >= 0 ? tabmap[S.tab[k]] : -1;
    }
    I.Ss = S.Ss;
    I.Se = S.Se;
    I.Ah = S.Ah;
    I.Al = S.Al;
    int nmcu;
    if (S.ns == 1) {
      const int c = S.ci[0];
      I.mcux = (G.dw[c] + 7) / 8;
      nmcu = I.mcux * ((G.dh[c] + 7) / 8);
    } else {
      I.mcux = G.mcux;
      nmcu = G.mcux * G.mcuy;
    }
    const int b0 = (int)(S.ecs0 - H.ecs0), b1 = (int)(S.ecs1 - H.ecs0);
    I.end = b1;
    int byte0 = b0, mcu0 = 0;
    if (S.restart > 0) {  // RSTn markers split the scan's segment
      const uint8_t *e = data + H.ecs0;
      for (int q = b0; q + 1 < b1 && mcu0 < nmcu; q++) {
        if (e[q] == 0xFF && e[q + 1] >= 0xD0 && e[q + 1] <= 0xD7) {
          I.mcu0 = mcu0;
          I.mcu1 = mcu0 + S.restart < nmcu ? mcu0 + S.restart : nmcu;
          I.byte0 = byte0;
          out->push_back(I);
          mcu0 += S.restart;
          byte0 = q + 2;
          q++;
        }
      }
    }
    if (mcu0 < nmcu) {
      I.mcu0 = mcu0;
      I.mcu1 = nmcu;
      I.byte0 = byte0;
      out->push_back(I);
    }
  }
}

}  // namespace fi
