// fi_jpeg_pcore.h -- the progressive JPEG entropy coder both halves of the
// encoder run: the host model (fi_jpeg_pwrite.cpp) and the device kernels
// (fi_jpeg_penc.hip) compile these same functions, so the model is the
// kernels' byte-level specification.  libjpeg-turbo's jcphuff.c (the four block
// procedures, EOB runs, the correction-bit buffer), jchuff.c
// jpeg_gen_optimal_table and the scan script of jpeg_simple_progression, for
// files written with one restart interval per block row of every scan.
// No HIP header: FI_PHD is empty for a host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FI_PHD __host__ __device__ inline
#else
#define FI_PHD inline
#endif

namespace fi {

constexpr int kPencMaxScans = 10;
constexpr int kPencTabs = 2 * kPencMaxScans;  // table slots of an image: 2 * scan + (0 | 1)
constexpr int kPencHist = 257;                // symbol counts of a table (the 257th is libjpeg's reserved one)
constexpr int kPencDhtMax = 2 + 2 + 1 + 16 + 256;
// jcphuff.c: MAX_CORR_BITS - DCTSIZE2 + 1; more buffered correction bits than this end the EOB run
constexpr int kPencCorrFlush = 1000 - 64 + 1;

struct PencScan {
  uint8_t ncomp, comp, ss, se, ah, al;  // ncomp 3: interleaved (comp unused)
};

FI_PHD int penc_nscans(int nc) { return nc == 3 ? 10 : 6; }
FI_PHD PencScan penc_scan(int nc, int s) {
  // jcparam.c jpeg_simple_progression
  constexpr PencScan ycc[10] = {{3, 0, 0, 0, 0, 1},  {1, 0, 1, 5, 0, 2},  {1, 2, 1, 63, 0, 1}, {1, 1, 1, 63, 0, 1},
                                {1, 0, 6, 63, 0, 2}, {1, 0, 1, 63, 2, 1}, {3, 0, 0, 0, 1, 0},  {1, 2, 1, 63, 1, 0},
                                {1, 1, 1, 63, 1, 0}, {1, 0, 1, 63, 1, 0}};
  constexpr PencScan gray[6] = {{1, 0, 0, 0, 0, 1},  {1, 0, 1, 5, 0, 2}, {1, 0, 6, 63, 0, 2},
                                {1, 0, 1, 63, 2, 1}, {1, 0, 0, 0, 1, 0}, {1, 0, 1, 63, 1, 0}};
  return nc == 3 ? ycc[s] : gray[s];
}

// Geometry of an image's scans.  bpm as the baseline encoder has it (1 gray,
// 3 4:4:4, 6 4:2:0); wb / hb: the components' own block grids.
struct PencGeom {
  int32_t nc, bpm, mcux, mcuy;
  int32_t wb[3], hb[3];
};
FI_PHD void penc_geom(int w, int h, int channels, int subsampling, PencGeom *G) {
  const bool s420 = channels == 3 && subsampling == 2;
  const int m = s420 ? 16 : 8;
  G->nc = channels == 3 ? 3 : 1;
  G->bpm = channels != 3 ? 1 : s420 ? 6 : 3;
  G->mcux = (w + m - 1) / m;
  G->mcuy = (h + m - 1) / m;
  for (int c = 0; c < 3; c++) {
    const int wc = c && s420 ? (w + 1) / 2 : w, hc = c && s420 ? (h + 1) / 2 : h;
    G->wb[c] = (wc + 7) / 8;
    G->hb[c] = (hc + 7) / 8;
  }
}
// restart intervals (block rows) of a scan, and the blocks of one of them
FI_PHD int penc_scan_rows(const PencGeom &G, const PencScan &S) { return S.ss == 0 ? G.mcuy : G.hb[S.comp]; }
FI_PHD int penc_scan_blocks(const PencGeom &G, const PencScan &S) { return S.ss == 0 ? G.mcux * G.bpm : G.wb[S.comp]; }
// the DRI value of a scan: MCUs per row
FI_PHD int penc_scan_interval(const PencGeom &G, const PencScan &S) { return S.ss == 0 ? G.mcux : G.wb[S.comp]; }

// Worst-case bits a block adds to a scan's interval, for any int16
// coefficients (DESIGN.md 3.6b has the derivation)
FI_PHD int penc_block_bits(const PencScan &S) {
  const int nk = S.se - S.ss + 1;
  if (S.ss == 0) return S.ah ? 1 : 32;
  return S.ah ? 17 * nk + 60 : 31 * nk + 30;
}
// worst-case bytes of one interval's slot: stuffed, with its RSTn
FI_PHD size_t penc_slot_bytes(const PencScan &S, int blocks) {
  const size_t bits = (size_t)blocks * penc_block_bits(S) + 30;
  return ((bits + 7) / 8) * 2 + 2;
}

// Where the coefficient blocks (64 int16, zigzag order) lie.  planar: the
// layout of fi_debug_jpeg_coefs_host (a plane per component, padded to whole
// MCUs); else the MCU order k_jpeg_fdct writes.
struct PencLayout {
  const int16_t *base;
  int32_t planar, bpm, mcux;
  int64_t plane[3];
  int32_t pw[3];
};
FI_PHD const int16_t *penc_block(const PencLayout &L, int c, int bx, int by) {
  if (L.planar) return L.base + L.plane[c] + ((int64_t)by * L.pw[c] + bx) * 64;
  int64_t b;
  if (L.bpm == 1)
    b = (int64_t)by * L.mcux + bx;
  else if (L.bpm == 3)
    b = ((int64_t)by * L.mcux + bx) * 3 + c;
  else if (c == 0)
    b = ((int64_t)(by >> 1) * L.mcux + (bx >> 1)) * 6 + (by & 1) * 2 + (bx & 1);
  else
    b = ((int64_t)by * L.mcux + bx) * 6 + 3 + c;
  return L.base + b * 64;
}
// block j of MCU row r of an interleaved scan (jccoefct.c's dummy blocks included)
FI_PHD const int16_t *penc_block_mcu(const PencLayout &L, int r, int j, int *comp) {
  const int mx = j / L.bpm, k = j - mx * L.bpm;
  if (L.bpm == 6) {
    *comp = k >= 4 ? k - 3 : 0;
    return k >= 4 ? penc_block(L, k - 3, mx, r) : penc_block(L, 0, 2 * mx + (k & 1), 2 * r + (k >> 1));
  }
  *comp = k;
  return penc_block(L, k, mx, r);
}

FI_PHD int penc_nbits(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

// Entropy-coded bytes of one interval: MSB first, a zero byte stuffed after
// every 0xFF.  Nothing is stored at or beyond cap; n counts regardless.
struct PencByteSink {
  uint8_t *out;
  int64_t cap, n;
  uint32_t acc;
  int fill;
  const uint32_t *code;  // [2][256]: (length << 16) | code
  FI_PHD void init(uint8_t *o, int64_t c, const uint32_t *cd) {
    out = o;
    cap = c;
    n = 0;
    acc = 0;
    fill = 0;
    code = cd;
  }
  FI_PHD void byte(uint32_t b) {
    if (n < cap) out[n] = (uint8_t)b;
    n++;
  }
  FI_PHD void bits(uint32_t v, int nb) {  // nb <= 16
    if (!nb) return;
    acc = (acc << nb) | (v & ((1u << nb) - 1u));
    fill += nb;
    while (fill >= 8) {
      const uint32_t b = (acc >> (fill - 8)) & 255u;
      byte(b);
      if (b == 255u) byte(0);
      fill -= 8;
    }
  }
  FI_PHD void sym(int t, int s) {
    const uint32_t e = code[256 * t + s];
    bits(e & 0xFFFFu, (int)(e >> 16));
  }
  FI_PHD void finish() {  // jcphuff.c flush_bits: 1-bits to the byte boundary
    if (fill) bits((1u << (8 - fill)) - 1u, 8 - fill);
  }
};

// EOB run and buffered correction bits of an AC scan (jcphuff.c's EOBRUN, BE, bit_buffer)
struct PencRun {
  uint32_t eobrun, be;
  uint32_t corr[32];  // BE <= 937 + 63 bits
  FI_PHD uint32_t bit(uint32_t i) const { return (corr[i >> 5] >> (i & 31)) & 1u; }
  FI_PHD void set(uint32_t i, uint32_t b) { corr[i >> 5] = (corr[i >> 5] & ~(1u << (i & 31))) | (b << (i & 31)); }
};

template <class Sink>
FI_PHD void penc_emit_eobrun(Sink &sink, PencRun &R) {
  if (!R.eobrun) return;
  const int nb = penc_nbits(R.eobrun) - 1;  // <= 14: a run never reaches 0x7FFF (penc_interval)
  sink.sym(0, nb << 4);
  sink.bits(R.eobrun, nb);
  R.eobrun = 0;
  for (uint32_t i = 0; i < R.be; i++) sink.bits(R.bit(i), 1);
  R.be = 0;
}

// How an AC scan reaches a block's 64 coefficients: as they lie (the host), or
// through a copy nearer to the lane (the kernels stage each block in LDS: one
// round trip to memory per block, not one per coefficient)
struct PencDirect {
  FI_PHD const int16_t *load(const int16_t *b) { return b; }
};

// One restart interval (block row `row`) of scan S: jcphuff.c's
// encode_mcu_DC_first / DC_refine / AC_first / AC_refine over its blocks and
// the flush at its end.  A Sink takes sym(table slot 0 | 1, symbol) and
// bits(value, count).  Returns the correction-buffer flushes (BE beyond
// kPencCorrFlush) that ended an EOB run inside the interval.
template <class Sink, class Stage>
FI_PHD int penc_interval(const PencGeom &G, const PencScan &S, const PencLayout &L, int row, Sink &sink, Stage &stage) {
  const int nblk = penc_scan_blocks(G, S);
  const int al = S.al;
  if (S.ss == 0) {
    int last[3] = {0, 0, 0};
    for (int j = 0; j < nblk; j++) {
      int c;
      const int16_t *b = penc_block_mcu(L, row, j, &c);
      const int t = (int)b[0] >> al;
      if (S.ah) {
        sink.bits((uint32_t)t & 1u, 1);
        continue;
      }
      const int d = t - last[c];
      last[c] = t;
      const int nb = penc_nbits((uint32_t)(d < 0 ? -d : d));
      sink.sym(c ? 1 : 0, nb);
      sink.bits((uint32_t)(d < 0 ? d - 1 : d), nb);
    }
    return 0;
  }
  PencRun R;
  R.eobrun = 0;
  R.be = 0;
  int flushes = 0;
  const int ss = S.ss, se = S.se;
  for (int j = 0; j < nblk; j++) {  // (an interval is one block row, <= 8192 blocks: the run stays below 0x7FFF)
    const int16_t *b = stage.load(penc_block(L, S.comp, j, row));
    int r = 0;
    if (!S.ah) {
      for (int k = ss; k <= se; k++) {
        const int v = b[k];
        const int a = (v < 0 ? -v : v) >> al;
        if (!a) {
          r++;
          continue;
        }
        penc_emit_eobrun(sink, R);
        for (; r > 15; r -= 16) sink.sym(0, 0xF0);
        const int nb = penc_nbits((uint32_t)a);
        sink.sym(0, (r << 4) + nb);
        sink.bits((uint32_t)(v < 0 ? ~a : a), nb);
        r = 0;
      }
      if (r > 0) R.eobrun++;
      continue;
    }
    int eob = 0;  // the last newly nonzero coefficient
    for (int k = ss; k <= se; k++) {
      const int v = b[k];
      if (((v < 0 ? -v : v) >> al) == 1) eob = k;
    }
    uint32_t br0 = R.be, br = 0;  // this block's correction bits: corr[br0 .. br0 + br)
    for (int k = ss; k <= se; k++) {
      const int v = b[k];
      const int a = (v < 0 ? -v : v) >> al;
      if (!a) {
        r++;
        continue;
      }
      while (r > 15 && k <= eob) {
        penc_emit_eobrun(sink, R);
        sink.sym(0, 0xF0);
        r -= 16;
        for (uint32_t i = 0; i < br; i++) sink.bits(R.bit(br0 + i), 1);
        br0 = 0;
        br = 0;
      }
      if (a > 1) {
        R.set(br0 + br, (uint32_t)a & 1u);
        br++;
        continue;
      }
      penc_emit_eobrun(sink, R);
      sink.sym(0, (r << 4) + 1);
      sink.bits(v < 0 ? 0u : 1u, 1);
      for (uint32_t i = 0; i < br; i++) sink.bits(R.bit(br0 + i), 1);
      br0 = 0;
      br = 0;
      r = 0;
    }
    if (r > 0 || br > 0) {
      R.eobrun++;
      R.be += br;
      if (R.be > (uint32_t)kPencCorrFlush) {
        penc_emit_eobrun(sink, R);
        flushes++;
      }
    }
  }
  penc_emit_eobrun(sink, R);
  return flushes;
}
template <class Sink>
FI_PHD int penc_interval(const PencGeom &G, const PencScan &S, const PencLayout &L, int row, Sink &sink) {
  PencDirect direct;
  return penc_interval(G, S, L, row, sink, direct);
}

// jchuff.c jpeg_gen_optimal_table from a table's symbol counts: bits[1..16],
// the symbols by code length then value, and jpeg_make_c_derived_tbl's codes
// ((length << 16) | code; 0 for a symbol without one).  Returns the symbols.
FI_PHD int penc_gen_table(const uint32_t *counts, uint8_t bits_out[17], uint8_t *vals, uint32_t *code) {
  int64_t freq[257];
  int16_t others[257];
  uint8_t codesize[257];
  int16_t nz[257];  // symbols with a count, ascending: the searches below keep libjpeg's order
  int nnz = 0;
  for (int i = 0; i < 257; i++) {
    freq[i] = i == 256 ? 1 : (int64_t)counts[i];  // the reserved symbol keeps the all-ones code unused
    others[i] = -1;
    codesize[i] = 0;
    if (freq[i]) nz[nnz++] = (int16_t)i;
  }
  for (;;) {
    // the two least frequent symbols; of equal counts the larger symbol value
    int c1 = -1, c2 = -1;
    int64_t v = 1000000000L;
    for (int t = 0; t < nnz; t++) {
      const int i = nz[t];
      if (freq[i] && freq[i] <= v) {
        v = freq[i];
        c1 = i;
      }
    }
    v = 1000000000L;
    for (int t = 0; t < nnz; t++) {
      const int i = nz[t];
      if (freq[i] && freq[i] <= v && i != c1) {
        v = freq[i];
        c2 = i;
      }
    }
    if (c2 < 0) break;
    freq[c1] += freq[c2];
    freq[c2] = 0;
    codesize[c1]++;
    while (others[c1] >= 0) {
      c1 = others[c1];
      codesize[c1]++;
    }
    others[c1] = (int16_t)c2;
    codesize[c2]++;
    while (others[c2] >= 0) {
      c2 = others[c2];
      codesize[c2]++;
    }
  }
  int bits[33];
  for (int i = 0; i < 33; i++) bits[i] = 0;
  for (int t = 0; t < nnz; t++) {
    const int cs = codesize[nz[t]];
    if (cs) bits[cs > 32 ? 32 : cs]++;  // (257 symbols of counts below 2^32 stay well within 32)
  }
  int i;
  for (i = 32; i > 16; i--) {
    while (bits[i] > 0) {
      int j = i - 2;
      while (bits[j] == 0) j--;
      bits[i] -= 2;
      bits[i - 1]++;
      bits[j + 1] += 2;
      bits[j]--;
    }
  }
  while (bits[i] == 0) i--;
  bits[i]--;  // the reserved symbol's code
  for (int l = 0; l <= 16; l++) bits_out[l] = (uint8_t)bits[l];
  int p = 0;
  for (int l = 1; l <= 32; l++)
    for (int t = 0; t < nnz; t++)
      if (nz[t] < 256 && codesize[nz[t]] == l) vals[p++] = (uint8_t)nz[t];
  for (int s = 0; s < 256; s++) code[s] = 0;
  uint32_t cd = 0;
  int q = 0;
  for (int l = 1; l <= 16; l++) {
    for (int t = 0; t < bits[l]; t++) code[vals[q++]] = ((uint32_t)l << 16) | cd++;
    cd <<= 1;
  }
  return p;
}

// The DHT segment of a table: returns its length (<= kPencDhtMax)
FI_PHD int penc_write_dht(uint8_t *o, int tc_th, const uint8_t bits[17], const uint8_t *vals, int nvals) {
  const int len = 2 + 1 + 16 + nvals;
  o[0] = 0xFF;
  o[1] = 0xC4;
  o[2] = (uint8_t)(len >> 8);
  o[3] = (uint8_t)(len & 255);
  o[4] = (uint8_t)tc_th;
  for (int l = 1; l <= 16; l++) o[4 + l] = bits[l];
  for (int t = 0; t < nvals; t++) o[21 + t] = vals[t];
  return 2 + len;
}
// the tables scan S writes before its SOS: their count, and Tc << 4 | Th of each
FI_PHD int penc_scan_tables(const PencScan &S, int tc_th[2]) {
  if (S.ss == 0) {
    if (S.ah) return 0;
    tc_th[0] = 0x00;
    tc_th[1] = 0x01;
    return S.ncomp == 3 ? 2 : 1;
  }
  tc_th[0] = S.comp ? 0x11 : 0x10;
  return 1;
}

}  // namespace fi
