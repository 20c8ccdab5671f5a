// fi_jpeg_prog.h -- the four block procedures of a progressive JPEG scan
// (libjpeg jdphuff.c: decode_mcu_DC_first, _DC_refine, _AC_first, _AC_refine),
// written once over the bit reader and the table type so that k_jpeg_prog
// (fi_jpeg.hip: the lockstep BitReader, tables in LDS) and the host decoder
// (fi_jpeg_prog_host.cpp: a byte reader, the same tables in host memory) run
// the same code; the host build is the one checked under ASan/UBSan.
//
// OPS supplies  static int sym(BR &, const TAB *)  -- one Huffman symbol, and
// deposit() (see jpeg_prog_correct).
// BR supplies fill() (>= 32 bits buffered, zero bits after a marker or the
// scan's end), peek(n) and skip(n), 1 <= n <= 24.
// `b` is the block's 64 coefficients in zigzag order; a first-pass procedure
// writes b[Ss .. Se] only.  The refinement procedures touch no memory: they
// work on bit masks of the block (JpegProgRefine).
#pragma once
#include <stdint.h>

#include "fi_internal.h"

namespace fi {

struct JpegProgState {  // per restart interval; wave-uniform on the device
  uint32_t eobrun;      // blocks of the running end-of-band run still to come
  int32_t pred[3];      // DC predictions of the scan's components
};

template <class BR>
__host__ __device__ inline uint32_t jpeg_prog_bits(BR &br, int n) {
  br.fill();
  const uint32_t r = br.peek(n);
  br.skip(n);
  return r;
}

// DC, first pass: the Huffman-coded difference, scaled by Al
template <class OPS, class BR, class TAB>
__host__ __device__ inline void jpeg_prog_dc_first(BR &br, const TAB *tab, int16_t *b, int32_t &pred, int Al) {
  int s = OPS::sym(br, tab) & 15;  // (a DC table's symbols are <= 15: jpeg_build_huff)
  if (s) {
    const uint32_t r = jpeg_prog_bits(br, s);
    s = r < (1u << (s - 1)) ? (int)r - (1 << s) + 1 : (int)r;  // HUFF_EXTEND
  }
  pred = (int32_t)((uint32_t)pred + (uint32_t)s);  // (corrupt data may wrap it; no signed overflow)
  b[0] = (int16_t)((uint32_t)pred << Al);
}

// DC, refinement: one more bit of every block (the caller ors 1 << Al in)
template <class BR>
__host__ __device__ inline bool jpeg_prog_dc_refine(BR &br) {
  return jpeg_prog_bits(br, 1) != 0;
}

// AC, first pass of the band Ss .. Se.  Both AC procedures return false where
// corrupt data makes libjpeg store a coefficient outside the band (it may be
// in another scan's band, or below 63's guard entry): such an image is left
// to the host decoder (FI_EUNSUPPORTED; k_jpeg_prog raises a per-image flag).
template <class OPS, class BR, class TAB>
__host__ __device__ inline bool jpeg_prog_ac_first(BR &br, const TAB *tab, int16_t *b, uint32_t &eobrun, int Ss, int Se,
                                                   int Al) {
  if (eobrun > 0) {  // the block is part of an end-of-band run
    eobrun--;
    return true;
  }
  bool ok = true;
  for (int k = Ss; k <= Se; k++) {
    const int rs = OPS::sym(br, tab);
    int r = rs >> 4, s = rs & 15;
    if (s) {
      k += r;
      const uint32_t v = jpeg_prog_bits(br, s);
      s = v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v;
      if (k <= Se)
        b[k] = (int16_t)((uint32_t)s << Al);
      else
        ok = false;  // (corrupt data: libjpeg writes past the band)
    } else if (r == 15) {
      k += 15;  // ZRL
    } else {    // EOBr: this block and 2^r - 1 + extra bits more
      eobrun = 1u << r;
      if (r) eobrun += jpeg_prog_bits(br, r);
      eobrun--;
      break;
    }
  }
  return ok;
}

// AC refinement works on bit masks of the block, bit z = zigzag coefficient z:
// in, of the block as the earlier scans left it: `nz` nonzero, `has` the bit
// being coded is already set (corrupt data only); out: `corr` correction to
// apply (+1 or -1 in the bit position, away from zero), `newp` / `newm` newly
// nonzero coefficients.  The device keeps one coefficient per lane and builds
// the masks with ballots, so the procedure itself touches no memory.
struct JpegProgRefine {
  uint64_t nz, has;
  uint64_t corr, newp, newm;
};

__host__ __device__ inline uint64_t jpeg_prog_below(int k) {  // bits 0 .. k - 1
  return k >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << k) - 1;
}

// The correction bits of the already-nonzero coefficients `m` a run passes,
// lowest coefficient first, read together.  OPS::deposit(bits, n, m) puts the
// n bits (the first one read = the most significant) on the set positions of
// m, lowest first.
template <class OPS, class BR>
__host__ __device__ inline void jpeg_prog_correct(BR &br, JpegProgRefine &R, uint64_t m) {
  const int n = __builtin_popcountll(m);
  if (n == 0) return;
  uint64_t bits = 0;
  for (int left = n; left > 0;) {
    const int t = left < 24 ? left : 24;
    bits = (bits << t) | jpeg_prog_bits(br, t);
    left -= t;
  }
  R.corr |= OPS::deposit(bits, n, m) & ~R.has;
}

// AC, refinement of the band Ss .. Se.  jdphuff.c walks the band coefficient
// by coefficient: a run of r skips r still-zero coefficients and stops at the
// next one, and every nonzero coefficient on the way takes one correction
// bit.  Where the run ends depends on the zero positions only, so here it is
// found from the mask and the correction bits it passes are read in one go.
template <class OPS, class BR, class TAB>
__host__ __device__ inline bool jpeg_prog_ac_refine(BR &br, const TAB *tab, JpegProgRefine &R, uint32_t &eobrun, int Ss,
                                                    int Se) {
  const uint64_t band = jpeg_prog_below(Se + 1);
  int k = Ss;
  bool ok = true;
  if (eobrun == 0) {
    for (; k <= Se; k++) {
      const int rs = OPS::sym(br, tab);
      const int r = rs >> 4;
      int s = rs & 15;
      if (s) {  // a newly nonzero coefficient: its size is 1 (libjpeg warns otherwise and goes on alike)
        s = jpeg_prog_bits(br, 1) ? 1 : -1;
      } else if (r != 15) {
        eobrun = 1u << r;
        if (r) eobrun += jpeg_prog_bits(br, r);
        break;  // the rest of the block is handled by the EOB logic
      }
      // skip r still-zero coefficients (ZRL: s = 0, r = 15) to the next one
      const uint64_t from = band & ~jpeg_prog_below(k);
      uint64_t zm = ~R.nz & from;
      for (int i = 0; i < r && zm; i++) zm &= zm - 1;
      const int kend = zm ? __builtin_ctzll(zm) : Se + 1;  // the target zero coefficient
      jpeg_prog_correct<OPS>(br, R, R.nz & from & jpeg_prog_below(kend));
      k = kend;
      if (s && k <= Se)
        (s > 0 ? R.newp : R.newm) |= (uint64_t)1 << k;
      else if (s)
        ok = false;  // (corrupt data: libjpeg stores at k = Se + 1 too)
    }
  }
  if (eobrun > 0) {  // correction bits for the rest of the band
    if (k <= Se) jpeg_prog_correct<OPS>(br, R, R.nz & band & ~jpeg_prog_below(k));
    eobrun--;
  }
  return ok;
}

// coefficient z after the refinement: jdphuff.c's p1 / m1 rule
__host__ __device__ inline int16_t jpeg_prog_refined(int16_t c, int z, const JpegProgRefine &R, int Al) {
  const int p1 = 1 << Al, m1 = -(1 << Al);  // 1 and -1 in the bit position being coded
  if ((R.corr >> z) & 1) return (int16_t)(c >= 0 ? c + p1 : c + m1);
  if ((R.newp >> z) & 1) return (int16_t)p1;
  if ((R.newm >> z) & 1) return (int16_t)m1;
  return c;
}

// the block of MCU `mcu`, component slot k, sub-block (by, bx) in the padded grid
__host__ __device__ inline int64_t jpeg_prog_block(const JpegProgItem &I, int mcu, int hs, int vs, int by, int bx,
                                                   int bw) {
  const int my = mcu / I.mcux, mx = mcu - my * I.mcux;
  const int row = I.ns == 1 ? my : my * vs + by, col = I.ns == 1 ? mx : mx * hs + bx;
  return (int64_t)row * bw + col;
}

}  // namespace fi
