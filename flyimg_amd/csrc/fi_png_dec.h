// fi_png_dec.h -- what the GPU PNG decoder's device half (fi_png_dec.hip) and
// host half (fi_png_parse.cpp) share: the parsed source, and -- as plain
// inline functions that compile for the host and the device alike -- the
// inflater: bit reader, decode-table construction, symbol decode, the 32 KiB
// ring and zlib's validity rules.  The functions take (lane, nlanes): the
// device runs them with the 64 lanes of a wave in wave-uniform control flow
// (the lanes share the table fill, a match's bytes and the flushes, and
// FI_PNG_SYNC orders their LDS traffic), the host with (0, 1), so
// tests/native/png_read_driver.cpp runs under ASan/UBSan the very code the
// device runs.  No HIP header is needed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "fi_png_sum.h"

// FI_PNG_UNI marks a value every lane holds alike (read from LDS at a uniform
// address): the compiler then keeps the bit buffer, the positions and the
// branches that depend on them on the scalar unit.  (FI_PNG_WAVE: defined by
// fi_png_dec.hip, the one file whose device code calls these functions.)
#if defined(__HIP_DEVICE_COMPILE__) && defined(FI_PNG_WAVE)
#define FI_PNG_SYNC() __syncthreads()
#define FI_PNG_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define FI_PNG_SYNC() ((void)0)
#define FI_PNG_UNI(x) ((uint32_t)(x))
#endif

namespace fi {

// ---- host: the file (fi_png_parse.cpp) -------------------------------------------
struct PngSrc {
  int32_t w = 0, h = 0;
  int32_t channels = 0;    // natural count: 1, 2, 3, 4; palette 3, with tRNS 4
  int32_t color_type = 0;  // 0, 2, 3, 4, 6
  int32_t bpp = 0;         // bytes per pixel of the filtered stream (palette: 1)
  int32_t meta = 0;        // FI_PNG_META_*
  bool palette = false;
  uint32_t pal[256];       // r | g << 8 | b << 16 | a << 24, Pillow's convert() rules for missing entries
  std::vector<std::pair<size_t, size_t>> idat;  // (offset, length) of every IDAT payload
  size_t zbytes = 0;       // their sum: the zlib stream
};
// FI_OK only for files the device path reproduces exactly, FI_EUNSUPPORTED =
// decode on the host, FI_EINVAL = no signature or a broken IHDR
int png_parse(const uint8_t *data, size_t len, PngSrc *out);
// the IDAT payloads back to back -> dst (zbytes bytes)
void png_copy_zstream(const uint8_t *data, const PngSrc &S, uint8_t *dst);
// FI_OK, or FI_EINVAL where out_channels (0, 3, 4) does not fit the source; *outc = the channels written
int png_out_channels(const PngSrc &S, int out_channels, int *outc);

// ---- the inflater -------------------------------------------------------------------
// CMF / FLG as zlib's inflate takes them: deflate, a window up to 32 KiB, the check bits, no dictionary
FI_ENC_HD bool png_zlib_header_ok(uint32_t cmf, uint32_t flg) {
  return (cmf & 15u) == 8u && (cmf >> 4) <= 7u && !(flg & 0x20u) && ((cmf << 8) | flg) % 31u == 0u;
}
constexpr int kPngRing = 32768;      // the window, a ring
constexpr int kPngPrimBits = 9;      // primary lookup: the low 9 bits of the bit buffer
constexpr int kPngFlushBytes = 4096; // ring -> stream whenever this much is waiting
enum PngDecErr {                     // nonzero: the image ends with FI_EINVAL
  kPngErrInput = 1,     // the input ends early
  kPngErrBlockType,     // BTYPE 3
  kPngErrStored,        // LEN / NLEN
  kPngErrCounts,        // HLIT > 286 or HDIST > 30
  kPngErrCodeLens,      // the code-length code: over-subscribed, incomplete, no previous length, run too long
  kPngErrNoEob,         // no end-of-block code
  kPngErrLitLen,        // lit/len set over-subscribed or incomplete
  kPngErrDist,          // distance set over-subscribed, or incomplete with more than one code
  kPngErrSymbol,        // a code outside the set, lit/len 286 / 287, distance 30 / 31
  kPngErrFar,           // a distance that reaches before the start of the output
  kPngErrLong,          // output beyond the expected size
  kPngErrShort,         // the stream ends before the expected size
  kPngErrAdler,         // Adler-32 mismatch
  kPngErrFilter,        // a filter byte above 4
};

struct alignas(16) PngDecTabs {  // per wave, in LDS on the device
  uint16_t lprim[1 << kPngPrimBits], dprim[1 << kPngPrimBits], cprim[128];  // sym | len << 9; 0 = take the walk
  uint16_t lsym[288], dsym[32], csym[19];   // symbols in canonical order
  uint16_t lcount[16], dcount[16], ccount[16];
  uint16_t code[320];                       // scratch of png_dec_build
  uint8_t lens[320];                        // lit/len lengths, then distance lengths
  uint8_t cl[19];
};

// the payload as the bit reader sees it: word(pos) = the four bytes at pos, the first in
// the low bits, 0 behind the end
struct PngHostIn {
  const uint8_t *p;
  uint32_t n;
  FI_ENC_HD uint32_t word(uint32_t pos) const {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; k++)
      if (pos + k < n) v |= (uint32_t)p[pos + k] << (8 * k);
    return v;
  }
};
// Where the canonical walk stands behind the primary table's lengths: codes
// longer than kPngPrimBits bits continue from here, the counts in registers.
struct PngWalk {
  int32_t first, index;
  int32_t cnt[15 - kPngPrimBits];
};
FI_ENC_HD PngWalk png_walk_init(const uint16_t *count) {
  PngWalk W;
  W.first = 0;
  W.index = 0;
  for (int l = 1; l <= kPngPrimBits; l++) {
    const int c = (int)FI_PNG_UNI(count[l]);
    W.index += c;
    W.first = (W.first + c) << 1;
  }
  for (int l = kPngPrimBits + 1; l < 16; l++) W.cnt[l - kPngPrimBits - 1] = (int)FI_PNG_UNI(count[l]);
  return W;
}
// the primary tables as the symbol loop reads them: the device keeps them in registers
// (fi_png_dec.hip), load() after every table build
struct PngHostLook {
  const PngDecTabs *T;
  PngWalk lw, dw;
  FI_ENC_HD void load(const PngDecTabs *t, int) {
    T = t;
    lw = png_walk_init(t->lcount);
    dw = png_walk_init(t->dcount);
  }
  FI_ENC_HD uint32_t lprim(uint32_t i) const { return T->lprim[i]; }
  FI_ENC_HD uint32_t dprim(uint32_t i) const { return T->dprim[i]; }
};

template <class In>
struct PngBits {
  In in;
  uint32_t n;    // payload bytes
  uint32_t pos;  // bytes taken into buf (virtual zero bytes behind the end included)
  uint64_t buf;
  int cnt;
  FI_ENC_HD void fill() {  // >= 33 bits: a code of 15 bits and its 13 extra bits, or a stored block's LEN / NLEN
    if (cnt <= 32) {
      buf |= (uint64_t)in.word(pos) << cnt;
      pos += 4;
      cnt += 32;
    }
  }
  FI_ENC_HD uint32_t peek(int nb) const { return (uint32_t)(buf & ((1ull << nb) - 1ull)); }
  FI_ENC_HD void drop(int nb) {
    buf >>= nb;
    cnt -= nb;
  }
  FI_ENC_HD uint32_t take(int nb) {  // nb <= 32, after fill()
    const uint32_t v = peek(nb);
    drop(nb);
    return v;
  }
  // bits consumed went past the payload: the zero bits fill() supplied were used
  FI_ENC_HD bool over() const { return (uint64_t)pos * 8u - (uint64_t)cnt > (uint64_t)n * 8u; }
  FI_ENC_HD uint32_t byte_pos() const { return pos - (uint32_t)(cnt >> 3); }  // once byte aligned
};

// Canonical codes of len[0..n-1] (<= 15 bits): count[l], sym[] in canonical
// order, and the primary table over the low primbits bits.  Returns 0, 1 =
// over-subscribed, 2 = incomplete (the tables are built all the same); *maxlen
// = the longest length.  Lane 0 assigns the codes, the lanes fill the table.
FI_ENC_HD int png_dec_build(const uint8_t *len, int n, uint16_t *count, uint16_t *sym, uint16_t *prim, int primbits,
                            uint16_t *code, int *maxlen, int lane, int nlanes) {
  FI_PNG_SYNC();  // the lengths are written, the previous tables are no longer read
  for (int i = lane; i < (1 << primbits); i += nlanes) prim[i] = 0;
  if (lane == 0) {
    uint16_t offs[16], next[16];
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    offs[1] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int l = 1; l < 16; l++) {
      c = (c + count[l - 1]) << 1;
      next[l] = (uint16_t)c;
      if (l < 15) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    }
    for (int s = 0; s < n; s++) {
      const int l = len[s];
      if (!l) continue;
      sym[offs[l]++] = (uint16_t)s;
      code[s] = next[l]++;
    }
  }
  FI_PNG_SYNC();
  int left = 1, mx = 0, res = 0;
  for (int l = 1; l < 16; l++) {
    left <<= 1;
    left -= (int)FI_PNG_UNI(count[l]);
    if (left < 0) {
      res = 1;
      break;
    }
    if (FI_PNG_UNI(count[l])) mx = l;
  }
  if (!res && left > 0) res = 2;
  *maxlen = mx;
  if (res == 1) return res;  // (an over-subscribed set has no canonical codes)
  for (int s = lane; s < n; s += nlanes) {
    const int l = len[s];
    if (!l || l > primbits) continue;
    uint32_t r = 0;
    const uint32_t c = code[s];
    for (int k = 0; k < l; k++) r |= ((c >> k) & 1u) << (l - 1 - k);
    for (uint32_t k = r; k < (1u << primbits); k += 1u << l) prim[k] = (uint16_t)(s | (l << 9));
  }
  FI_PNG_SYNC();
  return res;
}

// One symbol (after fill()): e = the primary table's entry for the next bits;
// where it is 0 the code is longer: the canonical walk bit by bit (as
// jpeg_decode_sym); -1 = a code outside the set
template <class In>
FI_ENC_HD int png_dec_sym(PngBits<In> &b, uint32_t e, const uint16_t *count, const uint16_t *sym) {
  if (e) {
    b.drop((int)(e >> 9));
    return (int)(e & 511u);
  }
  uint64_t v = b.buf;
  int code = 0, first = 0, index = 0;
  for (int l = 1; l < 16; l++) {
    code |= (int)(v & 1u);
    v >>= 1;
    const int c = (int)FI_PNG_UNI(count[l]);
    if (code - first < c) {
      b.drop(l);
      return (int)FI_PNG_UNI(sym[index + (code - first)]);
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// A lit/len or distance symbol (after fill()): e = the primary table's entry;
// where it is 0 the code has more than kPngPrimBits bits and the walk goes on
// from W, one bit per length; -1 = a code outside the set
template <class In>
FI_ENC_HD int png_dec_sym_w(PngBits<In> &b, uint32_t e, const PngWalk &W, const uint16_t *sym) {
  if (e) {
    b.drop((int)(e >> 9));
    return (int)(e & 511u);
  }
  uint64_t v = b.buf >> kPngPrimBits;
  int code = (int)(__builtin_bitreverse32(b.peek(kPngPrimBits)) >> (32 - kPngPrimBits)) << 1;
  int first = W.first, index = W.index;
#pragma unroll
  for (int l = kPngPrimBits + 1; l < 16; l++) {
    code |= (int)(v & 1u);
    v >>= 1;
    const int c = W.cnt[l - kPngPrimBits - 1];
    if (code - first < c) {
      b.drop(l);
      return (int)FI_PNG_UNI(sym[index + (code - first)]);
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// ring[from, to) -> out: whole dwords while `to` allows (from and out are dword
// aligned), single bytes for the rest when `all`; returns the new `from`.
// Every store stays below cap.
FI_ENC_HD uint32_t png_dec_flush(const uint8_t *ring, uint8_t *out, uint32_t cap, uint32_t from, uint32_t to, bool all,
                                 int lane, int nlanes) {
  FI_PNG_SYNC();
  const uint32_t nw = (to - from) >> 2;
  const uint32_t *rw = reinterpret_cast<const uint32_t *>(ring);
  uint32_t *ow = reinterpret_cast<uint32_t *>(out);
  for (uint32_t i = (uint32_t)lane; i < nw; i += (uint32_t)nlanes) {
    const uint32_t p = from + 4u * i;
    if (p + 4u <= cap) ow[p >> 2] = rw[(p & (kPngRing - 1)) >> 2];
  }
  from += 4u * nw;
  if (all) {
    for (uint32_t p = from + (uint32_t)lane; p < to; p += (uint32_t)nlanes)
      if (p < cap) out[p] = ring[p & (kPngRing - 1)];
    from = to;
  }
  return from;
}

// Inflates the zlib stream `raw` (n bytes, header included) to exactly `expect`
// bytes in out (capacity cap >= expect, dword aligned), through the ring (kPngRing
// bytes, dword aligned).  Returns 0 or a PngDecErr; *trailer = the stream's
// Adler-32.  Terminates on any bytes: every iteration consumes input bits or
// emits output, and bits behind the payload are zeros that end the image.
template <class In, class Look>
FI_ENC_HD int png_inflate(In in, Look look, const uint8_t *raw, uint32_t n, uint8_t *ring, PngDecTabs *T, uint8_t *out,
                          uint32_t cap, uint32_t expect, uint32_t *trailer, int lane, int nlanes) {
  constexpr uint8_t clord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  PngBits<In> b{in, n, 2u, 0ull, 0};  // behind CMF / FLG (fi_png_info checked them)
  uint32_t o = 0, flushed = 0;        // bytes produced, bytes stored
  int err = 0;
  if (expect > cap) return kPngErrLong;
  for (bool last = false; !last && !err;) {
    b.fill();
    last = b.take(1) != 0;
    const uint32_t type = b.take(2);
    if (b.over()) {
      err = kPngErrInput;
      break;
    }
    if (type == 3) {
      err = kPngErrBlockType;
      break;
    }
    if (type == 0) {
      b.drop(b.cnt & 7);
      b.fill();
      const uint32_t ln = b.take(16), nl = b.take(16);
      if (b.over()) {
        err = kPngErrInput;
        break;
      }
      if ((ln ^ 0xFFFFu) != nl) {
        err = kPngErrStored;
        break;
      }
      uint32_t ip = b.byte_pos();
      if (ln > n - ip) {
        err = kPngErrInput;
        break;
      }
      if (ln > expect - o) {
        err = kPngErrLong;
        break;
      }
      for (uint32_t done = 0; done < ln;) {  // a wave-wide copy, a flush's worth at a time
        const uint32_t m = ln - done < (uint32_t)kPngFlushBytes ? ln - done : (uint32_t)kPngFlushBytes;
        FI_PNG_SYNC();
        for (uint32_t i = (uint32_t)lane; i < m; i += (uint32_t)nlanes) ring[(o + i) & (kPngRing - 1)] = raw[ip + i];
        o += m;
        ip += m;
        done += m;
        flushed = png_dec_flush(ring, out, cap, flushed, o, false, lane, nlanes);
      }
      b.pos = ip;
      b.buf = 0;
      b.cnt = 0;
      continue;
    }
    int hlit = 288, hdist = 32;
    if (type == 1) {
      FI_PNG_SYNC();
      for (int s = lane; s < 288; s += nlanes) T->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
      for (int s = lane; s < 32; s += nlanes) T->lens[288 + s] = 5;
    } else {
      hlit = (int)b.take(5) + 257;
      hdist = (int)b.take(5) + 1;
      const int hclen = (int)b.take(4) + 4;
      if (hlit > 286 || hdist > 30) {
        err = kPngErrCounts;
        break;
      }
      FI_PNG_SYNC();
      if (lane == 0) {
        for (int i = 0; i < 19; i++) T->cl[i] = 0;
      }
      for (int i = 0; i < hclen; i++) {
        b.fill();
        const uint32_t v = b.take(3);
        if (lane == 0) T->cl[clord[i]] = (uint8_t)v;
      }
      if (b.over()) {
        err = kPngErrInput;
        break;
      }
      int mx = 0;
      if (png_dec_build(T->cl, 19, T->ccount, T->csym, T->cprim, 7, T->code, &mx, lane, nlanes) || mx == 0) {
        err = kPngErrCodeLens;
        break;
      }
      // the lit/len and distance lengths are one sequence: a 16 / 17 / 18 run may cross the boundary
      const int total = hlit + hdist;
      int prev = -1;
      for (int i = 0; i < total && !err;) {
        b.fill();
        const int s = png_dec_sym(b, FI_PNG_UNI(T->cprim[b.peek(7)]), T->ccount, T->csym);
        int rep = 1, val = s;
        if (s < 0) {
          err = kPngErrCodeLens;
        } else if (s == 16) {
          val = prev;
          rep = 3 + (int)b.take(2);
          if (prev < 0) err = kPngErrCodeLens;
        } else if (s == 17) {
          val = 0;
          rep = 3 + (int)b.take(3);
        } else if (s == 18) {
          val = 0;
          rep = 11 + (int)b.take(7);
        }
        if (!err && b.over()) err = kPngErrInput;
        if (!err && i + rep > total) err = kPngErrCodeLens;
        if (err) break;
        for (int k = lane; k < rep; k += nlanes) T->lens[(i + k < hlit ? 0 : 288 - hlit) + i + k] = (uint8_t)val;
        i += rep;
        prev = val;
      }
      if (err) break;
      FI_PNG_SYNC();
      if (FI_PNG_UNI(T->lens[256]) == 0) {
        err = kPngErrNoEob;
        break;
      }
    }
    int mx = 0;
    if (png_dec_build(T->lens, hlit, T->lcount, T->lsym, T->lprim, kPngPrimBits, T->code, &mx, lane, nlanes)) {
      err = kPngErrLitLen;
      break;
    }
    const int dr = png_dec_build(T->lens + 288, hdist, T->dcount, T->dsym, T->dprim, kPngPrimBits, T->code, &mx, lane,
                                 nlanes);
    if (dr == 1 || (dr == 2 && mx > 1)) {  // (zlib: one distance code of one bit, or none, may stay incomplete)
      err = kPngErrDist;
      break;
    }
    look.load(T, lane);
    for (;;) {  // the symbol loop
      b.fill();
      const int s = png_dec_sym_w(b, look.lprim(b.peek(kPngPrimBits)), look.lw, T->lsym);
      if (b.over()) {
        err = kPngErrInput;
        break;
      }
      if (s < 0 || s > 285) {
        err = kPngErrSymbol;
        break;
      }
      if (s < 256) {
        if (o >= expect) {
          err = kPngErrLong;
          break;
        }
        if (lane == 0) ring[o & (kPngRing - 1)] = (uint8_t)s;
        o++;
      } else if (s == 256) {
        break;
      } else {
        const int le = s < 265 || s == 285 ? 0 : (s - 261) >> 2;
        const int ln = s == 285 ? 258 : s < 265 ? s - 254 : 3 + ((4 + ((s - 261) & 3)) << le) + (int)b.take(le);
        b.fill();
        const int ds = png_dec_sym_w(b, look.dprim(b.peek(kPngPrimBits)), look.dw, T->dsym);
        if (ds < 0 || ds > 29) {
          err = b.over() ? kPngErrInput : kPngErrSymbol;
          break;
        }
        const int de = enc_prefix_extra(ds);
        const uint32_t dist = ds < 4 ? (uint32_t)ds + 1u : 1u + ((2u + ((uint32_t)ds & 1u)) << de) + b.take(de);
        if (b.over()) {
          err = kPngErrInput;
          break;
        }
        if (dist > o) {
          err = kPngErrFar;
          break;
        }
        if ((uint32_t)ln > expect - o) {
          err = kPngErrLong;
          break;
        }
        // byte i comes from i % dist behind the match's start: never a byte this match writes.  At
        // distances near the ring's size a byte's slot is another byte's source: read, then write.
        FI_PNG_SYNC();
        for (int i0 = 0; i0 < ln; i0 += nlanes) {
          const int i = i0 + lane;
          uint8_t v = 0;
          if (i < ln) v = ring[(o - dist + (dist >= (uint32_t)ln ? (uint32_t)i : (uint32_t)i % dist)) & (kPngRing - 1)];
          FI_PNG_SYNC();
          if (i < ln) ring[(o + (uint32_t)i) & (kPngRing - 1)] = v;
        }
        o += (uint32_t)ln;
      }
      if (o - flushed >= (uint32_t)kPngFlushBytes) flushed = png_dec_flush(ring, out, cap, flushed, o, false, lane, nlanes);
    }
  }
  flushed = png_dec_flush(ring, out, cap, flushed, o, true, lane, nlanes);
  if (err) return err;
  if (o != expect) return kPngErrShort;
  b.drop(b.cnt & 7);
  b.fill();
  uint32_t t = 0;
  for (int k = 0; k < 4; k++) t = (t << 8) | b.take(8);
  if (b.over()) return kPngErrInput;
  *trailer = t;
  return 0;
}

// Adler-32 of d[0..n): partial sums per segment, combined (png_adler_append)
FI_ENC_HD uint32_t png_dec_adler(const uint8_t *d, uint32_t n, uint32_t seg) {
  uint32_t a = 1, b = 0;
  for (uint32_t s0 = 0; s0 < n; s0 += seg) {
    const uint32_t m = n - s0 < seg ? n - s0 : seg;
    uint64_t sa = 0, sb = 0;
    for (uint32_t i = 0; i < m; i++) {
      sa += d[s0 + i];
      sb += (uint64_t)d[s0 + i] * (m - i);
    }
    png_adler_append(&a, &b, (uint32_t)(sa % 65521u), (uint32_t)(sb % 65521u), m);
  }
  return (b << 16) | a;
}

// ---- filters ---------------------------------------------------------------------------
FI_ENC_HD int png_dec_paeth(int a, int b, int c) {  // the order a, then b, then c
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// one reconstructed byte: x = the filtered byte, a / b / c = left, above, above left
FI_ENC_HD int png_dec_recon(int ft, int x, int a, int b, int c) {
  const int p = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : png_dec_paeth(a, b, c);
  return (x + p) & 255;
}

}  // namespace fi
