// fi_png_sum.h -- the checksum arithmetic of zlib streams and PNG chunks that
// the GPU PNG encoder (fi_png_enc.h) and decoder (fi_png_dec.h) share, as plain
// inline functions that compile for the host and the device alike: CRC-32 of
// a concatenation from the parts' CRCs, Adler-32 from per-band partial sums.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fi_enc_code.h"

namespace fi {

uint32_t png_crc32(uint32_t crc, const uint8_t *p, size_t n);  // zlib's crc32() (fi_png_write.cpp)

// ---- CRC-32 (reflected, polynomial 0xEDB88320) ---------------------------------
// One byte through the register, bit by bit (the kernels build their 256-entry
// table from it).
FI_ENC_HD uint32_t png_crc_byte(uint32_t c) {
  for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  return c;
}
// a * b mod P in the reflected representation (bit 31 = x^0)
FI_ENC_HD uint32_t png_crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int k = 0; k < 32; k++) {
    r ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return r;
}
// x^(8 n) mod P
FI_ENC_HD uint32_t png_crc_xpow8(uint64_t n) {
  uint32_t r = 0x80000000u;  // x^0
  uint32_t sq = 0x00800000u; // x^8
  for (; n; n >>= 1) {
    if (n & 1) r = png_crc_mulmod(r, sq);
    sq = png_crc_mulmod(sq, sq);
  }
  return r;
}
// crc32(A || B) from crc32(A), crc32(B) and B's length
FI_ENC_HD uint32_t png_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return png_crc_mulmod(crc_a, png_crc_xpow8(len_b)) ^ crc_b;
}

// ---- Adler-32 ------------------------------------------------------------------
// A band of n bytes d[0..n-1] contributes sa = sum d[i] and sb = sum (n - i) d[i],
// both mod 65521; (a, b) is the running checksum (1, 0 before the first byte).
FI_ENC_HD void png_adler_append(uint32_t *a, uint32_t *b, uint32_t sa, uint32_t sb, uint32_t n) {
  *b = (uint32_t)((*b + (uint64_t)(n % 65521u) * *a + sb) % 65521u);
  *a = (*a + sa) % 65521u;
}

}  // namespace fi
