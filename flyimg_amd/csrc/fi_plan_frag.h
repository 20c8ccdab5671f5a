// fi_plan_frag.h -- internal to the planner (fi_plan_mfma.cpp, fi_plan_sc.cpp):
// integer weights as signed-byte limbs in v_mfma_i32_16x16x64_i8 operand
// order.  With fi_internal.h mfma_i8_k this is the one place that knows the
// byte order of a host-built fragment.
#pragma once
#include "fi_plan.h"

namespace fi {

// k = sum out[q] 256^q: balanced signed base-256 digits (each in [-128, 127]),
// the last limb taking the remainder
template <int N, class T>
inline void limbs(T k, T out[N]) {
  for (int q = 0; q + 1 < N; q++) {
    out[q] = ((k + 128) & 255) - 128;
    k = (k - out[q]) / 256;
  }
  out[N - 1] = k;
}

// The N limb fragments (256 int32 = 64 lanes x 16 bytes each, consecutive from
// frag[base]) of one 16 x 64 operand block: w(r, k) is the integer weight of
// row (A) / column (B) r = 0..15 at K slot k = 0..63.
template <int N, class W>
inline void fill_frag(std::vector<int32_t> &frag, size_t base, const W &w) {
  uint8_t *b = reinterpret_cast<uint8_t *>(&frag[base]);
  for (int l = 0; l < 64; l++)
    for (int j = 0; j < 16; j++) {
      int32_t limb[N];
      limbs<N>((int32_t)w(l & 15, mfma_i8_k(l, j)), limb);
      for (int q = 0; q < N; q++) b[q * 1024 + l * 16 + j] = (uint8_t)(int8_t)limb[q];
    }
}

}  // namespace fi
