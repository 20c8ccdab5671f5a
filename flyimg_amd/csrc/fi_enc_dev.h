// fi_enc_dev.h -- device-only helpers the encoder kernels share
// (fi_png_enc.hip, fi_webp_enc.hip, fi_jpeg_enc.hip), all inlined into their
// callers: wave scan and sum, the bit offsets of a 256-thread chunk, the OR of
// a code into an LDS bit buffer, the image of a row / block of the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fi {

__device__ __forceinline__ int enc_scan64(int v) {  // inclusive prefix sum over the wave
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}
__device__ __forceinline__ uint32_t enc_sum64(uint32_t v) {  // sum over the wave, in every lane
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// A workgroup of 256 threads, each with nb bits to write: the bits of the
// threads before this one; *total = the chunk's bits.  wsum: 4 words of LDS,
// free again after the caller's next barrier.  (Holds a barrier: every thread
// of the workgroup calls it.)
__device__ __forceinline__ int enc_offset256(int nb, int *wsum, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = enc_scan64(nb);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int before = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k < wave) before += wsum[k];
    sum += wsum[k];
  }
  *total = sum;
  return before + incl - nb;
}

// ORs the low nb (<= 60) bits of v into the LSB-first bit buffer buf[0..words)
// at bit `bit`; false (nothing written) where they would leave the buffer.
// kGuard = false: the caller's chunk cannot leave its buffer by construction
// and the check is left out.
template <bool kGuard = true>
__device__ __forceinline__ bool enc_or_bits(uint32_t *buf, int words, int bit, uint64_t v, int nb) {
  const int w = bit >> 5, s = bit & 31;
  if (!nb) return true;
  if (kGuard && w + 2 >= words) return false;
  const uint32_t lo = (uint32_t)v << s;
  const uint64_t rest = v >> (32 - s);  // (s = 0: the bits from 32 up)
  if (lo) atomicOr(&buf[w], lo);
  if ((uint32_t)rest) atomicOr(&buf[w + 1], (uint32_t)rest);
  if ((uint32_t)(rest >> 32)) atomicOr(&buf[w + 2], (uint32_t)(rest >> 32));
  return true;
}

// the last of descs[0..n) whose start `field` is <= key: the image of row / block / MCU block `key`
template <typename D, typename T>
__device__ __forceinline__ int enc_find_image(const D *__restrict__ descs, int n, int64_t key, T D::*field) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (descs[mid].*field <= key)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace fi
