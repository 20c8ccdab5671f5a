// fi_enc_pack.h -- the device half of what the GPU encoders (baseline and
// progressive JPEG, PNG, WebP) share when they gather a batch's files into one
// contiguous stream: the exclusive scan of the item lengths and the copy of a
// slot to its (unaligned) place.  What an item is -- a restart interval, a
// piece, a band, a whole image -- is the codec's; the rest is here once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fi {

struct EncItem {      // what item k adds to the packed stream
  int64_t len;        // its bytes
  int img;            // its image in the batch
  bool first, last;   // of its image
};

// Exclusive scan of item(k).len over k < n by one workgroup of 256 threads,
// 256 items at a time with the running total carried in `base`.  dst[k] (dst
// may be null) = where item k starts; imgpos[2 i] / [2 i + 1] = start / end of
// image i, written by its first / last item.
template <typename Item>
__device__ __forceinline__ void enc_scan_items(int n, Item item, int64_t *__restrict__ dst,
                                               int64_t *__restrict__ imgpos) {
  __shared__ int64_t part[256];
  __shared__ int64_t base;
  const int t = threadIdx.x;
  if (t == 0) base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int k = i0 + t;
    EncItem I{0, 0, false, false};
    if (k < n) I = item(k);
    part[t] = I.len;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int64_t a = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += a;
      __syncthreads();
    }
    const int64_t start = base + part[t] - I.len;
    if (k < n) {
      if (dst) dst[k] = start;
      if (I.first) imgpos[2 * I.img] = start;
      if (I.last) imgpos[2 * I.img + 1] = start + I.len;
    }
    __syncthreads();
    if (t == 255) base += part[255];
    __syncthreads();
  }
}

// src[0, n) -> dst[0, n) by the threads t, t + step, ...: bytes until dst is
// dword aligned, dword stores (the source bytes come through the cache, src is
// not aligned with dst), bytes for the rest.  Needs step >= 3 threads.
__device__ __forceinline__ void enc_copy_aligned(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, int64_t n,
                                                 int64_t t, int64_t step) {
  const int64_t to_align = (int64_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
  const int64_t head = n < to_align ? n : to_align;
  if (t < head) dst[t] = src[t];
  const int64_t nw = (n - head) >> 2;
  uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
  const uint8_t *sw = src + head;
  for (int64_t i = t; i < nw; i += step) {
    const uint8_t *p = sw + 4 * i;
    dw[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  }
  const int64_t tail0 = head + 4 * nw;
  if (t < n - tail0) dst[tail0 + t] = src[tail0 + t];
}

}  // namespace fi
