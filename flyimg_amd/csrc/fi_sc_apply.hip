// fi_sc_apply.hip -- smartcrop.py's saliency stage, part 3: k_crop_apply3 /
// k_crop_apply3p, convert -crop of the winning box (SmartCropProcessor.php:30-34).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fi_internal.h"

namespace fi {

// convert <out> -crop WxH+X+Y with W = w + x, H = h + y as smartcrop.py prints
// them (:372-377); CropImage clips to the image.  kApplyBands workgroups per
// image, rows interleaved.
#ifndef FI_APPLY_WG
#define FI_APPLY_WG 8
#endif
constexpr int kApplyChunks = FI_APPLY_WG;  // workgroups per image
// The output is one contiguous byte array (oh rows of ow * C bytes): 16-byte
// destination chunks, each assembled from 5 aligned source dwords with
// v_alignbyte (the crop origin has any byte alignment); chunks that straddle a
// row end, and the unaligned head/tail of the array, go byte by byte.
__device__ __forceinline__ uint32_t ap_align(uint32_t hi, uint32_t lo, uint32_t sh) {
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
}
#ifndef FI_APPLY_U
#define FI_APPLY_U 2
#endif
constexpr int kApplyU = FI_APPLY_U;  // chunks per thread whose loads go out together
// one (image, part) of the crop copy: part of nparts workgroup-sized slices
__device__ __forceinline__ void crop_apply_item(const ApplyDesc *__restrict__ descs, const DevCrop *__restrict__ crops,
                                                const ScResult *__restrict__ results, int img, int part, int nparts) {
  const ApplyDesc &A = descs[img];
  const ScResult r = results[A.result];
  if (r.top < 0) return;
  const DevCrop c = crops[A.crop0 + r.top];
  const int gw = c.rw + c.rx, gh = c.rh + c.ry;
  const int ow = min(gw, A.W - c.rx), oh = min(gh, A.H - c.ry);
  if (part == 0 && threadIdx.x == 0) {
    A.out_wh[0] = ow;
    A.out_wh[1] = oh;
  }
  const int rowb = ow * A.C;
  const int64_t total = (int64_t)rowb * oh;
  if (total <= 0) return;
  const uint8_t *src0 = A.src + (int64_t)c.ry * A.src_stride + (int64_t)c.rx * A.C;
  // (row, byte) of output offset o: float reciprocal + exact correction (no
  // 64-bit division; total = rowb * oh < 2^31 for any thumbnail)
  const float inv_rowb = 1.0f / (float)rowb;
  auto rowcol = [&](int64_t o, int *y_, int *x_) {
    const int oo = (int)o;
    int y = (int)((float)oo * inv_rowb);
    int x = oo - y * rowb;
    while (x < 0) {
      y--;
      x += rowb;
    }
    while (x >= rowb) {
      y++;
      x -= rowb;
    }
    *y_ = y;
    *x_ = x;
  };
  auto src_of = [&](int64_t o) {
    int y, x;
    rowcol(o, &y, &x);
    return src0 + (int64_t)y * A.src_stride + x;
  };
  const int head = (int)((16 - ((uintptr_t)A.dst & 15)) & 15);
  const int64_t nchunk = head < total ? (total - head) / 16 : 0;
  const int64_t tail0 = head + 16 * nchunk;
  const int tid = threadIdx.x;
  if (part == 0) {
    for (int64_t o = tid; o < min<int64_t>(head, total); o += 256) A.dst[o] = *src_of(o);
    for (int64_t o = tail0 + tid; o < total; o += 256) A.dst[o] = *src_of(o);
  }
  const int64_t cs = (int64_t)nparts * 256;
  for (int64_t k0 = (int64_t)part * 256 + tid; k0 < nchunk; k0 += kApplyU * cs) {
    uint4 out[kApplyU];
#pragma unroll
    for (int u = 0; u < kApplyU; u++) {
      const int64_t k = k0 + u * cs;
      if (k >= nchunk) break;
      const int64_t o = head + 16 * k;
      int y, x;
      rowcol(o, &y, &x);
      if (x + 16 <= rowb) {
        const uint8_t *s = src0 + (int64_t)y * A.src_stride + x;
        const uint32_t *sa = reinterpret_cast<const uint32_t *>((uintptr_t)s & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
        const uint32_t w0 = sa[0], w1 = sa[1], w2 = sa[2], w3 = sa[3], w4 = sh ? sa[4] : 0u;
        out[u].x = ap_align(w1, w0, sh);
        out[u].y = ap_align(w2, w1, sh);
        out[u].z = ap_align(w3, w2, sh);
        out[u].w = ap_align(w4, w3, sh);
      } else {
        uint8_t b[16];
        int yy = y, xx = x;
#pragma unroll
        for (int j = 0; j < 16; j++) {  // straddles a row end
          b[j] = src0[(int64_t)yy * A.src_stride + xx];
          if (++xx == rowb) {
            xx = 0;
            yy++;
          }
        }
        out[u].x = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
        out[u].y = b[4] | (b[5] << 8) | (b[6] << 16) | ((uint32_t)b[7] << 24);
        out[u].z = b[8] | (b[9] << 8) | (b[10] << 16) | ((uint32_t)b[11] << 24);
        out[u].w = b[12] | (b[13] << 8) | (b[14] << 16) | ((uint32_t)b[15] << 24);
      }
    }
#pragma unroll
    for (int u = 0; u < kApplyU; u++) {
      const int64_t k = k0 + u * cs;
      if (k >= nchunk) break;
      *reinterpret_cast<uint4 *>(A.dst + head + 16 * k) = out[u];
    }
  }
}
__global__ __launch_bounds__(256) void k_crop_apply3(const ApplyDesc *__restrict__ descs,
                                                     const DevCrop *__restrict__ crops,
                                                     const ScResult *__restrict__ results) {
  crop_apply_item(descs, crops, results, blockIdx.y, blockIdx.x, gridDim.x);
}
// the same work from one workgroup per CU walking the (image, part) items: runs
// beside the next batch's persistent resample (no LDS, few VGPRs: it fits next
// to a 16-wave k_rs_vr workgroup, so neither kernel waits for the other's CUs)
__global__ __launch_bounds__(256, 8) void k_crop_apply3p(const ApplyDesc *__restrict__ descs,
                                                      const DevCrop *__restrict__ crops,
                                                      const ScResult *__restrict__ results, int n) {
  for (int item = blockIdx.x; item < n * kApplyChunks; item += gridDim.x)
    crop_apply_item(descs, crops, results, item / kApplyChunks, item % kApplyChunks, kApplyChunks);
}

int launch_crop_apply(hipStream_t s, const ApplyDesc *descs, int n, const DevCrop *crops, const ScResult *results,
                      int persistent_wgs) {
  if (n <= 0) return 0;
  if (persistent_wgs > 0)
    hipLaunchKernelGGL(k_crop_apply3p, dim3(min(persistent_wgs, n * kApplyChunks)), dim3(256), 0, s, descs, crops,
                       results, n);
  else
    hipLaunchKernelGGL(k_crop_apply3, dim3(kApplyChunks, n), dim3(256), 0, s, descs, crops, results);
  return 0;
}

}  // namespace fi
