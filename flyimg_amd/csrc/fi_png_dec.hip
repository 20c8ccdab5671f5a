// fi_png_dec.hip -- PNG decode on the GPU (opt-in): 8-bit non-interlaced
// sources of colour type 0 / 2 / 3 / 4 / 6 go from file bytes to pixels in the
// caller's device buffers.  The host (fi_png_parse.cpp) walks the chunks and
// joins the IDAT payloads; one upload carries the batch.  An image's deflate
// stream is one serial chain, as a JPEG scan is: the batch supplies the
// parallelism.
//
//   k_png_inflate   a 64-lane workgroup per image runs png_inflate
//            (fi_png_dec.h, the function the CPU tests run) in wave-uniform
//            control flow: the payload comes through a 512-byte window held
//            in two registers per lane, the primary decode tables sit in eight
//            more (an entry is one cross-lane read: no memory latency on the
//            symbol chain), the tables' long-code part and the 32 KiB window (a
//            ring) in LDS, so a back-reference never reads global memory this
//            kernel has just written; the lanes share a table's
//            fill, a stored block's and a match's bytes (byte i from i % dist)
//            and the ring's flushes into the image's filtered stream;
//   k_png_adler     a workgroup per image: Adler-32 partial sums per 64 KiB
//            segment, combined (png_adler_append), against the stream's trailer;
//   k_png_unfilter  a wave per image, the rows as a wavefront: lane l takes row
//            y0 + l of a 64-row band one pixel behind lane l - 1, whose pixel
//            above (b) arrives by a cross-lane move and stays one step as the
//            pixel above left (c); the band's last row goes to a carry row in
//            global memory that lane 0 of the next band reads behind a fence
//            (two carry rows alternate); the stores expand to the output
//            channels (gray replication, palette / tRNS lookup from LDS, alpha
//            fill).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fi_internal.h"
#define FI_PNG_WAVE 1
#include "fi_png_dec.h"

namespace fi {

struct PngDecDesc {     // one image of a decode batch
  uint8_t *dst;         // HWC u8 rows, outc channels
  int64_t dst_stride;
  int64_t in0;          // its zlib stream in the upload (16-byte aligned, readable to the next multiple of 16)
  int64_t stream0;      // its filtered stream in the work buffer (256-byte aligned)
  int64_t carry0;       // its two carry rows, carry_pitch apart
  uint32_t in_len;      // bytes of the zlib stream
  uint32_t nbytes;      // bytes of the filtered stream, H * (W * bpp + 1)
  uint32_t cap;         // bytes of its slot in the work buffer
  int32_t carry_pitch;
  int32_t W, H, bpp, outc;
  int32_t pal;          // index of its palette in the upload, -1: none
  int32_t pad_;
};

// The payload through two registers per lane -- 256 bytes each across the
// wave, the window and the one behind it (as BitReader, fi_jpeg.hip): a word
// of the stream is two cross-lane reads, no memory latency on the symbol chain.
// Wave-uniform calls only.
struct PngRegIn {
  const uint8_t *g;
  uint32_t n, n16;   // payload bytes; readable bytes (the upload pads to 16)
  uint32_t win, nxt;
  uint32_t wbase;    // multiple of 256
  __device__ __forceinline__ uint32_t load(uint32_t off) const {
    const uint32_t o = off + 4u * threadIdx.x;
    return (off < n16 && o < n16) ? *reinterpret_cast<const uint32_t *>(g + o) : 0u;
  }
  __device__ __forceinline__ uint32_t word(uint32_t pos) {
    if (pos - wbase >= 256u) {
      if (pos - wbase < 512u) {
        win = nxt;
        wbase += 256u;
      } else {  // the start, or behind a stored block
        wbase = pos & ~255u;
        win = load(wbase);
      }
      nxt = load(wbase + 256u);
    }
    const uint32_t o = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pos - wbase)), k = o >> 2;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)win, (int)k);
    const uint32_t hi = k < 63u ? (uint32_t)__builtin_amdgcn_readlane((int)win, (int)(k + 1u))
                                : (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt);
    uint32_t w = (uint32_t)(((uint64_t)hi << 32 | lo) >> (8u * (o & 3u)));
    if (pos + 4u > n) w = pos >= n ? 0u : w & ((1u << (8u * (n - pos))) - 1u);  // zeros behind the payload
    return w;
  }
};

// The primary lit/len and distance tables in registers: 512 u16 entries are
// 256 dwords, four per lane; an entry is one cross-lane read.
struct PngRegLook {
  uint32_t l[4], d[4];
  PngWalk lw, dw;
  __device__ __forceinline__ void load(const PngDecTabs *T, int lane) {
    lw = png_walk_init(T->lcount);
    dw = png_walk_init(T->dcount);
    const uint32_t *lw = reinterpret_cast<const uint32_t *>(T->lprim);
    const uint32_t *dw = reinterpret_cast<const uint32_t *>(T->dprim);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      l[r] = lw[64 * r + lane];
      d[r] = dw[64 * r + lane];
    }
  }
  static __device__ __forceinline__ uint32_t pick(const uint32_t (&t)[4], uint32_t i) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i >> 1)), ln = w & 63u, r = w >> 6;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)t[0], (int)ln);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)t[1], (int)ln);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)t[2], (int)ln);
    const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)t[3], (int)ln);
    const uint32_t v = r == 0 ? a : r == 1 ? b : r == 2 ? c : e;
    return (i & 1u) ? v >> 16 : v & 0xFFFFu;
  }
  __device__ __forceinline__ uint32_t lprim(uint32_t i) const { return pick(l, i); }
  __device__ __forceinline__ uint32_t dprim(uint32_t i) const { return pick(d, i); }
};

// state[2 i] = the image's PngDecErr (0: good so far), state[2 i + 1] = its Adler-32 trailer
__global__ __launch_bounds__(64) void k_png_inflate(const PngDecDesc *__restrict__ descs, int nd,
                                                    const uint8_t *__restrict__ upload, uint8_t *__restrict__ work,
                                                    uint32_t *__restrict__ state) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[kPngRing];
  __shared__ PngDecTabs T;
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= nd) return;
  const PngDecDesc &D = descs[img];
  const uint8_t *raw = upload + D.in0;
  PngRegIn in{raw, D.in_len, (D.in_len + 15u) & ~15u, 0u, 0u, 0x80000000u};
  PngRegLook look;
  uint32_t trailer = 0;
  const int err = png_inflate(in, look, raw, D.in_len, ring, &T, work + D.stream0, D.cap, D.nbytes, &trailer, lane, 64);
  if (lane == 0) {
    state[2 * img] = (uint32_t)err;
    state[2 * img + 1] = trailer;
  }
}

constexpr uint32_t kPngAdlerSeg = 65536;

__global__ __launch_bounds__(256) void k_png_adler(const PngDecDesc *__restrict__ descs, int nd,
                                                   const uint8_t *__restrict__ work, uint32_t *__restrict__ state) {
  __shared__ uint32_t ra[4], rb[4];
  const int img = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (img >= nd || state[2 * img]) return;
  const PngDecDesc &D = descs[img];
  const uint8_t *d = work + D.stream0;
  const uint32_t n = D.nbytes;
  uint32_t a = 1, b = 0;
  for (uint32_t s0 = 0; s0 < n; s0 += kPngAdlerSeg) {
    const uint32_t m = n - s0 < kPngAdlerSeg ? n - s0 : kPngAdlerSeg;
    uint64_t sa = 0, sb = 0;
    for (uint32_t i = (uint32_t)t * 16u; i < m; i += 256u * 16u) {
      uint32_t w[4] = {0, 0, 0, 0};
      if (i + 16u <= m) {
        const uint4 v = *reinterpret_cast<const uint4 *>(d + s0 + i);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else {
        for (uint32_t j = 0; i + j < m; j++) w[j >> 2] |= (uint32_t)d[s0 + i + j] << (8 * (j & 3));
      }
#pragma unroll
      for (uint32_t j = 0; j < 16; j++) {
        const uint32_t v = (w[j >> 2] >> (8 * (j & 3))) & 255u;  // (0 behind m)
        sa += v;
        if (i + j < m) sb += (uint64_t)v * (m - i - j);
      }
    }
    uint32_t pa = (uint32_t)(sa % 65521u), pb = (uint32_t)(sb % 65521u);
#pragma unroll
    for (int k = 32; k; k >>= 1) {
      pa += __shfl_xor(pa, k, 64);
      pb += __shfl_xor(pb, k, 64);
    }
    __syncthreads();
    if (lane == 0) {
      ra[wave] = pa;
      rb[wave] = pb;
    }
    __syncthreads();
    png_adler_append(&a, &b, (ra[0] + ra[1] + ra[2] + ra[3]) % 65521u, (rb[0] + rb[1] + rb[2] + rb[3]) % 65521u, m);
  }
  if (t == 0 && ((b << 16) | a) != state[2 * img + 1]) state[2 * img] = kPngErrAdler;
}

__device__ __forceinline__ uint32_t png_load_px(const uint8_t *p, int bpp) {
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (j < bpp) v |= (uint32_t)p[j] << (8 * j);
  return v;
}

constexpr int kPngStepChunk = 16;  // wavefront steps per group of loads

__global__ __launch_bounds__(64) void k_png_unfilter(const PngDecDesc *__restrict__ descs, int nd,
                                                     const uint32_t *__restrict__ pals, uint8_t *__restrict__ work,
                                                     uint32_t *__restrict__ state) {
  __shared__ uint32_t pal[256];
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= nd || state[2 * img]) return;
  const PngDecDesc &D = descs[img];
  const int W = D.W, H = D.H, bpp = D.bpp, outc = D.outc;
  const bool paletted = D.pal >= 0;
  if (paletted) {
    for (int i = lane; i < 256; i += 64) pal[i] = pals[(int64_t)D.pal * 256 + i];
  }
  __syncthreads();
  const uint8_t *stream = work + D.stream0;
  const int64_t rowlen = (int64_t)W * bpp + 1;
  bool bad = false;
  for (int y0 = 0, band = 0; y0 < H; y0 += 64, band++) {
    const int y = y0 + lane;
    const bool active = y < H;
    const int lastlane = std::min(64, H - y0) - 1;
    const bool more = y0 + 64 < H;  // the band's last row is the next band's row above
    const uint8_t *row = stream + (int64_t)(active ? y : 0) * rowlen;
    const uint8_t *cin = work + D.carry0 + (int64_t)(band & 1) * D.carry_pitch;
    uint8_t *cout = work + D.carry0 + (int64_t)((band + 1) & 1) * D.carry_pitch;
    uint8_t *orow = D.dst + (int64_t)(active ? y : 0) * D.dst_stride;
    int ft = active ? row[0] : 0;
    if (ft > 4) {
      bad = true;
      ft = 0;
    }
    uint32_t cur = 0, bprev = 0;  // this lane's last pixel (a), the last pixel above (c)
    for (int s0 = 0; s0 < W + lastlane; s0 += kPngStepChunk) {
      uint32_t raw[kPngStepChunk], up[kPngStepChunk];
#pragma unroll
      for (int k = 0; k < kPngStepChunk; k++) {
        const int x = s0 + k - lane;
        raw[k] = (active && x >= 0 && x < W) ? png_load_px(row + 1 + (int64_t)x * bpp, bpp) : 0u;
        up[k] = (lane == 0 && y0 > 0 && x < W) ? png_load_px(cin + (int64_t)x * bpp, bpp) : 0u;
      }
#pragma unroll
      for (int k = 0; k < kPngStepChunk; k++) {
        const int x = s0 + k - lane;
        const uint32_t above = __shfl_up(cur, 1, 64);  // lane l - 1 finished this x one step ago
        const uint32_t bb = lane == 0 ? up[k] : above;
        const uint32_t aa = x > 0 ? cur : 0u, cc = x > 0 ? bprev : 0u;
        uint32_t r = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (j < bpp)
            r |= (uint32_t)png_dec_recon(ft, (int)((raw[k] >> (8 * j)) & 255u), (int)((aa >> (8 * j)) & 255u),
                                         (int)((bb >> (8 * j)) & 255u), (int)((cc >> (8 * j)) & 255u))
                 << (8 * j);
        bprev = bb;
        cur = r;
        if (active && x >= 0 && x < W) {
          if (more && lane == lastlane) {
            uint8_t *c = cout + (int64_t)x * bpp;
#pragma unroll
            for (int j = 0; j < 4; j++)
              if (j < bpp) c[j] = (uint8_t)(r >> (8 * j));
          }
          // source pixel -> output channels
          uint32_t o = r;
          if (paletted) {
            o = pal[r & 255u];
          } else if (bpp == 1) {
            o = (r & 255u) * 0x010101u | 0xFF000000u;
          } else if (bpp == 2) {
            o = outc == 2 ? r : ((r & 255u) * 0x010101u | ((r >> 8) << 24));
          } else if (bpp == 3) {
            o = r | 0xFF000000u;
          }
          uint8_t *q = orow + (int64_t)x * outc;
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (j < outc) q[j] = (uint8_t)(o >> (8 * j));
        }
      }
    }
    if (more) {  // the carry row is read by another lane than the one that wrote it
      __threadfence();
      __syncthreads();
    }
  }
  if (__any(bad) && lane == 0) state[2 * img] = kPngErrFilter;
}

// ---------------------------------------------------------------------------
// host: batch plan + launches (`alloc` / `stage` as in jpeg_decode_batch)
// ---------------------------------------------------------------------------
int png_decode_batch(hipStream_t st, const uint8_t *const *data, const size_t *len, int n, uint8_t *const *dst,
                     const int64_t *dst_stride, const int32_t *out_channels, int32_t *status,
                     void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *), void *actx,
                     std::string *err) {
  std::vector<PngDecDesc> descs;
  std::vector<PngSrc> srcs;
  std::vector<int> desc_img;
  auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t in_total = 0, stream_total = 0, carry_total = 0;
  int npal = 0;
  for (int i = 0; i < n; i++) {
    PngSrc S;
    status[i] = data[i] ? png_parse(data[i], len[i], &S) : FI_EINVAL;
    if (status[i]) continue;
    int outc = 0;
    status[i] = png_out_channels(S, out_channels ? out_channels[i] : 0, &outc);
    if (!status[i] && (!dst[i] || dst_stride[i] < (int64_t)S.w * outc)) status[i] = FI_EINVAL;
    if (status[i]) continue;
    PngDecDesc D{};
    D.dst = dst[i];
    D.dst_stride = dst_stride[i];
    D.in0 = (int64_t)in_total;
    D.in_len = (uint32_t)S.zbytes;
    D.nbytes = (uint32_t)((int64_t)S.h * ((int64_t)S.w * S.bpp + 1));
    D.cap = (uint32_t)std::min<size_t>(up256((size_t)D.nbytes + 16), 0xFFFFFF00u);
    D.stream0 = (int64_t)stream_total;
    D.carry_pitch = (int32_t)up256((size_t)S.w * S.bpp);
    D.carry0 = (int64_t)carry_total;
    D.W = S.w;
    D.H = S.h;
    D.bpp = S.bpp;
    D.outc = outc;
    D.pal = S.palette ? npal++ : -1;
    in_total += up256(S.zbytes + 16);
    stream_total += D.cap;
    carry_total += 2 * (size_t)D.carry_pitch;
    descs.push_back(D);
    srcs.push_back(std::move(S));
    desc_img.push_back(i);
  }
  if (descs.empty()) return 0;
  const int nd = (int)descs.size();
  // upload: descriptors, palettes, zlib streams;  work: states, filtered streams, carry rows
  const size_t o_desc = 0, o_pal = o_desc + up256(descs.size() * sizeof(PngDecDesc));
  const size_t o_in = o_pal + up256((size_t)npal * 1024);
  const size_t up_total = o_in + in_total;
  const size_t k_state = 0, k_stream = k_state + up256((size_t)nd * 8);
  const size_t k_carry = k_stream + stream_total;
  const size_t work_total = k_carry + carry_total + 256;
  uint8_t *dup = (uint8_t *)alloc(actx, 0, up_total);
  uint8_t *hst = (uint8_t *)alloc(actx, 3, up_total);
  uint8_t *dwork = (uint8_t *)alloc(actx, 1, work_total);
  if (!dup || !hst || !dwork) {
    *err = "memory for the PNG decode batch";
    return FI_ENOMEM;
  }
  for (int k = 0; k < nd; k++) {
    PngDecDesc &D = descs[k];
    D.in0 += (int64_t)o_in;
    D.stream0 += (int64_t)k_stream;
    D.carry0 += (int64_t)k_carry;
    if (D.pal >= 0) memcpy(hst + o_pal + (size_t)D.pal * 1024, srcs[k].pal, 1024);
    png_copy_zstream(data[desc_img[k]], srcs[k], hst + D.in0);
  }
  memcpy(hst + o_desc, descs.data(), descs.size() * sizeof(PngDecDesc));
  uint32_t *dstate = (uint32_t *)(dwork + k_state);
  if (hipMemcpyAsync(dup, hst, up_total, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(dstate, 0, (size_t)nd * 8, st) != hipSuccess) {
    *err = "PNG decode batch upload";
    return FI_EDEVICE;
  }
  const PngDecDesc *dd = (const PngDecDesc *)(dup + o_desc);
  stage(actx, "k_png_inflate");
  hipLaunchKernelGGL(k_png_inflate, dim3((unsigned)nd), dim3(64), 0, st, dd, nd, dup, dwork, dstate);
  stage(actx, "k_png_adler");
  hipLaunchKernelGGL(k_png_adler, dim3((unsigned)nd), dim3(256), 0, st, dd, nd, dwork, dstate);
  stage(actx, "k_png_unfilter");
  hipLaunchKernelGGL(k_png_unfilter, dim3((unsigned)nd), dim3(64), 0, st, dd, nd, (const uint32_t *)(dup + o_pal),
                     dwork, dstate);
  stage(actx, nullptr);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(hst, dstate, (size_t)nd * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    *err = "PNG decode kernels";
    return FI_EDEVICE;
  }
  for (int k = 0; k < nd; k++) {
    uint32_t e = 0;
    memcpy(&e, hst + (size_t)k * 8, 4);
    if (e) status[desc_img[k]] = FI_EINVAL;
  }
  return 0;
}
}  // namespace fi
