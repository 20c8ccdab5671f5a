// fi_enc_batch.h -- the host half of what the *_encode_batch functions of the
// GPU encoders (fi_jpeg_enc.hip, fi_jpeg_penc.hip, fi_png_enc.hip,
// fi_webp_enc.hip) share: the layout of their device arenas, the per-image
// argument check, and the tail that fetches the packed stream and hands every
// caller its file.  Plain host C++ (tests/native/enc_batch_driver.cpp builds it
// alone); only enc_finish, inside __HIPCC__, talks to the device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/flyimg_hip.h"

namespace fi {

// Offsets of consecutive regions, each starting on a 256-byte boundary.
class EncArena {
 public:
  size_t add(size_t bytes) {  // the offset of a region of `bytes`
    const size_t at = end_;
    end_ += (bytes + 255) & ~(size_t)255;
    return at;
  }
  size_t total() const { return end_; }

 private:
  size_t end_ = 0;
};

// Status of image i before any work: the codec's own check, then what every
// encoder asks of the source and the output buffer.
inline int enc_io_status(int codec_check_rc, const void *src, int64_t stride, int w, int c, const void *out,
                         size_t out_cap) {
  if (codec_check_rc) return codec_check_rc;
  return !src || stride < (int64_t)w * c || (out_cap && !out) ? FI_EINVAL : 0;
}

// Hands out the files of the batch's nd accepted images: file k (image
// desc_img[k] of the call) is staged[pos[2 k], pos[2 k + 1]).  A file longer
// than its buffer gets FI_ENOMEM and its true length; nothing is written past
// out_cap, and of the file itself the first out_cap bytes
// (copy_prefix_when_short) or nothing at all.
inline void enc_deliver(const int64_t *pos, int nd, const int *desc_img, const uint8_t *staged, uint8_t *const *out,
                        const size_t *out_cap, size_t *out_len, int32_t *status, bool copy_prefix_when_short) {
  for (int k = 0; k < nd; k++) {
    const int i = desc_img[k];
    const size_t len = (size_t)(pos[2 * k + 1] - pos[2 * k]);
    out_len[i] = len;
    if (len > out_cap[i]) {
      status[i] = FI_ENOMEM;
      if (copy_prefix_when_short && out_cap[i]) memcpy(out[i], staged + pos[2 * k], out_cap[i]);
      continue;
    }
    memcpy(out[i], staged + pos[2 * k], len);
  }
}

#ifdef __HIPCC__
// The end of every *_encode_batch, after its last launch: fetches the image
// positions dpos[2 nd] (with fault_msg: and the fault word the kernels set
// behind them), then exactly the packed bytes of dpack, and delivers them.
// `hst` is the pinned buffer of the upload (>= 16 nd + 16 bytes), `limit` the
// most the batch can have packed, `codec` the name in the messages.
inline int enc_finish(hipStream_t st, void *(*alloc)(void *, int, size_t), void *actx, uint8_t *hst,
                      const int64_t *dpos, int nd, const char *fault_msg, const uint8_t *dpack, size_t limit,
                      const char *codec, const std::vector<int> &desc_img, uint8_t *const *out, const size_t *out_cap,
                      size_t *out_len, int32_t *status, bool copy_prefix_when_short, std::string *err) {
  const std::string name = codec;
  const size_t pos_bytes = (size_t)nd * 16;
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(hst, dpos, pos_bytes + (fault_msg ? 16 : 0), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    *err = name + " encode kernels";
    return FI_EDEVICE;
  }
  std::vector<int64_t> pos((size_t)nd * 2);
  memcpy(pos.data(), hst, pos_bytes);
  int32_t fault = 0;
  if (fault_msg) memcpy(&fault, hst + pos_bytes, 4);
  if (fault) {
    *err = fault_msg;
    return FI_EDEVICE;
  }
  const int64_t total = pos[2 * (size_t)nd - 1];
  if (total < 0 || (size_t)total > limit) {
    *err = name + " encode: packed size out of range";
    return FI_EDEVICE;
  }
  hst = (uint8_t *)alloc(actx, 3, (size_t)total);
  if (!hst) {
    *err = "pinned memory for the " + name + " encode download";
    return FI_ENOMEM;
  }
  if (hipMemcpyAsync(hst, dpack, (size_t)total, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    *err = name + " encode download";
    return FI_EDEVICE;
  }
  enc_deliver(pos.data(), nd, desc_img.data(), hst, out, out_cap, out_len, status, copy_prefix_when_short);
  return 0;
}
#endif

}  // namespace fi
