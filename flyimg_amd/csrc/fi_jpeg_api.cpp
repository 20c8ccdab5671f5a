// fi_jpeg_api.cpp -- the GPU codec entry points of the runtime (fi_runtime.h): JPEG decode, baseline and
// progressive JPEG encode, PNG encode and decode, lossless WebP encode.  The codecs are fi_jpeg.hip, fi_jpeg_enc.hip,
// fi_jpeg_penc.hip, fi_png_enc.hip, fi_webp_enc.hip, fi_png_dec.hip and their host halves; what every device entry
// point does around its batch (device, lock, order, timers, the first failing image) is codec_call, once.
#include "fi_runtime.h"
#include "fi_jpeg.h"
#include "fi_jpeg_enc.h"
#include "fi_png_enc.h"
#include "fi_webp_enc.h"
#include "fi_png_dec.h"

using namespace fi;

// The `alloc` of the codec batches (see jpeg_encode_batch) on the context's
// buffers: the encoders' set (ENC) or the decoders'.
template <bool ENC>
static void *codec_alloc(void *actx, int which, size_t bytes) {
  fi_ctx *c = static_cast<fi_ctx *>(actx);
  if (which == 3) {  // pinned host staging (no copy of an earlier request is in flight: the batches synchronise)
    void **host = ENC ? &c->jpeg_enc_host : &c->jpeg_host;
    return ensure_pinned_buf(host, ENC ? &c->jpeg_enc_host_cap : &c->jpeg_host_cap, bytes) == FI_OK ? *host : nullptr;
  }
  DevBuf *b = &(ENC ? c->jpeg_enc : c->jpeg)[which];
  return ensure(c, b, bytes) == FI_OK ? b->p : nullptr;
}
static void codec_stage(void *actx, const char *name) {  // ends the running kernel's range, starts `name`'s
  fi_ctx *c = static_cast<fi_ctx *>(actx);
  delete c->jpeg_enc_timer;
  c->jpeg_enc_timer = name ? new Timer(c, name, 0) : nullptr;
}
// One codec batch of n > 0 images on the context's stream, under its lock and
// behind fi_apply: `run(&err)` is the batch (its kernels timed through
// codec_stage); then the first image it turned down, if any, is the call's
// error, with `what(status)` as its message.
template <typename Run, typename What>
static int codec_call(fi_ctx *c, int32_t n, const int32_t *status, Run run, What what) {
  HIP_TRY(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  if (order_after_apply(c) != FI_OK) return set_err(FI_EDEVICE, "hipStreamWaitEvent failed");
  std::string err;
  const int rc = run(&err);
  codec_stage(c, nullptr);
  collect_timers(c);
  if (rc) return set_err(rc, "%s", err.c_str());
  for (int i = 0; i < n; i++)  // the others are done
    if (status[i]) return set_err(status[i], "image %d: %s", i, what(status[i]));
  return FI_OK;
}

extern "C" {

// GPU JPEG decode (fi_jpeg.hip): the decode half of the host codec pipeline
// (ImageProcessor's `convert` reads the source with libjpeg) on the device
int fi_jpeg_info_ex(const uint8_t *data, size_t len, uint32_t flags, int32_t *w, int32_t *h, int32_t *channels,
                    int32_t *nscans, int32_t *nlevels) {
  if (!data || !w || !h || !channels || (flags & ~FI_JPEG_PROGRESSIVE)) return set_err(FI_EINVAL, "bad arguments");
  int W = 0, H = 0, C = 0, NS = 0, NL = 0;
  const int rc = jpeg_info_ex(data, len, flags, &W, &H, &C, &NS, &NL);
  if (rc) return set_err(rc, rc == FI_EUNSUPPORTED ? "JPEG stream the GPU decoder does not handle" : "malformed JPEG");
  *w = W;
  *h = H;
  *channels = C;
  if (nscans) *nscans = NS;
  if (nlevels) *nlevels = NL;
  return FI_OK;
}
int fi_jpeg_info(const uint8_t *data, size_t len, int32_t *w, int32_t *h, int32_t *channels) {
  return fi_jpeg_info_ex(data, len, 0, w, h, channels, nullptr, nullptr);
}
int fi_jpeg_orientation(const uint8_t *data, size_t len, int32_t *orientation) {
  if (!data || !orientation) return set_err(FI_EINVAL, "bad arguments");
  int o = 1;
  const int rc = jpeg_orientation(data, len, &o);
  if (rc)
    return set_err(rc, rc == FI_EUNSUPPORTED ? "EXIF orientation to be read on the host" : "not a JPEG");
  *orientation = o;
  return FI_OK;
}
int fi_jpeg_decode_device_view(fi_ctx *c, const uint8_t *const *data, const size_t *len, int32_t n, uint8_t *const *dst,
                               const int64_t *dst_stride, int32_t out_channels, uint32_t flags,
                               const fi_jpeg_view *views, int32_t *status) {
  if (!c || n < 0 || (n > 0 && (!data || !len || !dst || !dst_stride || !status)) ||
      (out_channels != 0 && out_channels != 3) || (flags & ~FI_JPEG_PROGRESSIVE))
    return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  return codec_call(
      c, n, status,
      [&](std::string *err) {
        return jpeg_decode_batch(c->stream, data, len, n, dst, dst_stride, out_channels, flags, views, status,
                                 codec_alloc<false>, codec_stage, c, err);
      },
      [](int s) {  // the caller decodes these on the host
        return s == FI_EUNSUPPORTED ? "JPEG stream or EXIF orientation the GPU decoder does not handle"
                                    : "malformed JPEG or bad view";
      });
}
int fi_jpeg_decode_device_ex(fi_ctx *c, const uint8_t *const *data, const size_t *len, int32_t n, uint8_t *const *dst,
                             const int64_t *dst_stride, int32_t out_channels, uint32_t flags, int32_t *status) {
  return fi_jpeg_decode_device_view(c, data, len, n, dst, dst_stride, out_channels, flags, nullptr, status);
}
int fi_jpeg_decode_device(fi_ctx *c, const uint8_t *const *data, const size_t *len, int32_t n, uint8_t *const *dst,
                          const int64_t *dst_stride, int32_t out_channels, int32_t *status) {
  return fi_jpeg_decode_device_ex(c, data, len, n, dst, dst_stride, out_channels, 0, status);
}
// Test hook: a progressive stream's coefficients from the host decoder
// (fi_jpeg_prog_host.cpp): info = {components, bw[3], bh[3]}; qt = the quant
// table of each component, natural order; coefs (may be NULL: sizes only) =
// the zigzag int16 blocks of component 0, 1, 2, [bh][bw][64] each
int fi_debug_jpeg_coefs_host(const uint8_t *data, size_t len, uint32_t flags, int32_t info[7], uint16_t qt[192],
                             int16_t *coefs, size_t coefs_cap) {
  if (!data || !info || !qt) return set_err(FI_EINVAL, "bad arguments");
  JpegHdr H;
  JpegGeom G;
  std::vector<int16_t> co;
  const int rc = jpeg_prog_coefs_host(data, len, flags, &H, &G, &co);
  if (rc) return set_err(rc, rc == FI_EUNSUPPORTED ? "not a progressive stream the decoder handles" : "malformed JPEG");
  info[0] = H.ncomp;
  for (int k = 0; k < 3; k++) {
    info[1 + k] = G.bw[k];
    info[4 + k] = G.bh[k];
    for (int z = 0; z < 64; z++) qt[64 * k + z] = k < H.ncomp ? H.qt[H.tq[k]][z] : 0;
  }
  if (coefs) {
    if (coefs_cap < co.size()) return set_err(FI_ENOMEM, "coefs_cap is below the coefficient count");
    memcpy(coefs, co.data(), co.size() * sizeof(int16_t));
  }
  return FI_OK;
}
// GPU JPEG encode (fi_jpeg_enc.hip): the write half of `convert` (IM writes the
// output with libjpeg) on the device
int fi_jpeg_encode_bound(int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling, size_t *bytes) {
  if (!bytes) return set_err(FI_EINVAL, "bad arguments");
  const int rc = jpeg_enc_bound(w, h, channels, quality, subsampling, bytes);
  if (rc)
    return set_err(rc, rc == FI_EUNSUPPORTED ? "channel count or subsampling the GPU JPEG encoder does not write"
                                             : "bad JPEG dimensions or quality");
  return FI_OK;
}
int fi_jpeg_encode_bound_ex(int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling,
                            uint32_t flags, size_t *bytes) {
  if (!bytes || (flags & ~FI_JPEG_ENC_PROGRESSIVE)) return set_err(FI_EINVAL, "bad arguments");
  if (!flags) return fi_jpeg_encode_bound(w, h, channels, quality, subsampling, bytes);
  const int rc = jpeg_penc_bound(w, h, channels, quality, subsampling, bytes);
  if (rc)
    return set_err(rc, rc == FI_EUNSUPPORTED ? "channel count or subsampling the GPU JPEG encoder does not write"
                                             : "bad JPEG dimensions or quality");
  return FI_OK;
}
// Test hook: the progressive encoder's host model (fi_jpeg_pwrite.cpp)
int fi_debug_jpeg_prog_write_host(const int16_t *coefs, size_t ncoefs, int32_t w, int32_t h, int32_t channels,
                                  int32_t quality, int32_t subsampling, uint8_t *out, size_t out_cap,
                                  size_t *out_len, int32_t *flushes) {
  if (!coefs || !out_len || !flushes || (out_cap && !out)) return set_err(FI_EINVAL, "bad arguments");
  std::vector<uint8_t> file;
  int fl = 0;
  const int rc = jpeg_penc_write(coefs, ncoefs, w, h, channels, quality, subsampling, &file, &fl);
  if (rc) return set_err(rc, "settings the progressive writer turns down, or a coefficient count that does not fit them");
  *out_len = file.size();
  *flushes = fl;
  if (file.size() > out_cap) return set_err(FI_ENOMEM, "out_cap is below the file size (out_len)");
  memcpy(out, file.data(), file.size());
  return FI_OK;
}
int fi_jpeg_encode_device(fi_ctx *c, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                          const int32_t *channels, const int64_t *src_stride, const int32_t *quality,
                          const int32_t *subsampling, int32_t n, uint8_t *const *out, const size_t *out_cap,
                          size_t *out_len, int32_t *status) {
  return fi_jpeg_encode_device_ex(c, src, w, h, channels, src_stride, quality, subsampling, n, out, out_cap, out_len,
                                  status, 0);
}
int fi_jpeg_encode_device_ex(fi_ctx *c, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                             const int32_t *channels, const int64_t *src_stride, const int32_t *quality,
                             const int32_t *subsampling, int32_t n, uint8_t *const *out, const size_t *out_cap,
                             size_t *out_len, int32_t *status, uint32_t flags) {
  if (!c || n < 0 || (flags & ~FI_JPEG_ENC_PROGRESSIVE) ||
      (n > 0 && (!src || !w || !h || !channels || !src_stride || !quality || !subsampling || !out || !out_cap ||
                 !out_len || !status)))
    return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  return codec_call(
      c, n, status,
      [&](std::string *err) {
        return (flags & FI_JPEG_ENC_PROGRESSIVE ? jpeg_pencode_batch : jpeg_encode_batch)(
            c->stream, src, w, h, channels, src_stride, quality, subsampling, n, out, out_cap, out_len, status,
            codec_alloc<true>, codec_stage, c, err);
      },
      [](int s) {
        return s == FI_EUNSUPPORTED ? "channel count or subsampling the GPU JPEG encoder does not write"
               : s == FI_ENOMEM     ? "out_cap is below the encoded size (out_len)"
                                    : "bad JPEG source, dimensions or quality";
      });
}
// GPU PNG encode (fi_png_enc.hip): the outputs JPEG cannot carry (alpha); the
// JPEG encoder's scratch, staging and timing plumbing
int fi_png_encode_bound(int32_t w, int32_t h, int32_t channels, size_t *bytes) {
  if (!bytes) return set_err(FI_EINVAL, "bad arguments");
  const int rc = png_enc_bound(w, h, channels, bytes);
  if (rc)
    return set_err(rc, rc == FI_EUNSUPPORTED ? "filtered stream beyond 2^31 - 1 bytes" : "bad PNG dimensions or channels");
  return FI_OK;
}
int fi_png_encode_device(fi_ctx *c, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                         const int32_t *channels, const int64_t *src_stride, const int32_t *filter, int32_t n,
                         uint8_t *const *out, const size_t *out_cap, size_t *out_len, int32_t *status) {
  if (!c || n < 0 || (n > 0 && (!src || !w || !h || !channels || !src_stride || !out || !out_cap || !out_len || !status)))
    return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  return codec_call(
      c, n, status,
      [&](std::string *err) {
        return png_encode_batch(c->stream, src, w, h, channels, src_stride, filter, n, out, out_cap, out_len, status,
                                codec_alloc<true>, codec_stage, c, err);
      },
      [](int s) {
        return s == FI_EUNSUPPORTED ? "filtered stream beyond 2^31 - 1 bytes"
               : s == FI_ENOMEM     ? "out_cap is below the encoded size (out_len)"
                                    : "bad PNG source, dimensions, channels or filter";
      });
}
// GPU lossless WebP encode (fi_webp_enc.hip): the PNG encoder's conventions and plumbing
int fi_webp_encode_bound(int32_t w, int32_t h, int32_t channels, size_t *bytes) {
  if (!bytes) return set_err(FI_EINVAL, "bad arguments");
  const int rc = webp_enc_bound(w, h, channels, bytes);
  if (rc) return set_err(rc, rc == FI_EUNSUPPORTED ? "a side above 16384" : "bad WebP dimensions or channels");
  return FI_OK;
}
int fi_debug_webp_encode_host(const uint8_t *src, int32_t w, int32_t h, int32_t channels, int64_t src_stride,
                              int32_t predictor, uint8_t *out, size_t out_cap, size_t *out_len) {
  if (!src || !out_len || (out_cap && !out)) return set_err(FI_EINVAL, "bad arguments");
  const int rc = webp_encode_host(src, w, h, channels, src_stride, predictor, out, out_cap, out_len);
  if (rc == FI_ENOMEM) return set_err(rc, "out_cap is below the encoded size (out_len)");
  if (rc == FI_EDEVICE) return set_err(rc, "WebP encode: the bits emitted differ from the bits priced");
  if (rc)
    return set_err(rc, rc == FI_EUNSUPPORTED ? "a side above 16384" : "bad WebP source, dimensions, channels or predictor");
  return FI_OK;
}
int fi_webp_encode_device(fi_ctx *c, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                          const int32_t *channels, const int64_t *src_stride, const int32_t *predictor, int32_t n,
                          uint8_t *const *out, const size_t *out_cap, size_t *out_len, int32_t *status) {
  if (!c || n < 0 || (n > 0 && (!src || !w || !h || !channels || !src_stride || !out || !out_cap || !out_len || !status)))
    return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  return codec_call(
      c, n, status,
      [&](std::string *err) {
        return webp_encode_batch(c->stream, src, w, h, channels, src_stride, predictor, n, out, out_cap, out_len,
                                 status, codec_alloc<true>, codec_stage, c, err);
      },
      [](int s) {
        return s == FI_EUNSUPPORTED ? "a side above 16384"
               : s == FI_ENOMEM     ? "out_cap is below the encoded size (out_len)"
                                    : "bad WebP source, dimensions, channels or predictor";
      });
}
// GPU PNG decode (fi_png_dec.hip): the sources a JPEG cannot be (alpha, palette); the JPEG
// decoder's scratch, staging and timing plumbing
int fi_png_info(const uint8_t *data, size_t len, int32_t *w, int32_t *h, int32_t *channels, int32_t *color_type,
                int32_t *meta) {
  if (!data || !w || !h || !channels) return set_err(FI_EINVAL, "bad arguments");
  PngSrc S;
  const int rc = png_parse(data, len, &S);
  if (rc) return set_err(rc, rc == FI_EUNSUPPORTED ? "PNG file the GPU decoder does not handle" : "not a PNG file");
  *w = S.w;
  *h = S.h;
  *channels = S.channels;
  if (color_type) *color_type = S.color_type;
  if (meta) *meta = S.meta;
  return FI_OK;
}
int fi_png_decode_device(fi_ctx *c, const uint8_t *const *data, const size_t *len, int32_t n, uint8_t *const *dst,
                         const int64_t *dst_stride, const int32_t *out_channels, int32_t *status) {
  if (!c || n < 0 || (n > 0 && (!data || !len || !dst || !dst_stride || !status)))
    return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  return codec_call(
      c, n, status,
      [&](std::string *err) {
        return png_decode_batch(c->stream, data, len, n, dst, dst_stride, out_channels, status, codec_alloc<false>,
                                codec_stage, c, err);
      },
      [](int s) {  // the caller decodes these on the host
        return s == FI_EUNSUPPORTED ? "PNG file the GPU decoder does not handle"
                                    : "malformed PNG, or out_channels / dst_stride that do not fit it";
      });
}

}  // extern "C"
