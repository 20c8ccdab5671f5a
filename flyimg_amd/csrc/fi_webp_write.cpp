// fi_webp_write.cpp -- host side of the GPU lossless WebP encoder
// (fi_webp_enc.hip): the argument check, the size bound and the host form of
// the encoder, which runs fi_webp_enc.h's functions with (lane, nlanes) =
// (0, 1) and writes the bytes the device writes.  Host C++ only.
#include "fi_webp_enc.h"

#include <string.h>

#include <memory>
#include <vector>

#include "../../include/flyimg_hip.h"

namespace fi {

int webp_enc_check(int w, int h, int channels, int predictor) {
  if (channels < 1 || channels > 4 || w < 1 || h < 1 || predictor < -1 || predictor > 13) return FI_EINVAL;
  if (w > kWebpMaxSide || h > kWebpMaxSide) return FI_EUNSUPPORTED;  // the header has 14 bits
  return 0;
}

int webp_fallback_hdr_bits(int channels) {
  WebpImg I{};
  I.W = I.H = 1;  // (the header's fields have fixed widths)
  I.C = channels;
  std::unique_ptr<WebpBuildWork> ws(new WebpBuildWork);
  std::vector<uint32_t> tabs(kWebpHist);
  WebpBits dry{nullptr, 0, 0, 0};
  webp_write_head(I, false, nullptr, nullptr, tabs.data(), &dry, ws.get());
  return (int)dry.pos;
}

static WebpImg webp_geometry(int w, int h, int channels, int predictor) {
  WebpImg I{};
  I.W = w;
  I.H = h;
  I.C = channels;
  I.pred = predictor;
  I.bw = (w + 15) >> kWebpBlockBits;
  I.bh = (h + 15) >> kWebpBlockBits;
  I.npix = w * h;
  I.nbands = (I.npix + kWebpBand - 1) / kWebpBand;
  I.fb_hdr = webp_fallback_hdr_bits(channels);
  return I;
}

// RIFF header, the fallback form's payload head, a byte per varying channel and
// pixel, the pad byte
int webp_enc_bound(int w, int h, int channels, size_t *bytes) {
  const int rc = webp_enc_check(w, h, channels, -1);
  if (rc) return rc;
  *bytes = (size_t)kWebpRiffBytes + (size_t)((webp_fallback_hdr_bits(channels) + 7) >> 3) + (size_t)w * h * channels + 1;
  return 0;
}

int webp_encode_host(const uint8_t *src, int w, int h, int channels, int64_t stride, int predictor, uint8_t *out,
                     size_t out_cap, size_t *out_len) {
  *out_len = 0;
  const int rc = webp_enc_check(w, h, channels, predictor);
  if (rc) return rc;
  if (!src || stride < (int64_t)w * channels) return FI_EINVAL;
  size_t bound = 0;
  (void)webp_enc_bound(w, h, channels, &bound);
  WebpImg I = webp_geometry(w, h, channels, predictor);
  I.src = src;
  I.stride = stride;
  I.slot_bytes = (int64_t)((bound + 4 + 15) & ~(size_t)15);
  const int64_t nblk = (int64_t)I.bw * I.bh;
  std::vector<uint32_t> resid((size_t)I.npix), tok((size_t)I.npix), bandhists((size_t)I.nbands * kWebpHist);
  std::vector<uint32_t> imghist(kWebpHist, 0), tabs(kWebpHist), slot((size_t)I.slot_bytes / 4 + 4, 0);
  std::vector<uint8_t> modes((size_t)nblk);
  std::vector<int32_t> ntok((size_t)I.nbands);
  std::vector<int64_t> bandoff((size_t)I.nbands);
  uint32_t cost[16];
  for (int64_t b = 0; b < nblk; b++) webp_pred_block(I, (int)b, 0, 1, cost, resid.data(), modes.data());
  std::unique_ptr<WebpLzWork> lz(new WebpLzWork);
  for (int b = 0; b < I.nbands; b++) {
    const int n = webp_min(kWebpBand, I.npix - b * kWebpBand);
    webp_lz_band(resid.data() + (size_t)b * kWebpBand, n, 0, 1, lz.get(), tok.data() + (size_t)b * kWebpBand, &ntok[b],
                 bandhists.data() + (size_t)b * kWebpHist, imghist.data());
  }
  std::unique_ptr<WebpBuildWork> ws(new WebpBuildWork);
  WebpImgOut R{};
  int32_t fault = 0;
  webp_build_image(I, imghist.data(), modes.data(), bandhists.data(), 0, 1, ws.get(), tabs.data(), bandoff.data(),
                   slot.data(), &R, &fault);
  if (fault) return FI_EDEVICE;
  // the tokens, band by band, at the bit offsets the image was priced with
  WebpBits bw{slot.data() + kWebpRiffBytes / 4, 0, (I.slot_bytes - kWebpRiffBytes) * 8, 0};
  for (int b = 0; b < I.nbands; b++) {
    const int n = webp_min(kWebpBand, I.npix - b * kWebpBand);
    const int nt = R.fallback ? n : ntok[b];
    bw.pos = bandoff[b];
    for (int i = 0; i < nt; i++) {
      const uint32_t t = R.fallback ? (uint32_t)i : tok[(size_t)b * kWebpBand + i];
      uint32_t argb = 0;
      if (!(t & 0x80000000u)) {
        const int64_t p = (int64_t)b * kWebpBand + t;
        argb = R.fallback ? webp_px(I, (int)(p % I.W), (int)(p / I.W), I.C <= 2) : resid[(size_t)p];
      }
      uint64_t v;
      const int nb = webp_token_bits(t, argb, tabs.data(), &v);  // at most 60 bits
      enc_put(&bw, (uint32_t)v, webp_min(nb, 32));
      if (nb > 32) enc_put(&bw, (uint32_t)(v >> 32), nb - 32);
      if (bw.over) return FI_EDEVICE;
    }
    if (bw.pos != (b + 1 < I.nbands ? bandoff[b + 1] : R.total_bits)) return FI_EDEVICE;
  }
  *out_len = (size_t)R.file_bytes;
  if ((size_t)R.file_bytes > out_cap) return FI_ENOMEM;
  memcpy(out, slot.data(), (size_t)R.file_bytes);  // (the words are little endian, as the device's)
  return 0;
}

}  // namespace fi
