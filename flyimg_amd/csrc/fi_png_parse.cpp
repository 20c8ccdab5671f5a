// fi_png_parse.cpp -- host side of the GPU PNG decoder (fi_png_dec.hip): the
// chunk walk that decides whether the device path reproduces a file exactly
// (fi_png_info), PLTE / tRNS, and the IDAT payloads joined into one zlib
// stream -- chunk boundaries, empty and 1-byte IDATs disappear here.  Host C++
// only; CRC-32 from fi_png_write.cpp.
#include "fi_png_dec.h"

#include <string.h>

#include "../../include/flyimg_hip.h"

namespace fi {

static uint32_t rd32(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
static bool is_type(const uint8_t *p, const char *t) { return memcmp(p, t, 4) == 0; }

// tEXt / zTXt / iTXt: the keyword (up to the first NUL) is one Pillow's exif_transpose could
// take an orientation from
static bool orient_keyword(const uint8_t *p, size_t n) {
  static const char *const keys[3] = {"Raw profile type exif", "Raw profile type APP1", "XML:com.adobe.xmp"};
  size_t k = 0;
  while (k < n && p[k]) k++;
  if (k == n) return false;
  for (const char *key : keys)
    if (strlen(key) == k && memcmp(p, key, k) == 0) return true;
  return false;
}

int png_parse(const uint8_t *data, size_t len, PngSrc *S) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (!data || len < 8 + 25 || memcmp(data, sig, 8) != 0) return FI_EINVAL;
  const uint8_t *ih = data + 8;
  if (rd32(ih) != 13 || !is_type(ih + 4, "IHDR")) return FI_EINVAL;
  const uint32_t w = rd32(ih + 8), h = rd32(ih + 12);
  const int depth = ih[16], ct = ih[17], comp = ih[18], filt = ih[19], lace = ih[20];
  if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || comp != 0 || filt != 0 || lace > 1) return FI_EINVAL;
  const bool depth_ok = ct == 0   ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                        : ct == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                        : (ct == 2 || ct == 4 || ct == 6) ? (depth == 8 || depth == 16)
                                                          : false;
  if (!depth_ok) return FI_EINVAL;
  if (png_crc32(0, ih + 4, 17) != rd32(ih + 21)) return FI_EUNSUPPORTED;
  if (depth != 8 || lace != 0) return FI_EUNSUPPORTED;
  S->w = (int32_t)w;
  S->h = (int32_t)h;
  S->color_type = ct;
  S->palette = ct == 3;
  S->bpp = ct == 0 ? 1 : ct == 4 ? 2 : ct == 2 ? 3 : ct == 6 ? 4 : 1;
  S->channels = ct == 3 ? 3 : S->bpp;
  S->meta = 0;
  S->idat.clear();
  S->zbytes = 0;
  if ((int64_t)h * ((int64_t)w * S->bpp + 1) > 0x7FFFFFFFll) return FI_EUNSUPPORTED;
  for (int i = 0; i < 256; i++) S->pal[i] = 0xFF000000u;  // an index beyond PLTE: (0, 0, 0), alpha 255
  bool plte = false, trns = false, iend = false, idat_closed = false;
  size_t at = 8 + 25;
  while (!iend) {
    if (len - at < 12) return FI_EUNSUPPORTED;  // no IEND
    const uint32_t cl = rd32(data + at);
    const uint8_t *ty = data + at + 4;
    if (cl > 0x7FFFFFFFu || (size_t)cl > len - at - 12) return FI_EUNSUPPORTED;
    const uint8_t *body = ty + 4;
    const bool critical = !(ty[0] & 0x20);
    const bool known = is_type(ty, "PLTE") || is_type(ty, "tRNS") || is_type(ty, "IDAT") || is_type(ty, "IEND");
    if (critical && !known) return FI_EUNSUPPORTED;  // (a second IHDR among them)
    if (known && png_crc32(0, ty, (size_t)cl + 4) != rd32(body + cl)) return FI_EUNSUPPORTED;
    if (!S->idat.empty() && !is_type(ty, "IDAT")) idat_closed = true;
    if (is_type(ty, "IDAT")) {
      if (idat_closed) return FI_EUNSUPPORTED;  // IDATs apart
      S->idat.push_back({(size_t)(body - data), (size_t)cl});
      S->zbytes += cl;
    } else if (is_type(ty, "PLTE")) {
      if (plte || trns || !S->idat.empty() || cl == 0 || cl % 3 != 0 || cl > 768) return FI_EUNSUPPORTED;
      plte = true;
      for (uint32_t i = 0; i < cl / 3; i++)
        S->pal[i] = 0xFF000000u | body[3 * i] | ((uint32_t)body[3 * i + 1] << 8) | ((uint32_t)body[3 * i + 2] << 16);
    } else if (is_type(ty, "tRNS")) {
      // a colour key (types 0 and 2) is not applied here; types 4 and 6 may not carry one
      if (ct != 3 || trns || !plte || !S->idat.empty() || cl > 256) return FI_EUNSUPPORTED;
      trns = true;
      for (uint32_t i = 0; i < cl; i++) S->pal[i] = (S->pal[i] & 0x00FFFFFFu) | ((uint32_t)body[i] << 24);
    } else if (is_type(ty, "IEND")) {
      if (cl != 0) return FI_EUNSUPPORTED;
      iend = true;
    } else if (is_type(ty, "acTL")) {
      return FI_EUNSUPPORTED;
    } else if (is_type(ty, "eXIf")) {
      S->meta |= FI_PNG_META_ORIENT;
    } else if (is_type(ty, "tEXt") || is_type(ty, "zTXt") || is_type(ty, "iTXt")) {
      if (orient_keyword(body, cl)) S->meta |= FI_PNG_META_ORIENT;
    }
    at += 12 + (size_t)cl;
  }
  if (at != len) return FI_EUNSUPPORTED;  // bytes after IEND
  if (ct == 3 && !plte) return FI_EUNSUPPORTED;
  if (trns) S->channels = 4;
  if (S->idat.empty() || S->zbytes < 2 || S->zbytes > 0x7FFFFFFFu) return FI_EUNSUPPORTED;
  // the zlib header, wherever the chunk boundaries put its two bytes
  uint8_t zh[2] = {0, 0};
  int got = 0;
  for (size_t k = 0; k < S->idat.size() && got < 2; k++)
    for (size_t j = 0; j < S->idat[k].second && got < 2; j++) zh[got++] = data[S->idat[k].first + j];
  if (!png_zlib_header_ok(zh[0], zh[1])) return FI_EUNSUPPORTED;
  return FI_OK;
}

void png_copy_zstream(const uint8_t *data, const PngSrc &S, uint8_t *dst) {
  for (const auto &c : S.idat) {
    if (c.second) memcpy(dst, data + c.first, c.second);
    dst += c.second;
  }
}

int png_out_channels(const PngSrc &S, int out_channels, int *outc) {
  const bool alpha = S.channels == 2 || S.channels == 4;
  if (out_channels == 0) {
    *outc = S.channels;
  } else if (out_channels == 3) {
    if (alpha) return FI_EINVAL;
    *outc = 3;
  } else if (out_channels == 4) {
    *outc = 4;
  } else {
    return FI_EINVAL;
  }
  return FI_OK;
}

}  // namespace fi
