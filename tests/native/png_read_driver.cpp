// Stand-alone driver of the GPU PNG decoder's host half (fi_png_parse.cpp) and
// of the inflater that host and device share (fi_png_dec.h), built under
// ASan/UBSan by tests/test_png_decode_cpu.py.  The inflater runs exactly as the
// device runs it, with one lane instead of 64: through the 32 KiB ring, with
// the flushes, into a buffer of exactly the expected size (heap memory, so a
// store past it is a sanitizer report).  One command per stdin line, one answer
// line each:
//   info HEX         -> "INFO <rc> <w> <h> <channels> <colour type> <meta>"
//   inflate N HEX    -> "INF <PngDecErr> <hex of the N bytes, when 0>": the zlib stream HEX, N bytes expected;
//                       the Adler-32 is compared as k_png_adler does (segments, combined)
//   file HEX         -> "FILE <status>": fi_png_info's answer, or what fi_png_decode_device answers for the file:
//                       parse, join the IDATs, inflate, Adler-32, filter bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../flyimg_amd/csrc/fi_png_dec.h"
#include "../../include/flyimg_hip.h"

using namespace fi;

static std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  v.reserve(s.size() / 2);
  auto nib = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)(nib(s[i]) * 16 + nib(s[i + 1])));
  return v;
}

// 0 or a PngDecErr; out = the inflated bytes
static int inflate_checked(const std::vector<uint8_t> &z, uint32_t expect, std::vector<uint8_t> *out) {
  std::vector<uint32_t> ring(kPngRing / 4), buf((expect + 3) / 4 + 1);
  // the payload in a buffer of its own size: a read past it is a report
  uint8_t *raw = (uint8_t *)malloc(z.size() ? z.size() : 1);
  if (z.size()) memcpy(raw, z.data(), z.size());
  PngDecTabs *T = new PngDecTabs;
  memset(T, 0, sizeof(*T));
  uint32_t trailer = 0;
  // (cap = expect: the word buffer's slack is never stored to)
  int err = png_inflate(PngHostIn{raw, (uint32_t)z.size()}, PngHostLook{T}, raw, (uint32_t)z.size(), (uint8_t *)ring.data(), T,
                        (uint8_t *)buf.data(), expect, expect, &trailer, 0, 1);
  const uint8_t *o = (const uint8_t *)buf.data();
  if (!err && png_dec_adler(o, expect, 65536) != trailer) err = kPngErrAdler;
  if (!err && png_dec_adler(o, expect, 7) != trailer) err = kPngErrAdler;  // (any segment size combines alike)
  if (!err) out->assign(o, o + expect);
  delete T;
  free(raw);
  return err;
}

int main() {
  char *line = nullptr;
  size_t cap = 0;
  int done = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::istringstream in(line);
    std::string cmd, hx;
    in >> cmd;
    if (cmd == "info") {
      in >> hx;
      const std::vector<uint8_t> f = unhex(hx);
      PngSrc S;
      const int rc = png_parse(f.data(), f.size(), &S);
      printf("INFO %d %d %d %d %d %d\n", rc, rc ? 0 : S.w, rc ? 0 : S.h, rc ? 0 : S.channels, rc ? 0 : S.color_type,
             rc == FI_EINVAL ? 0 : S.meta);
    } else if (cmd == "inflate") {
      uint32_t expect = 0;
      in >> expect >> hx;
      const std::vector<uint8_t> z = unhex(hx);
      std::vector<uint8_t> out;
      // (fi_png_info turns down a header zlib would refuse before the device sees the stream)
      const int err = z.size() < 2 || !png_zlib_header_ok(z[0], z[1]) ? (int)kPngErrInput : inflate_checked(z, expect, &out);
      printf("INF %d ", err);
      for (uint8_t v : out) printf("%02x", v);
      printf("\n");
    } else if (cmd == "file") {
      in >> hx;
      const std::vector<uint8_t> f = unhex(hx);
      PngSrc S;
      int st = png_parse(f.data(), f.size(), &S);
      if (!st) {
        std::vector<uint8_t> z(S.zbytes), px;
        png_copy_zstream(f.data(), S, z.data());
        const uint32_t rowlen = (uint32_t)S.w * (uint32_t)S.bpp + 1u;
        if (inflate_checked(z, (uint32_t)S.h * rowlen, &px)) st = FI_EINVAL;
        for (int y = 0; !st && y < S.h; y++)
          if (px[(size_t)y * rowlen] > 4) st = FI_EINVAL;
      }
      printf("FILE %d\n", st);
    } else {
      printf("UNKNOWN\n");
    }
    done++;
  }
  printf("DONE %d\n", done);
  free(line);
  return 0;
}
