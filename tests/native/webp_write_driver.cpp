// Stand-alone driver of the GPU lossless WebP encoder's host half
// (fi_webp_write.cpp) and of the code that host and device share
// (fi_webp_enc.h), built under ASan/UBSan by tests/test_webp_encode_cpu.py.
// One command per stdin line, one answer line each:
//   bound W H C                  -> "BOUND <rc> <bytes>"
//   enc W H C STRIDE PRED CAP IN OUT -> "ENC <rc> <out_len>"; IN: a file of H * STRIDE source bytes; the
//                                   file goes to OUT from a heap buffer of exactly CAP bytes (-1: the bound)
//   code N F...                  -> "CODE <bits> <hex of the code as the stream carries it> <len>:<reversed code> ..."
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../flyimg_amd/csrc/fi_webp_enc.h"

using namespace fi;

static std::vector<uint8_t> slurp(const std::string &path) {
  std::vector<uint8_t> v;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return v;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

int main() {
  char *line = nullptr;
  size_t cap = 0;
  int done = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "bound") {
      int w, h, c;
      in >> w >> h >> c;
      size_t b = 0;
      const int rc = webp_enc_bound(w, h, c, &b);
      printf("BOUND %d %zu\n", rc, b);
    } else if (cmd == "enc") {
      int w, h, c, pred;
      long long stride, ocap;
      std::string ipath, opath;
      in >> w >> h >> c >> stride >> pred >> ocap >> ipath >> opath;
      const std::vector<uint8_t> px = slurp(ipath);
      size_t bound = 0;
      if (ocap < 0 && webp_enc_bound(w, h, c, &bound) == 0) ocap = (long long)bound;
      if (ocap < 0) ocap = 0;
      // exactly the bytes the call may touch: the sanitizer sees any other
      std::unique_ptr<uint8_t[]> src(new uint8_t[px.size() ? px.size() : 1]);
      memcpy(src.get(), px.data(), px.size());
      std::unique_ptr<uint8_t[]> out(new uint8_t[ocap ? ocap : 1]);
      size_t len = 0;
      int rc = -100;
      if (h < 1 || stride < 0 || (size_t)((long long)(h - 1) * stride + (long long)w * c) <= px.size() || w < 1 || c < 1)
        rc = webp_encode_host(src.get(), w, h, c, stride, pred, out.get(), (size_t)ocap, &len);
      if (rc == 0) {
        FILE *f = fopen(opath.c_str(), "wb");
        if (f) {
          fwrite(out.get(), 1, len, f);
          fclose(f);
        }
      }
      printf("ENC %d %zu\n", rc, len);
    } else if (cmd == "code") {
      int n;
      in >> n;
      std::vector<uint32_t> f;
      uint32_t v;
      while (in >> v) f.push_back(v);
      if (n < 1 || n > kWebpG || (int)f.size() != n) {
        printf("REJECT\n");
      } else {
        std::vector<uint32_t> tab(n), words(1024, 0);
        std::unique_ptr<WebpCodeWork> ws(new WebpCodeWork);
        WebpBits bw{words.data(), 0, 1024 * 32, 0};
        webp_write_code(f.data(), n, tab.data(), &bw, ws.get());
        printf("CODE %lld ", bw.over ? -1ll : (long long)bw.pos);
        for (long long i = 0; i < (bw.pos + 7) / 8; i++) printf("%02x", (words[i / 4] >> (8 * (i % 4))) & 255u);
        for (int i = 0; i < n; i++) printf(" %u:%u", tab[i] >> 16, tab[i] & 0xFFFFu);
        printf("\n");
      }
    } else {
      continue;
    }
    done++;
  }
  free(line);
  printf("DONE %d\n", done);
  return 0;
}
