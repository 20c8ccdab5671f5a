// jpeg_pwrite_driver -- the progressive JPEG encoder's host model and writer
// (fi_jpeg_pwrite.cpp with fi_jpeg_pcore.h: scan script, the four block
// procedures, optimal tables, file layout, size bound) on its own, for
// ASan/UBSan.  Reads lines "w h channels quality subsampling" from stdin; line
// k takes its coefficients (raw int16, the layout of fi_debug_jpeg_coefs_host)
// from <dir>/<k>.coef and writes the file to <dir>/<k>.jpg; prints
// "<k> LEN <bytes> FLUSH <flushes> BOUND <bound>" per line, "<k> REJECT <rc>"
// for settings or a coefficient count the writer turns down, "DONE <lines>" at
// the end.  A file beyond its bound is an error of the bound.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../flyimg_amd/csrc/fi_jpeg_enc.h"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  int w, h, c, q, s, n = 0;
  while (scanf("%d %d %d %d %d", &w, &h, &c, &q, &s) == 5) {
    std::vector<int16_t> coefs;
    FILE *f = fopen((dir + "/" + std::to_string(n) + ".coef").c_str(), "rb");
    if (f) {
      int16_t buf[4096];
      size_t got;
      while ((got = fread(buf, 2, 4096, f)) > 0) coefs.insert(coefs.end(), buf, buf + got);
      fclose(f);
    }
    size_t bound = 0;
    const int rb = fi::jpeg_penc_bound(w, h, c, q, s, &bound);
    if (rb != fi::jpeg_enc_check(w, h, c, q, s)) return 3;
    std::vector<uint8_t> file;
    int flushes = 0;
    const int rc = rb ? rb : fi::jpeg_penc_write(coefs.data(), coefs.size(), w, h, c, q, s, &file, &flushes);
    if (rc) {
      printf("%d REJECT %d\n", n++, rc);
      continue;
    }
    if (file.size() > bound) return 4;
    f = fopen((dir + "/" + std::to_string(n) + ".jpg").c_str(), "wb");
    if (!f || fwrite(file.data(), 1, file.size(), f) != file.size()) return 5;
    fclose(f);
    printf("%d LEN %zu FLUSH %d BOUND %zu\n", n++, file.size(), flushes, bound);
  }
  printf("DONE %d\n", n);
  return 0;
}
