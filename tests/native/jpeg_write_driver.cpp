// jpeg_write_driver -- the GPU JPEG encoder's host side (fi_jpeg_write.cpp:
// tables, header writer, size bound) on its own, for ASan/UBSan.  Reads lines
// "w h channels quality subsampling" from stdin and writes each header to
// <dir>/<line number>.hdr; prints the bound per line, "DONE <lines>" at the
// end.  Bad arguments must be turned down by the check, never written.
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
    size_t bound = 0;
    const int rc = fi::jpeg_enc_bound(w, h, c, q, s, &bound);
    if (rc != fi::jpeg_enc_check(w, h, c, q, s)) return 3;
    if (rc) {
      printf("%d REJECT %d\n", n++, rc);
      continue;
    }
    std::vector<uint8_t> hdr;
    fi::jpeg_enc_write_header(w, h, c, q, s, &hdr);
    uint16_t qt[2][64];
    fi::jpeg_enc_quant_tables(q, qt);
    uint32_t huff[1024];
    fi::jpeg_enc_huff_tables(huff);
    int codes = 0;
    for (int i = 0; i < 1024; i++) codes += huff[i] != 0;
    if (codes != 12 + 162 + 12 + 162 || hdr.size() >= bound) return 4;
    const std::string path = dir + "/" + std::to_string(n) + ".hdr";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(hdr.data(), 1, hdr.size(), f) != hdr.size()) return 5;
    fclose(f);
    printf("%d BOUND %zu\n", n++, bound);
  }
  printf("DONE %d\n", n);
  return 0;
}
