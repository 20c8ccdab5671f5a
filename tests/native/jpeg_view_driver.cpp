// jpeg_view_driver -- the host side of the GPU decoder's views on its own, for
// ASan/UBSan: the index map of fi_jpeg_view.h and the EXIF orientation reader
// (fi_jpeg_parse.cpp jpeg_orientation).
//   jpeg_view_driver map           prints "MAP o W H : sx,sy ..." (the oriented
//                                  image in row-major order) for o = 1..8 at 5x3 and 1x4
//   jpeg_view_driver fuzz <files>  prints "FILE <index> <rc> <orientation>" per file,
//                                  then runs jpeg_orientation over every truncation of
//                                  the file and over seeded single-byte mutations of its
//                                  APP1 bodies, each in an exact-size heap buffer;
//                                  "DONE <calls>" at the end
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../flyimg_amd/csrc/fi_jpeg.h"
#include "../../flyimg_amd/csrc/fi_jpeg_view.h"

static uint32_t rng_state = 0x9E3779B9u;
static uint32_t rng() {  // xorshift32, fixed seed
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

static long calls = 0;
static int run(const uint8_t *d, size_t n, int *o) {
  std::vector<uint8_t> exact(d, d + n);  // exact size: a read past the end is a heap overflow
  *o = -1;
  const int rc = fi::jpeg_orientation(exact.data(), n, o);
  calls++;
  if (rc == FI_OK && (*o < 1 || *o > 8)) {
    fprintf(stderr, "orientation %d out of range\n", *o);
    exit(3);
  }
  return rc;
}

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "map") == 0) {
    const int sizes[2][2] = {{5, 3}, {1, 4}};
    for (const auto &wh : sizes)
      for (int o = 1; o <= 8; o++) {
        const int W = wh[0], H = wh[1];
        const int ow = fi::jpeg_view_transposed(o) ? H : W, oh = fi::jpeg_view_transposed(o) ? W : H;
        printf("MAP %d %d %d :", o, W, H);
        for (int v = 0; v < oh; v++)
          for (int u = 0; u < ow; u++) {
            int sx, sy;
            fi::jpeg_view_map(o, W, H, u, v, &sx, &sy);
            printf(" %d,%d", sx, sy);
          }
        printf("\n");
      }
    return 0;
  }
  if (argc < 3 || strcmp(argv[1], "fuzz") != 0) return 2;
  for (int a = 2; a < argc; a++) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) return 2;
    std::vector<uint8_t> d;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    int o;
    const int rc = run(d.data(), d.size(), &o);
    printf("FILE %d %d %d\n", a - 2, rc, o);
    for (size_t n = 0; n < d.size(); n++) run(d.data(), n, &o);
    // the APP1 bodies of the (well-formed up to SOS) file
    std::vector<size_t> body;
    for (size_t p = 2; p + 4 <= d.size() && d[p] == 0xFF && d[p + 1] != 0xDA;) {
      const size_t L = ((size_t)d[p + 2] << 8) | d[p + 3];
      if (L < 2 || p + 2 + L > d.size()) break;
      if (d[p + 1] == 0xE1)
        for (size_t q = p + 2; q < p + 2 + L; q++) body.push_back(q);  // (the length bytes too)
      p += 2 + L;
    }
    for (int k = 0; k < 2000 && !body.empty(); k++) {
      const size_t q = body[rng() % body.size()];
      const uint8_t keep = d[q];
      d[q] = (uint8_t)(k % 4 == 0 ? rng() : keep ^ (1u << (rng() % 8)));
      run(d.data(), d.size(), &o);
      d[q] = keep;
    }
  }
  printf("DONE %ld\n", calls);
  return 0;
}
