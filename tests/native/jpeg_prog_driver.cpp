// Host-only driver for the progressive JPEG path under ASan/UBSan: the parser
// (fi_jpeg_parse.cpp), the scan scheduler (jpeg_prog_items) and the host
// entropy decoder (fi_jpeg_prog_host.cpp), which runs the block procedures of
// fi_jpeg_prog.h that k_jpeg_prog runs on the device.  Every file named on
// the command line must decode (the damaged streams after "--damaged" may also
// be handed to the host, FI_EUNSUPPORTED); then every 7th truncation and 3000 seeded
// mutations of it (half of them in the entropy-coded bytes) are run.  The
// input, segment and coefficient buffers are exact-size heap allocations, so
// any access outside them trips ASan.  The mutants of a file are spread over
// a few threads (each mutant's bytes depend on its number only).  Prints
// "DONE <n>".
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../flyimg_amd/csrc/fi_jpeg.h"

static int run(const std::vector<uint8_t> &t) {
  fi::JpegHdr H;
  fi::JpegGeom G;
  std::vector<int16_t> coefs;
  return fi::jpeg_prog_coefs_host(t.data(), t.size(), FI_JPEG_PROGRESSIVE, &H, &G, &coefs);
}

int main(int argc, char **argv) {
  long n = 0;
  std::atomic<long> decoded(0);
  bool damaged = false;
  for (int a = 1; a < argc; a++) {
    if (std::string(argv[a]) == "--damaged") {
      damaged = true;
      continue;
    }
    FILE *f = fopen(argv[a], "rb");
    if (!f) return 2;
    std::vector<uint8_t> d;
    int ch;
    while ((ch = fgetc(f)) != EOF) d.push_back((uint8_t)ch);
    fclose(f);
    const int rc = run(d);
    if (rc != 0 && !(damaged && rc == FI_EUNSUPPORTED)) {
      fprintf(stderr, "%s does not decode\n", argv[a]);
      return 3;
    }
    n++;
    size_t sos = 0;  // the first SOS: entropy-coded bytes (and the later scans' headers) follow
    while (sos + 1 < d.size() && !(d[sos] == 0xFF && d[sos + 1] == 0xDA)) sos++;
    for (size_t L = 0; L < d.size(); L += 7) {
      std::vector<uint8_t> t(d.begin(), d.begin() + L);  // exact-size copy: overreads trip ASan
      run(t);
      n++;
    }
    auto mutant = [&](int m) {
      uint64_t rng = 0x9E3779B97F4A7C15ull * (uint64_t)(m + 1) + (uint64_t)a;
      auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
      };
      next();
      std::vector<uint8_t> t = d;
      const int k = 1 + (int)(next() % 4);
      for (int j = 0; j < k; j++) {
        if (m & 1) {  // entropy-coded bytes
          t[sos + next() % (t.size() - sos)] = (uint8_t)next();
        } else {      // headers, sometimes anywhere
          const size_t lim = (next() & 3) ? (sos + 16 < t.size() ? sos + 16 : t.size()) : t.size();
          t[next() % lim] = (uint8_t)next();
        }
      }
      decoded += run(t) == 0;
    };
    std::vector<std::thread> th;
    for (int w = 0; w < 8; w++)
      th.emplace_back([&, w]() {
        for (int m = w; m < 3000; m += 8) mutant(m);
      });
    for (auto &t : th) t.join();
    n += 3000;
  }
  printf("DONE %ld (%ld mutants decoded)\n", n, decoded.load());
  return 0;
}
