// Stand-alone driver of the GPU PNG encoder's host half (fi_png_write.cpp) and
// of the code that host and device share (fi_png_enc.h), built under
// ASan/UBSan by tests/test_png_encode_cpu.py.  One command per stdin line, one
// answer line each:
//   hdr W H C F        -> "HDR <33 bytes hex> <12 bytes hex> <bound> <stream bytes>" or "REJECT <rc>"
//   crc HEXA HEXB      -> "CRC <crc32(A)> <crc32(B)> <combined>"
//   adler BAND HEX     -> "ADLER <adler32 of the bytes, combined from bands of BAND bytes>"
//   huff MAXBITS F...  -> "HUFF <len>:<reversed code> ..."
//   block LAST N SYM.. -> "BLOCK <stored> <block bits> <bits written> <hex of the dynamic or fixed block>"; a symbol is a
//                         literal byte value, or LEN,DIST; N = the bytes they stand for
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../flyimg_amd/csrc/fi_png_enc.h"

using namespace fi;

static std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return v;
}
static void hex(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}

struct BitW {
  std::vector<uint8_t> out;
  int pos = 0;
  void put(uint64_t v, int nb) {
    for (int k = 0; k < nb; k++, pos++) {
      if ((pos & 7) == 0) out.push_back(0);
      out.back() |= (uint8_t)(((v >> k) & 1u) << (pos & 7));
    }
  }
};

int main() {
  char *line = nullptr;
  size_t cap = 0;
  int done = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "hdr") {
      int w, h, c, f;
      in >> w >> h >> c >> f;
      const int rc = png_enc_check(w, h, c, f);
      size_t bound = 0;
      if (rc || png_enc_bound(w, h, c, &bound)) {
        printf("REJECT %d\n", rc);
      } else {
        uint8_t hd[kPngHdrBytes], ie[12];
        png_enc_write_header(w, h, c, hd);
        png_enc_write_iend(ie);
        printf("HDR ");
        hex(hd, sizeof(hd));
        printf(" ");
        hex(ie, sizeof(ie));
        printf(" %zu %lld\n", bound, (long long)png_enc_stream_bytes(w, h, c));
      }
    } else if (cmd == "crc") {
      std::string a, b;
      in >> a >> b;
      const std::vector<uint8_t> A = unhex(a), B = unhex(b);
      const uint32_t ca = png_crc32(0, A.data(), A.size()), cb = png_crc32(0, B.data(), B.size());
      printf("CRC %u %u %u\n", ca, cb, png_crc_combine(ca, cb, B.size()));
    } else if (cmd == "adler") {
      size_t band;
      std::string d;
      in >> band >> d;
      const std::vector<uint8_t> D = unhex(d);
      uint32_t a = 1, b = 0;
      for (size_t o = 0; o < D.size(); o += band) {
        const size_t n = std::min(band, D.size() - o);
        uint64_t sa = 0, sb = 0;
        for (size_t i = 0; i < n; i++) {
          sa += D[o + i];
          sb += (uint64_t)D[o + i] * (n - i);
        }
        png_adler_append(&a, &b, (uint32_t)(sa % 65521u), (uint32_t)(sb % 65521u), (uint32_t)n);
      }
      printf("ADLER %u\n", (b << 16) | a);
    } else if (cmd == "huff") {
      int maxbits;
      in >> maxbits;
      std::vector<uint32_t> f;
      uint32_t v;
      while (in >> v) f.push_back(v);
      if (f.empty() || f.size() > 288 || maxbits < 1 || maxbits > 15) {
        printf("REJECT\n");
      } else {
        std::vector<uint8_t> len(f.size());
        std::vector<uint32_t> tab(f.size());
        PngHuffWork *ws = new PngHuffWork;
        png_huff_lengths(f.data(), (int)f.size(), maxbits, len.data(), ws);
        uint32_t work[34];
        png_huff_codes(len.data(), (int)f.size(), maxbits, tab.data(), work);
        delete ws;
        printf("HUFF");
        for (size_t i = 0; i < f.size(); i++) printf(" %u:%u", tab[i] >> 16, tab[i] & 0xFFFFu);
        printf("\n");
      }
    } else if (cmd == "block") {
      int last, n;
      in >> last >> n;
      std::vector<std::pair<int, int>> syms;  // (literal, 0) or (length, distance)
      std::string tok;
      while (in >> tok) {
        const size_t c = tok.find(',');
        if (c == std::string::npos)
          syms.push_back({atoi(tok.c_str()), 0});
        else
          syms.push_back({atoi(tok.substr(0, c).c_str()), atoi(tok.substr(c + 1).c_str())});
      }
      std::vector<uint32_t> hist(kPngHist, 0);
      int eb, ev;
      for (auto &s : syms) {
        if (!s.second) {
          hist[s.first]++;
        } else {
          hist[png_len_sym(s.first, &eb, &ev)]++;
          hist[kPngLL + png_dist_sym(s.second, &eb, &ev)]++;
        }
      }
      PngBandCode *K = new PngBandCode;
      PngCodeWork *ws = new PngCodeWork;
      png_build_block(hist.data(), n, last != 0, K, ws);
      BitW bw;
      bw.put((last ? 1u : 0u) | ((uint32_t)K->btype << 1), 3);
      for (int i = 0; i * 32 < K->hdr_bits; i++) bw.put(K->hdr[i], std::min(32, K->hdr_bits - 32 * i));
      for (auto &s : syms) {
        if (!s.second) {
          bw.put(K->ll[s.first] & 0xFFFFu, (int)(K->ll[s.first] >> 16));
        } else {
          const int ls = png_len_sym(s.first, &eb, &ev);
          bw.put(K->ll[ls] & 0xFFFFu, (int)(K->ll[ls] >> 16));
          bw.put((uint32_t)ev, eb);
          const int ds = png_dist_sym(s.second, &eb, &ev);
          bw.put(K->dist[ds] & 0xFFFFu, (int)(K->dist[ds] >> 16));
          bw.put((uint32_t)ev, eb);
        }
      }
      bw.put(K->ll[256] & 0xFFFFu, (int)(K->ll[256] >> 16));
      printf("BLOCK %d %d %d ", K->stored, K->block_bits, bw.pos);
      hex(bw.out.data(), bw.out.size());
      printf("\n");
      delete K;
      delete ws;
    } else {
      continue;
    }
    done++;
  }
  free(line);
  printf("DONE %d\n", done);
  return 0;
}
