// Stand-alone driver of the GPU PNG encoder's host half (fi_png_write.cpp) and
// of the code that host and device share (fi_png_enc.h, fi_enc_code.h), built
// under ASan/UBSan by tests/test_png_encode_cpu.py.  One command per stdin line, one
// answer line each:
//   hdr W H C F        -> "HDR <33 bytes hex> <12 bytes hex> <bound> <stream bytes>" or "REJECT <rc>"
//   crc HEXA HEXB      -> "CRC <crc32(A)> <crc32(B)> <combined>"
//   adler BAND HEX     -> "ADLER <adler32 of the bytes, combined from bands of BAND bytes>"
//   huff MAXBITS F...  -> "HUFF <len>:<reversed code> ..."
//   block LAST N SYM.. -> "BLOCK <stored> <block bits> <bits written> <hex of the dynamic or fixed block>"; a symbol is a
//                         literal byte value, or LEN,DIST; N = the bytes they stand for
//   rle LEN...         -> "RLE <sym>:<extra> ..." (enc_rle_lengths: 16 / 17 / 18 with their repeat counts' extra value)
//   bits CAP V:W ...   -> "BITS <over> <hex of the CAP bits> <position after each write, comma separated> <the same,
//                         counting only>"; every V of W bits through enc_put into a buffer of exactly CAP bits
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
        EncHuffWork *ws = new EncHuffWork;
        enc_huff_lengths(f.data(), (int)f.size(), maxbits, len.data(), ws);
        uint32_t work[34];
        enc_huff_codes(len.data(), (int)f.size(), maxbits, tab.data(), work);
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
          hist[kPngLL + enc_prefix_sym(s.second, &eb, &ev)]++;
        }
      }
      PngBandCode *K = new PngBandCode;
      PngCodeWork *ws = new PngCodeWork;
      png_build_block(hist.data(), n, last != 0, K, ws);
      // (a symbol takes at most 48 bits)
      std::vector<uint32_t> words(((size_t)syms.size() * 48 + kPngHdrWords * 32 + 64) / 32, 0);
      EncBits bw{words.data(), 0, (int64_t)words.size() * 32, 0};
      enc_put(&bw, (last ? 1u : 0u) | ((uint32_t)K->btype << 1), 3);
      for (int i = 0; i * 32 < K->hdr_bits; i++) enc_put(&bw, K->hdr[i], std::min(32, K->hdr_bits - 32 * i));
      for (auto &s : syms) {
        if (!s.second) {
          enc_put(&bw, K->ll[s.first] & 0xFFFFu, (int)(K->ll[s.first] >> 16));
        } else {
          const int ls = png_len_sym(s.first, &eb, &ev);
          enc_put(&bw, K->ll[ls] & 0xFFFFu, (int)(K->ll[ls] >> 16));
          enc_put(&bw, (uint32_t)ev, eb);
          const int ds = enc_prefix_sym(s.second, &eb, &ev);
          enc_put(&bw, K->dist[ds] & 0xFFFFu, (int)(K->dist[ds] >> 16));
          enc_put(&bw, (uint32_t)ev, eb);
        }
      }
      enc_put(&bw, K->ll[256] & 0xFFFFu, (int)(K->ll[256] >> 16));
      printf("BLOCK %d %d %d ", K->stored, K->block_bits, bw.over ? -1 : (int)bw.pos);
      for (int64_t i = 0; i < (bw.pos + 7) / 8; i++) printf("%02x", (words[i / 4] >> (8 * (i % 4))) & 255u);
      printf("\n");
      delete K;
      delete ws;
    } else if (cmd == "rle") {
      std::vector<uint8_t> lens;
      int v;
      while (in >> v) lens.push_back((uint8_t)v);
      std::vector<uint16_t> rle(lens.size() + 1);
      uint32_t freq[19];
      const int nr = enc_rle_lengths(lens.data(), (int)lens.size(), rle.data(), freq);
      uint32_t seen[19] = {0};
      for (int i = 0; i < nr; i++) seen[rle[i] & 255]++;
      if (nr > (int)lens.size() || memcmp(seen, freq, sizeof(seen))) {
        printf("REJECT\n");
      } else {
        printf("RLE");
        for (int i = 0; i < nr; i++) printf(" %d:%d", rle[i] & 255, rle[i] >> 8);
        printf("\n");
      }
    } else if (cmd == "bits") {
      long long capbits;
      in >> capbits;
      std::vector<std::pair<uint32_t, int>> puts;
      std::string tok;
      while (in >> tok) {
        const size_t c = tok.find(':');
        puts.push_back({(uint32_t)strtoul(tok.substr(0, c).c_str(), nullptr, 10), atoi(tok.substr(c + 1).c_str())});
      }
      // exactly the words the capacity covers: the sanitizer sees any other
      const size_t nw = (size_t)((capbits + 31) / 32);
      uint32_t *words = new uint32_t[nw ? nw : 1]();
      EncBits wr{words, 0, capbits, 0}, cnt{nullptr, 0, 0, 0};
      std::string at, atc;
      for (auto &pw : puts) {
        enc_put(&wr, pw.first, pw.second);
        enc_put(&cnt, pw.first, pw.second);
        at += (at.empty() ? "" : ",") + std::to_string(wr.pos);
        atc += (atc.empty() ? "" : ",") + std::to_string(cnt.pos);
      }
      printf("BITS %d ", wr.over);
      for (long long i = 0; i < (capbits + 7) / 8; i++) printf("%02x", (words[i / 4] >> (8 * (i % 4))) & 255u);
      printf(" %s %s\n", at.c_str(), atc.c_str());
      delete[] words;
    } else {
      continue;
    }
    done++;
  }
  free(line);
  printf("DONE %d\n", done);
  return 0;
}
