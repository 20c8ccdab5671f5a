// enc_batch_driver -- fi_enc_batch.h on its own, no HIP: the arena offsets, the
// per-image argument check and enc_deliver's handling of capacities and of
// rejected images.  Prints "PASS <case>" or "FAIL <case>: <what>" per case and
// "DONE"; built by tests/test_enc_batch_cpu.py with the system C++ compiler
// under ASan/UBSan, so a write past a capacity also stops the program.
#include <stdio.h>

#include <functional>
#include <string>
#include <vector>

#include "../../flyimg_amd/csrc/fi_enc_batch.h"

using namespace fi;

namespace {

std::string fail;  // the first thing wrong in the running case
void expect(bool ok, const char *what) {
  if (!ok && fail.empty()) fail = what;
}

// a staged stream of `nd` files of the given lengths, file k filled with k + 1
struct Staged {
  std::vector<int64_t> pos;
  std::vector<uint8_t> bytes;
  explicit Staged(const std::vector<size_t> &lens) {
    for (size_t k = 0; k < lens.size(); k++) {
      pos.push_back((int64_t)bytes.size());
      bytes.insert(bytes.end(), lens[k], (uint8_t)(k + 1));
      pos.push_back((int64_t)bytes.size());
    }
  }
};

bool all_are(const uint8_t *p, size_t n, uint8_t v) {
  for (size_t i = 0; i < n; i++)
    if (p[i] != v) return false;
  return true;
}

void arena() {
  auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t sizes[] = {0, 1, 255, 256, 257, 1000, 65536 + 3, 48, (size_t)5 << 32, 7};
  // the ladder as the encoders wrote it by hand
  const size_t o0 = 0, o1 = o0 + up256(sizes[0]), o2 = o1 + up256(sizes[1]), o3 = o2 + up256(sizes[2]);
  const size_t o4 = o3 + up256(sizes[3]), o5 = o4 + up256(sizes[4]), o6 = o5 + up256(sizes[5]);
  const size_t o7 = o6 + up256(sizes[6]), o8 = o7 + up256(sizes[7]), o9 = o8 + up256(sizes[8]);
  const size_t total = o9 + up256(sizes[9]);
  const size_t want[] = {o0, o1, o2, o3, o4, o5, o6, o7, o8, o9};
  EncArena a;
  expect(a.total() == 0, "an empty arena has bytes");
  for (int k = 0; k < 10; k++) {
    const size_t at = a.add(sizes[k]);
    expect(at == want[k], "offset differs from the hand-written ladder");
    expect(at % 256 == 0, "offset is no multiple of 256");
    expect(a.total() >= at + sizes[k], "total does not cover the region");
  }
  expect(a.total() == total, "total differs from the hand-written ladder");
  expect(o1 == 0 && o2 == 256 && o3 == 512 && o4 == 768 && o5 == 1280, "the ladder itself");
}

void io_status() {
  uint8_t px[16], ob[4];
  expect(enc_io_status(0, px, 12, 4, 3, ob, 4) == 0, "good arguments turned down");
  expect(enc_io_status(FI_EUNSUPPORTED, nullptr, 0, 4, 3, nullptr, 4) == FI_EUNSUPPORTED, "the codec's status is lost");
  expect(enc_io_status(0, nullptr, 12, 4, 3, ob, 4) == FI_EINVAL, "null source");
  expect(enc_io_status(0, px, 11, 4, 3, ob, 4) == FI_EINVAL, "stride below a row");
  expect(enc_io_status(0, px, 12, 4, 3, nullptr, 4) == FI_EINVAL, "null output with a capacity");
  expect(enc_io_status(0, px, 12, 4, 3, nullptr, 0) == 0, "null output without a capacity");
  expect(enc_io_status(0, px, (int64_t)4 << 30, 1 << 30, 4, ob, 4) == 0, "a row of 2^32 bytes");
  expect(enc_io_status(0, px, ((int64_t)4 << 30) - 1, 1 << 30, 4, ob, 4) == FI_EINVAL, "a row of 2^32 bytes, stride below");
}

// one image, a file of `len` bytes into a buffer of exactly `cap` (so ASan sees a
// byte too many) and into one with 0xA5 behind the capacity
void deliver_one(size_t len, size_t cap, bool prefix, int want_status, size_t want_written) {
  const Staged S({len});
  const int desc_img[1] = {0};
  for (int guarded = 0; guarded < 2; guarded++) {
    std::vector<uint8_t> buf(cap + (guarded ? 64 : 0), 0xA5);
    uint8_t *out[1] = {buf.data()};
    const size_t out_cap[1] = {cap};
    size_t out_len[1] = {0};
    int32_t status[1] = {0};
    enc_deliver(S.pos.data(), 1, desc_img, S.bytes.data(), out, out_cap, out_len, status, prefix);
    expect(out_len[0] == len, "out_len is not the true length");
    expect(status[0] == want_status, "status");
    expect(all_are(buf.data(), want_written, 1), "the file's bytes are not in the buffer");
    expect(all_are(buf.data() + want_written, buf.size() - want_written, 0xA5), "bytes written that should not be");
  }
}

void deliver_cap0_null() {
  const Staged S({5});
  const int desc_img[1] = {0};
  for (int prefix = 0; prefix < 2; prefix++) {
    uint8_t *out[1] = {nullptr};
    const size_t out_cap[1] = {0};
    size_t out_len[1] = {0};
    int32_t status[1] = {0};
    enc_deliver(S.pos.data(), 1, desc_img, S.bytes.data(), out, out_cap, out_len, status, prefix != 0);
    expect(out_len[0] == 5 && status[0] == FI_ENOMEM, "length / status of a size query");
  }
}

// five images, the middle one (and the last) rejected before the batch: the
// accepted ones are descriptors 0, 1, 2 = images 0, 1, 3
void deliver_rejected_middle() {
  const Staged S({7, 9, 11});
  const int desc_img[3] = {0, 1, 3};
  std::vector<std::vector<uint8_t>> bufs(5, std::vector<uint8_t>(16, 0xA5));
  uint8_t *out[5];
  size_t out_cap[5], out_len[5] = {0, 0, 0, 0, 0};
  int32_t status[5] = {0, 0, FI_EUNSUPPORTED, 0, FI_EINVAL};
  for (int i = 0; i < 5; i++) {
    out[i] = bufs[i].data();
    out_cap[i] = 16;
  }
  enc_deliver(S.pos.data(), 3, desc_img, S.bytes.data(), out, out_cap, out_len, status, true);
  const size_t want_len[5] = {7, 9, 0, 11, 0};
  const int32_t want_status[5] = {0, 0, FI_EUNSUPPORTED, 0, FI_EINVAL};
  const uint8_t fill[5] = {1, 2, 0, 3, 0};
  for (int i = 0; i < 5; i++) {
    expect(out_len[i] == want_len[i], "out_len");
    expect(status[i] == want_status[i], "status");
    expect(all_are(bufs[i].data(), want_len[i], fill[i]), "an image received another image's file");
    expect(all_are(bufs[i].data() + want_len[i], 16 - want_len[i], 0xA5), "bytes behind a file, or in a rejected buffer");
  }
}

}  // namespace

int main() {
  const std::pair<const char *, std::function<void()>> cases[] = {
      {"arena", arena},
      {"io_status", io_status},
      {"deliver_len_eq_cap", [] { deliver_one(40, 40, true, 0, 40), deliver_one(40, 40, false, 0, 40); }},
      {"deliver_short_prefix", [] { deliver_one(41, 40, true, FI_ENOMEM, 40); }},
      {"deliver_short_no_prefix", [] { deliver_one(41, 40, false, FI_ENOMEM, 0); }},
      {"deliver_cap0_null", deliver_cap0_null},
      {"deliver_rejected_middle", deliver_rejected_middle},
  };
  for (const auto &c : cases) {
    fail.clear();
    c.second();
    if (fail.empty())
      printf("PASS %s\n", c.first);
    else
      printf("FAIL %s: %s\n", c.first, fail.c_str());
  }
  printf("DONE\n");
  return 0;
}
