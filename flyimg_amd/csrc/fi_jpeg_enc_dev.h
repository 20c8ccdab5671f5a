// fi_jpeg_enc_dev.h -- what the two GPU JPEG encoders share on the device side:
// the batch's image descriptor (with the fill of its common fields and the
// batch's quantisation tables) and the launch of k_jpeg_fdct (fi_jpeg_enc.hip),
// whose quantised coefficients the baseline coder (k_jpeg_henc) and the
// progressive one (fi_jpeg_penc.hip) both code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <vector>

#include "fi_jpeg_enc.h"

namespace fi {

struct JpegEncDesc {     // one image of an encode batch
  const uint8_t *src;    // HWC u8, 1 or 3 channels
  int64_t stride;
  int32_t W, H, C;
  int32_t bpm;           // blocks per MCU: 1 gray, 3 4:4:4, 6 4:2:0 (Y Y Y Y Cb Cr)
  int32_t mcux, mcuy;
  int32_t qt;            // index of its table pair (u16 [2][64], natural order)
  int32_t iv0;           // its first restart interval in the batch
  int64_t blk0;          // its first block in the batch (blocks in MCU order)
  int64_t slot0;         // byte offset of its first interval slot
  int64_t slot_bytes;    // bytes per slot
  int32_t hdr_off, hdr_len;  // its header bytes in the upload
};

struct JpegEncQts {      // the table pairs of a batch, one per distinct quality
  std::vector<uint16_t> tabs;  // u16 [2][64] per pair, natural order
  std::map<int, int> ix;       // quality -> pair
  int pair(int quality) {
    auto it = ix.find(quality);
    if (it == ix.end()) {
      uint16_t t[2][64];
      jpeg_enc_quant_tables(quality, t);
      it = ix.emplace(quality, (int)(tabs.size() / 128)).first;
      tabs.insert(tabs.end(), &t[0][0], &t[0][0] + 128);
    }
    return it->second;
  }
};

// the fields k_jpeg_fdct reads, for an image whose blocks start at blk0
inline JpegEncDesc jpeg_enc_desc(const uint8_t *src, int64_t stride, int w, int h, int channels, int quality,
                                 int subsampling, int64_t blk0, JpegEncQts *qts) {
  JpegEncDesc D{};
  D.src = src;
  D.stride = stride;
  D.W = w;
  D.H = h;
  D.C = channels;
  jpeg_enc_grid(w, h, channels, subsampling, &D.bpm, &D.mcux, &D.mcuy);
  D.qt = qts->pair(quality);
  D.blk0 = blk0;
  return D;
}

// k_jpeg_fdct over the batch's nblocks blocks: coef = 64 int16 per block in
// zigzag order, blocks in MCU order; acbits = the bits of each block's baseline
// AC symbols under the Annex K tables `huff` (jpeg_enc_huff_tables)
void jpeg_enc_launch_fdct(hipStream_t st, const JpegEncDesc *descs, int nimg, int64_t nblocks, const uint16_t *qts,
                          const uint32_t *huff, int16_t *coef, uint16_t *acbits);

}  // namespace fi
