// fi_jpeg_enc_dev.h -- what the two GPU JPEG encoders share on the device side:
// the batch's image descriptor and the launch of k_jpeg_fdct (fi_jpeg_enc.hip),
// whose quantised coefficients the baseline coder (k_jpeg_henc) and the
// progressive one (fi_jpeg_penc.hip) both code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// k_jpeg_fdct over the batch's nblocks blocks: coef = 64 int16 per block in
// zigzag order, blocks in MCU order; acbits = the bits of each block's baseline
// AC symbols under the Annex K tables `huff` (jpeg_enc_huff_tables)
void jpeg_enc_launch_fdct(hipStream_t st, const JpegEncDesc *descs, int nimg, int64_t nblocks, const uint16_t *qts,
                          const uint32_t *huff, int16_t *coef, uint16_t *acbits);

}  // namespace fi
