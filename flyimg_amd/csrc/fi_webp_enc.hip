// fi_webp_enc.hip -- lossless WebP (VP8L) encode on the GPU.  The algorithm is
// fi_webp_enc.h's inline code, which the host runs too (fi_webp_write.cpp: same
// bytes); this file holds the kernels around it, the emitter and the batch plan:
//
//   k_webp_pred   a wave per 16 x 16 block: subtract green, the cost sum
//            min(x, 256 - x) of the 14 predictor modes from original neighbours
//            (blocks are independent), the cheapest mode -> mode image, the
//            residual ARGB stream;
//   k_webp_lz     a wave per band of 8192 residual pixels, the band in LDS
//            beside a 4K-entry hash table of two-pixel prefixes that moves 64
//            positions at a time (LDS atomic max: the last position of a group
//            wins on the host and here alike); candidates: the table's and the
//            pixel before; greedy parse with a cost gate; tokens -> scratch,
//            the band's histograms -> its record and, added, the image's five;
//   k_webp_codes  a wave per image: lane 0 builds the five codes with the
//            length-limited builder of fi_enc_code.h and writes the RIFF and
//            VP8L headers, the transforms, the mode image and the codes into the
//            image's zeroed slot; the lanes price the bands from their
//            histograms; prefix sum -> each band's bit offset; the fallback
//            form (flat 8-bit codes, no predictor, no matches: the size bound)
//            is priced too and taken where smaller;
//   k_webp_emit   a workgroup per band: bits per token, prefix sum, 256 tokens
//            at a time ORed into an LDS bit buffer at the band's global bit
//            offset mod 32; whole dwords -> the slot with plain stores, the
//            band's first dword and its last partial dword with atomic OR (bands
//            are not byte aligned in VP8L: neighbours share those dwords);
//   k_webp_pack   exclusive scan of the file sizes (k_webp_scan: the scan of
//            fi_enc_pack.h with an image as the item), slots -> one contiguous
//            stream, which the host fetches with one copy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fi_enc_batch.h"
#include "fi_enc_dev.h"
#include "fi_enc_pack.h"
#include "fi_internal.h"
#define FI_WEBP_DEVICE 1
#include "fi_webp_enc.h"

namespace fi {

constexpr int kWebpChunkWords = 256 * 60 / 32 + 4;  // 256 tokens of at most 60 bits, a dword of lead, spill-over

__global__ __launch_bounds__(64) void k_webp_pred(const WebpImg *__restrict__ descs, int nimg, int64_t nblocks,
                                                  uint32_t *__restrict__ resid, uint8_t *__restrict__ modes) {
  __shared__ uint32_t cost[16];
  const int64_t blk = blockIdx.x;
  if (blk >= nblocks) return;
  const WebpImg &I = descs[enc_find_image(descs, nimg, blk, &WebpImg::block0)];
  webp_pred_block(I, (int)(blk - I.block0), (int)threadIdx.x, 64, cost, resid + I.px0, modes + I.block0);
}

__global__ __launch_bounds__(64) void k_webp_lz(const WebpImg *__restrict__ descs, const WebpBandRef *__restrict__ bands,
                                                int nbands, const uint32_t *__restrict__ resid,
                                                uint32_t *__restrict__ toks, int32_t *__restrict__ ntoks,
                                                uint32_t *__restrict__ bandhists, uint32_t *__restrict__ imghists) {
  __shared__ WebpLzWork S;
  const int band = blockIdx.x;
  if (band >= nbands) return;
  const WebpBandRef B = bands[band];
  const WebpImg &I = descs[B.img];
  const int64_t off = I.px0 + (int64_t)B.idx * kWebpBand;
  const int n = std::min(kWebpBand, I.npix - B.idx * kWebpBand);
  webp_lz_band(resid + off, n, (int)threadIdx.x, 64, &S, toks + off, ntoks + band,
               bandhists + (int64_t)band * kWebpHist, imghists + (int64_t)B.img * kWebpHist);
}

__global__ __launch_bounds__(64) void k_webp_codes(const WebpImg *__restrict__ descs, int nimg,
                                                   const uint32_t *__restrict__ imghists,
                                                   const uint8_t *__restrict__ modes,
                                                   const uint32_t *__restrict__ bandhists, uint32_t *__restrict__ tabs,
                                                   int64_t *__restrict__ bandoff, uint8_t *__restrict__ slots,
                                                   WebpImgOut *__restrict__ outs, int32_t *__restrict__ fault) {
  __shared__ WebpBuildWork ws;
  const int img = blockIdx.x;
  if (img >= nimg) return;
  const WebpImg &I = descs[img];
  webp_build_image(I, imghists + (int64_t)img * kWebpHist, modes + I.block0, bandhists + (int64_t)I.band0 * kWebpHist,
                   (int)threadIdx.x, 64, &ws, tabs + (int64_t)img * kWebpHist, bandoff + I.band0,
                   reinterpret_cast<uint32_t *>(slots + I.slot0), outs + img, fault);
}

__global__ __launch_bounds__(256) void k_webp_emit(const WebpImg *__restrict__ descs,
                                                   const WebpBandRef *__restrict__ bands, int nbands,
                                                   const uint32_t *__restrict__ resid, const uint32_t *__restrict__ toks,
                                                   const int32_t *__restrict__ ntoks, const uint32_t *__restrict__ tabs_g,
                                                   const int64_t *__restrict__ bandoff,
                                                   const WebpImgOut *__restrict__ outs, uint8_t *__restrict__ slots,
                                                   int32_t *__restrict__ fault) {
  __shared__ uint32_t tabs[kWebpHist];
  __shared__ uint32_t buf[kWebpChunkWords];
  __shared__ int wsum[4];
  const int band = blockIdx.x, t = threadIdx.x;
  if (band >= nbands) return;
  const WebpBandRef B = bands[band];
  const WebpImg &I = descs[B.img];
  const WebpImgOut &R = outs[B.img];
  const int n = std::min(kWebpBand, I.npix - B.idx * kWebpBand);
  const bool fb = R.fallback != 0;
  const int nt = fb ? n : ntoks[band];
  for (int i = t; i < kWebpHist; i += 256) tabs[i] = tabs_g[(int64_t)B.img * kWebpHist + i];
  for (int i = t; i < kWebpChunkWords; i += 256) buf[i] = 0;
  __syncthreads();
  uint32_t *slot = reinterpret_cast<uint32_t *>(slots + I.slot0);
  const int64_t slotwords = I.slot_bytes >> 2;
  int64_t cur = (int64_t)kWebpRiffBytes * 8 + bandoff[band];  // bit in the slot (uniform)
  const int64_t firstw = cur >> 5;
  const int64_t want = (int64_t)kWebpRiffBytes * 8 + (B.idx + 1 < I.nbands ? bandoff[band + 1] : R.total_bits);
  const int64_t off = I.px0 + (int64_t)B.idx * kWebpBand;
  const uint32_t *tk = toks + off, *rs = resid + off;
  bool ok = true;  // every dword found its place, and the band has the size k_webp_codes priced
  for (int base = 0; base < nt; base += 256) {
    const int i = base + t;
    uint64_t val = 0;
    int nb = 0;
    if (i < nt) {
      const uint32_t tok = fb ? (uint32_t)i : tk[i];
      uint32_t argb = 0;
      if (!(tok & 0x80000000u)) {
        if (fb) {
          const int64_t p = (int64_t)B.idx * kWebpBand + i;
          argb = webp_px(I, (int)(p % I.W), (int)(p / I.W), I.C <= 2);
        } else {
          argb = rs[tok];
        }
      }
      nb = webp_token_bits(tok, argb, tabs, &val);
    }
    int total;
    const int before = enc_offset256(nb, wsum, &total);
    const int64_t w0 = cur >> 5;
    // (no guard: a chunk is at most 31 + 256 * 60 bits, which kWebpChunkWords holds)
    (void)enc_or_bits<false>(buf, kWebpChunkWords, (int)(cur & 31) + before, val, nb);
    __syncthreads();
    const int64_t endbit = cur + total;
    const int nfull = (int)((endbit >> 5) - w0);  // dwords complete after this chunk
    for (int k = t; k < nfull; k += 256) {
      const int64_t gw = w0 + k;
      if (gw >= slotwords)
        ok = false;
      else if (gw == firstw)
        atomicOr(&slot[gw], buf[k]);  // shared with the band before, or with the header
      else
        slot[gw] = buf[k];
    }
    const uint32_t carry = buf[nfull];
    __syncthreads();
    for (int k = t; k < kWebpChunkWords; k += 256) buf[k] = k == 0 ? carry : 0u;
    __syncthreads();
    cur = endbit;
  }
  if (t == 0 && (cur & 31)) {  // shared with the band behind
    const int64_t gw = cur >> 5;
    if (gw >= slotwords)
      ok = false;
    else
      atomicOr(&slot[gw], buf[0]);
  }
  if (cur != want) ok = false;
  if (!ok) *fault = 1;
}

// every image is one item: its file, clamped to its slot
__global__ __launch_bounds__(256) void k_webp_scan(const WebpImg *__restrict__ descs,
                                                   const WebpImgOut *__restrict__ outs, int nimg,
                                                   int64_t *__restrict__ imgpos) {
  enc_scan_items(
      nimg, [=](int k) { return EncItem{std::min(outs[k].file_bytes, descs[k].slot_bytes), k, true, true}; }, nullptr,
      imgpos);
}

// blockIdx.x: the image, blockIdx.y: its share of the copy
__global__ __launch_bounds__(256) void k_webp_pack(const WebpImg *__restrict__ descs, int nimg,
                                                   const int64_t *__restrict__ imgpos,
                                                   const uint8_t *__restrict__ slots, uint8_t *__restrict__ packed) {
  const int img = blockIdx.x;
  if (img >= nimg) return;
  enc_copy_aligned(packed + imgpos[2 * img], slots + descs[img].slot0, imgpos[2 * img + 1] - imgpos[2 * img],
                   (int64_t)blockIdx.y * 256 + threadIdx.x, (int64_t)gridDim.y * 256);
}

// ---------------------------------------------------------------------------
// host: batch plan + launches (`alloc` / `stage` as in jpeg_encode_batch)
// ---------------------------------------------------------------------------
int webp_encode_batch(hipStream_t st, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                      const int32_t *channels, const int64_t *src_stride, const int32_t *predictor, int n,
                      uint8_t *const *out, const size_t *out_cap, size_t *out_len, int32_t *status,
                      void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *), void *actx,
                      std::string *err) {
  std::vector<WebpImg> descs;
  std::vector<int> desc_img;
  std::vector<WebpBandRef> bands;
  int64_t nblocks = 0, npix = 0, slot_total = 0;
  for (int i = 0; i < n; i++) {
    out_len[i] = 0;
    const int p = predictor ? predictor[i] : -1;
    status[i] = enc_io_status(webp_enc_check(w[i], h[i], channels[i], p), src[i], src_stride[i], w[i], channels[i],
                              out[i], out_cap[i]);
    if (status[i]) continue;
    size_t bnd = 0;
    (void)webp_enc_bound(w[i], h[i], channels[i], &bnd);
    WebpImg D{};
    D.src = src[i];
    D.stride = src_stride[i];
    D.W = w[i];
    D.H = h[i];
    D.C = channels[i];
    D.pred = p;
    D.bw = (D.W + 15) >> kWebpBlockBits;
    D.bh = (D.H + 15) >> kWebpBlockBits;
    D.npix = D.W * D.H;
    D.nbands = (D.npix + kWebpBand - 1) / kWebpBand;
    D.band0 = (int32_t)bands.size();
    D.fb_hdr = webp_fallback_hdr_bits(D.C);
    D.block0 = nblocks;
    D.px0 = npix;
    D.slot0 = slot_total;
    D.slot_bytes = (int64_t)((bnd + 4 + 15) & ~(size_t)15);
    if (bands.size() + (size_t)D.nbands > (size_t)1 << 24 || nblocks + (int64_t)D.bw * D.bh > (int64_t)1 << 30) {
      *err = "WebP encode batch too large";
      return FI_EINVAL;
    }
    for (int b = 0; b < D.nbands; b++) bands.push_back({(int32_t)descs.size(), b});
    nblocks += (int64_t)D.bw * D.bh;
    npix += D.npix;
    slot_total += D.slot_bytes;
    descs.push_back(D);
    desc_img.push_back(i);
  }
  if (descs.empty()) return 0;
  const int nd = (int)descs.size(), nb = (int)bands.size();
  // upload: descriptors, bands
  EncArena up, work;
  const size_t o_desc = up.add(descs.size() * sizeof(WebpImg));
  const size_t o_band = up.add(bands.size() * sizeof(WebpBandRef));
  const size_t up_total = up.total();
  // work: residuals, tokens, modes, token counts, band histograms, band offsets, code tables, decisions,
  // [zeroed from here] image histograms, positions + fault word, slots
  const size_t k_resid = work.add((size_t)npix * 4);
  const size_t k_tok = work.add((size_t)npix * 4);
  const size_t k_modes = work.add((size_t)nblocks);
  const size_t k_ntok = work.add((size_t)nb * 4);
  const size_t k_bhist = work.add((size_t)nb * kWebpHist * 4);
  const size_t k_boff = work.add((size_t)nb * 8);
  const size_t k_tabs = work.add((size_t)nd * kWebpHist * 4);
  const size_t k_outs = work.add((size_t)nd * sizeof(WebpImgOut));
  const size_t k_ihist = work.add((size_t)nd * kWebpHist * 4);
  const size_t k_pos = work.add((size_t)nd * 16 + 16);  // (+ the fault word behind the positions)
  const size_t k_slots = work.add((size_t)slot_total);
  const size_t work_total = work.total();
  uint8_t *dup = (uint8_t *)alloc(actx, 0, up_total);
  uint8_t *hst = (uint8_t *)alloc(actx, 3, std::max(up_total, (size_t)nd * 16 + 16));
  uint8_t *dwork = (uint8_t *)alloc(actx, 1, work_total);
  uint8_t *dpack = (uint8_t *)alloc(actx, 2, (size_t)slot_total + 16);
  if (!dup || !hst || !dwork || !dpack) {
    *err = "memory for the WebP encode batch";
    return FI_ENOMEM;
  }
  memcpy(hst + o_desc, descs.data(), descs.size() * sizeof(WebpImg));
  memcpy(hst + o_band, bands.data(), bands.size() * sizeof(WebpBandRef));
  if (hipMemcpyAsync(dup, hst, up_total, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(dwork + k_ihist, 0, work_total - k_ihist, st) != hipSuccess) {
    *err = "WebP encode batch upload";
    return FI_EDEVICE;
  }
  const WebpImg *dd = (const WebpImg *)(dup + o_desc);
  const WebpBandRef *db = (const WebpBandRef *)(dup + o_band);
  uint32_t *dresid = (uint32_t *)(dwork + k_resid), *dtok = (uint32_t *)(dwork + k_tok);
  uint8_t *dmodes = dwork + k_modes;
  int32_t *dntok = (int32_t *)(dwork + k_ntok);
  uint32_t *dbhist = (uint32_t *)(dwork + k_bhist), *dihist = (uint32_t *)(dwork + k_ihist);
  int64_t *dboff = (int64_t *)(dwork + k_boff);
  uint32_t *dtabs = (uint32_t *)(dwork + k_tabs);
  WebpImgOut *douts = (WebpImgOut *)(dwork + k_outs);
  int64_t *dpos = (int64_t *)(dwork + k_pos);
  int32_t *dfault = (int32_t *)(dpos + 2 * (size_t)nd);
  uint8_t *dslots = dwork + k_slots;
  stage(actx, "k_webp_pred");
  hipLaunchKernelGGL(k_webp_pred, dim3((unsigned)nblocks), dim3(64), 0, st, dd, nd, nblocks, dresid, dmodes);
  stage(actx, "k_webp_lz");
  hipLaunchKernelGGL(k_webp_lz, dim3((unsigned)nb), dim3(64), 0, st, dd, db, nb, dresid, dtok, dntok, dbhist, dihist);
  stage(actx, "k_webp_codes");
  hipLaunchKernelGGL(k_webp_codes, dim3((unsigned)nd), dim3(64), 0, st, dd, nd, dihist, dmodes, dbhist, dtabs, dboff,
                     dslots, douts, dfault);
  stage(actx, "k_webp_emit");
  hipLaunchKernelGGL(k_webp_emit, dim3((unsigned)nb), dim3(256), 0, st, dd, db, nb, dresid, dtok, dntok, dtabs, dboff,
                     douts, dslots, dfault);
  stage(actx, "k_webp_pack");
  hipLaunchKernelGGL(k_webp_scan, dim3(1), dim3(256), 0, st, dd, douts, nd, dpos);
  hipLaunchKernelGGL(k_webp_pack, dim3((unsigned)nd, 16), dim3(256), 0, st, dd, nd, dpos, dslots, dpack);
  stage(actx, nullptr);
  // (a file longer than its buffer: nothing is written, as in the host form)
  return enc_finish(st, alloc, actx, hst, dpos, nd, "WebP encode: the bits emitted differ from the bits priced", dpack,
                    (size_t)slot_total, "WebP", desc_img, out, out_cap, out_len, status, false, err);
}
}  // namespace fi
