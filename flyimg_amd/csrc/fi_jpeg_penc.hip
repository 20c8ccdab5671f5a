// fi_jpeg_penc.hip -- progressive JPEG encode with per-scan optimal Huffman
// tables on the GPU, byte-identical with libjpeg-turbo through Pillow's
// Image.save(buf, "JPEG", quality=q, subsampling=s, progressive=True,
// restart_marker_rows=1).  One restart interval per block row of every scan
// makes each interval independent: byte aligned, DC prediction 0, EOB run and
// correction bits flushed at its end.  The coder itself (jcphuff.c's block
// procedures, jpeg_gen_optimal_table) is fi_jpeg_pcore.h, the code the host
// model (fi_jpeg_pwrite.cpp) runs: the kernels cannot drift from it.
//
//   k_jpeg_fdct   (fi_jpeg_enc.hip) the quantised coefficients, as for baseline;
//   k_jpeg_pstat  a lane per (image, scan, interval), a workgroup per 64 block
//            rows of one scan: the interval's symbols are counted through an
//            LDS histogram into the 257 bins of the scan's table(s); an AC
//            scan's lane copies each block into LDS first (eight 16-byte loads
//            in flight, not a memory round trip per coefficient);
//   k_jpeg_ptab   a lane per table: jpeg_gen_optimal_table, the derived codes
//            and the bytes of the DHT segment -- no histogram leaves the device;
//   k_jpeg_pcode  the work units of k_jpeg_pstat again: every lane codes its
//            interval, stuffed and with its RSTn, into a slot of the bound's size;
//   k_jpeg_pscan + k_jpeg_ppack   a file is a list of pieces -- head, per scan
//            [DHT ..., DRI / SOS, intervals], EOI: exclusive scan of their
//            lengths over the batch, then one workgroup per piece copies it
//            into one contiguous stream, which the host fetches with one copy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fi_enc_batch.h"
#include "fi_enc_pack.h"
#include "fi_internal.h"
#include "fi_jpeg_enc.h"
#include "fi_jpeg_enc_dev.h"
#include "fi_jpeg_pcore.h"

namespace fi {

constexpr int kPencDhtPitch = 288;  // bytes kept per DHT segment (>= kPencDhtMax)
static_assert(kPencDhtPitch >= kPencDhtMax, "DHT pitch");

struct PencImg {  // one image of the batch
  PencGeom G;
  int64_t blk0;   // its first block among the batch's coefficients
};
struct PencGrp {  // up to 64 consecutive intervals of one scan of one image
  int32_t img, scan, row0, nrows;
  int32_t iv0, pad;  // index of row0's interval among the batch's
  int64_t slot0;     // byte offset of row0's slot; the rows follow at slot_bytes
  int64_t slot_bytes;
};
struct PencPiece {  // one run of bytes of a file
  int32_t img;
  int32_t kind;     // 0: len bytes at `off` of the uploaded segments; 1: the DHT of table `off`; 2: interval ix's slot at `off`
  int64_t off;
  int32_t len, ix;
  int32_t first, last;  // of its image
};

struct PencCountSink {  // statistics: symbols into an LDS histogram
  uint32_t *cnt;        // [2][kPencHist]
  FI_PHD void sym(int t, int s) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(&cnt[kPencHist * t + s], 1u);
#else
    cnt[kPencHist * t + s]++;
#endif
  }
  FI_PHD void bits(uint32_t, int) {}
};

// A lane's copy of the block it is coding: 64 int16 at a pitch of 33 dwords, so
// the lanes of a wave that read the same coefficient hit 64 different banks
constexpr int kPencStagePitch = 66;
struct PencLdsStage {
  int16_t *mine;  // this lane's 66 int16, dword aligned
  __device__ const int16_t *load(const int16_t *b) {
    uint4 v[8];  // (blocks are 128-byte aligned; memcpy keeps the accesses typed as the coder reads them)
    __builtin_memcpy(v, __builtin_assume_aligned(b, 16), 128);
    __builtin_memcpy(__builtin_assume_aligned(mine, 4), v, 128);
    return mine;
  }
};

__device__ __forceinline__ PencLayout penc_dev_layout(const PencImg &I, const int16_t *coef) {
  PencLayout L;
  L.base = coef + I.blk0 * 64;
  L.planar = 0;
  L.bpm = I.G.bpm;
  L.mcux = I.G.mcux;
  for (int c = 0; c < 3; c++) {
    L.plane[c] = 0;
    L.pw[c] = 0;
  }
  return L;
}

__global__ __launch_bounds__(64) void k_jpeg_pstat(const PencImg *__restrict__ imgs, const PencGrp *__restrict__ grps,
                                                   int ngrp, const int16_t *__restrict__ coef,
                                                   uint32_t *__restrict__ hist) {
  __shared__ uint32_t cnt[2 * kPencHist];
  __shared__ __attribute__((aligned(16))) int16_t blk[64 * kPencStagePitch];
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= ngrp) return;
  for (int i = lane; i < 2 * kPencHist; i += 64) cnt[i] = 0;
  __syncthreads();
  const PencGrp Gp = grps[g];
  const PencImg I = imgs[Gp.img];
  const PencScan S = penc_scan(I.G.nc, Gp.scan);
  if (lane < Gp.nrows) {
    const PencLayout L = penc_dev_layout(I, coef);
    PencCountSink sink{cnt};
    PencLdsStage stage{blk + lane * kPencStagePitch};
    (void)penc_interval(I.G, S, L, Gp.row0 + lane, sink, stage);
  }
  __syncthreads();
  uint32_t *h = hist + ((int64_t)Gp.img * kPencTabs + 2 * Gp.scan) * kPencHist;
  for (int i = lane; i < 2 * kPencHist; i += 64)
    if (cnt[i]) atomicAdd(&h[i], cnt[i]);
}

// table (image, 2 * scan + slot): codes [256], DHT bytes, DHT length (0: the scan has no such table)
__global__ __launch_bounds__(64) void k_jpeg_ptab(const PencImg *__restrict__ imgs, int nimg,
                                                  const uint32_t *__restrict__ hist, uint32_t *__restrict__ codes,
                                                  uint8_t *__restrict__ dht, int32_t *__restrict__ dhtlen) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= nimg * kPencTabs) return;
  const int img = t / kPencTabs, k = t - img * kPencTabs, scan = k >> 1, slot = k & 1;
  const int nc = imgs[img].G.nc;
  int tc[2], nt = 0;
  if (scan < penc_nscans(nc)) nt = penc_scan_tables(penc_scan(nc, scan), tc);
  if (slot >= nt) {
    dhtlen[t] = 0;
    return;
  }
  uint8_t bits[17], vals[256];
  const int nv = penc_gen_table(hist + (int64_t)t * kPencHist, bits, vals, codes + (int64_t)t * 256);
  dhtlen[t] = penc_write_dht(dht + (int64_t)t * kPencDhtPitch, tc[slot], bits, vals, nv);
}

__global__ __launch_bounds__(64) void k_jpeg_pcode(const PencImg *__restrict__ imgs, const PencGrp *__restrict__ grps,
                                                   int ngrp, const int16_t *__restrict__ coef,
                                                   const uint32_t *__restrict__ codes, uint8_t *__restrict__ slots,
                                                   int32_t *__restrict__ ivlen) {
  __shared__ uint32_t code[512];
  __shared__ __attribute__((aligned(16))) int16_t blk[64 * kPencStagePitch];
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= ngrp) return;
  const PencGrp Gp = grps[g];
  const uint32_t *cg = codes + ((int64_t)Gp.img * kPencTabs + 2 * Gp.scan) * 256;
  for (int i = lane; i < 512; i += 64) code[i] = cg[i];
  __syncthreads();
  if (lane >= Gp.nrows) return;
  const PencImg I = imgs[Gp.img];
  const PencScan S = penc_scan(I.G.nc, Gp.scan);
  const PencLayout L = penc_dev_layout(I, coef);
  const int row = Gp.row0 + lane;
  uint8_t *out = slots + Gp.slot0 + (int64_t)lane * Gp.slot_bytes;
  PencByteSink bs;
  bs.init(out, Gp.slot_bytes - 2, code);  // (the bound holds by construction; no store leaves the slot regardless)
  PencLdsStage stage{blk + lane * kPencStagePitch};
  (void)penc_interval(I.G, S, L, row, bs, stage);
  bs.finish();
  int64_t n = bs.n < bs.cap ? bs.n : bs.cap;
  if (row != penc_scan_rows(I.G, S) - 1) {  // RSTn, counted from 0 in every scan
    out[n] = 0xFF;
    out[n + 1] = (uint8_t)(0xD0 + (row & 7));
    n += 2;
  }
  ivlen[Gp.iv0 + lane] = (int32_t)n;
}

__device__ __forceinline__ int penc_piece_len(const PencPiece &P, const int32_t *dhtlen, const int32_t *ivlen) {
  return P.kind == 0 ? P.len : P.kind == 1 ? dhtlen[P.off] : ivlen[P.ix];
}

// Exclusive scan of the pieces' lengths over the batch.  One workgroup.
// dst[p] = where piece p starts; imgpos[2 i] / [2 i + 1] = start / end of image i.
__global__ __launch_bounds__(256) void k_jpeg_pscan(const PencPiece *__restrict__ pieces, int np,
                                                    const int32_t *__restrict__ dhtlen,
                                                    const int32_t *__restrict__ ivlen, int64_t *__restrict__ dst,
                                                    int64_t *__restrict__ imgpos) {
  enc_scan_items(
      np,
      [=](int p) {
        const PencPiece P = pieces[p];
        return EncItem{penc_piece_len(P, dhtlen, ivlen), P.img, P.first != 0, P.last != 0};
      },
      dst, imgpos);
}

__global__ __launch_bounds__(64) void k_jpeg_ppack(const PencPiece *__restrict__ pieces, int np,
                                                   const int32_t *__restrict__ dhtlen,
                                                   const int32_t *__restrict__ ivlen, const int64_t *__restrict__ dst,
                                                   const uint8_t *__restrict__ segs, const uint8_t *__restrict__ dht,
                                                   const uint8_t *__restrict__ slots, uint8_t *__restrict__ packed) {
  const int p = blockIdx.x, t = threadIdx.x;
  if (p >= np) return;
  const PencPiece P = pieces[p];
  const int n = penc_piece_len(P, dhtlen, ivlen);
  const uint8_t *s = P.kind == 0 ? segs + P.off : P.kind == 1 ? dht + P.off * kPencDhtPitch : slots + P.off;
  uint8_t *d = packed + dst[p];
  for (int i = t; i < n; i += 64) d[i] = s[i];
}

// ---------------------------------------------------------------------------
// host: batch plan + launches (`alloc` / `stage` as in jpeg_encode_batch)
// ---------------------------------------------------------------------------
int jpeg_pencode_batch(hipStream_t st, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                       const int32_t *channels, const int64_t *src_stride, const int32_t *quality,
                       const int32_t *subsampling, int n, uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                       int32_t *status, void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *),
                       void *actx, std::string *err) {
  std::vector<JpegEncDesc> descs;
  std::vector<PencImg> imgs;
  std::vector<int> desc_img;
  std::vector<PencGrp> grps;
  std::vector<PencPiece> pieces;
  JpegEncQts qts;
  std::vector<uint8_t> segs;  // the bytes the host knows: heads, DRI / SOS, EOI
  int64_t nblocks = 0, niv = 0;
  size_t slot_total = 0, bound_total = 0;
  for (int i = 0; i < n; i++) {
    out_len[i] = 0;
    status[i] = enc_io_status(jpeg_enc_check(w[i], h[i], channels[i], quality[i], subsampling[i]), src[i],
                              src_stride[i], w[i], channels[i], out[i], out_cap[i]);
    if (status[i]) continue;
    const int img = (int)descs.size();
    const JpegEncDesc D =
        jpeg_enc_desc(src[i], src_stride[i], w[i], h[i], channels[i], quality[i], subsampling[i], nblocks, &qts);
    PencImg I{};
    penc_geom(D.W, D.H, D.C, subsampling[i], &I.G);
    I.blk0 = nblocks;
    auto seg_piece = [&](size_t from, bool first, bool last) {
      pieces.push_back({img, 0, (int64_t)from, (int32_t)(segs.size() - from), 0, first ? 1 : 0, last ? 1 : 0});
    };
    size_t from = segs.size();
    jpeg_penc_write_head(D.W, D.H, D.C, quality[i], subsampling[i], &segs);
    seg_piece(from, true, false);
    int last_interval = 0;
    for (int s = 0; s < penc_nscans(I.G.nc); s++) {
      const PencScan S = penc_scan(I.G.nc, s);
      int tc[2];
      const int nt = penc_scan_tables(S, tc);
      for (int t = 0; t < nt; t++) pieces.push_back({img, 1, (int64_t)img * kPencTabs + 2 * s + t, 0, 0, 0, 0});
      from = segs.size();
      jpeg_penc_write_scan_tail(D.W, D.H, D.C, subsampling[i], s, &last_interval, &segs);
      seg_piece(from, false, false);
      const int rows = penc_scan_rows(I.G, S);
      const int64_t sb = (int64_t)penc_slot_bytes(S, penc_scan_blocks(I.G, S));
      for (int r = 0; r < rows; r++) {
        if (r % 64 == 0)
          grps.push_back({img, s, r, std::min(64, rows - r), (int32_t)(niv + r), 0,
                          (int64_t)slot_total + (int64_t)r * sb, sb});
        pieces.push_back({img, 2, (int64_t)slot_total + (int64_t)r * sb, 0, (int32_t)(niv + r), 0, 0});
      }
      niv += rows;
      slot_total += (size_t)sb * rows;
    }
    from = segs.size();
    segs.push_back(0xFF);
    segs.push_back(0xD9);
    seg_piece(from, false, true);
    if (niv > (int64_t)1 << 28 || pieces.size() > (size_t)1 << 28 || segs.size() > (size_t)1 << 30) {
      *err = "JPEG encode batch too large";
      return FI_EINVAL;
    }
    nblocks += (int64_t)D.bpm * D.mcux * D.mcuy;
    size_t bnd = 0;
    (void)jpeg_penc_bound(D.W, D.H, D.C, quality[i], subsampling[i], &bnd);
    bound_total += bnd;
    descs.push_back(D);
    imgs.push_back(I);
    desc_img.push_back(i);
  }
  if (descs.empty()) return 0;
  const int nd = (int)descs.size(), ngrp = (int)grps.size(), np = (int)pieces.size();
  const int ntab = nd * kPencTabs;
  // upload: descriptors, images, groups, pieces, quantisation tables, the Annex K tables (k_jpeg_fdct), segments
  uint32_t huff[1024];
  jpeg_enc_huff_tables(huff);
  EncArena up, work;
  const size_t o_desc = up.add(descs.size() * sizeof(JpegEncDesc));
  const size_t o_img = up.add(imgs.size() * sizeof(PencImg));
  const size_t o_grp = up.add(grps.size() * sizeof(PencGrp));
  const size_t o_piece = up.add(pieces.size() * sizeof(PencPiece));
  const size_t o_qt = up.add(qts.tabs.size() * 2);
  const size_t o_huff = up.add(sizeof(huff));
  const size_t o_seg = up.add(segs.size());
  const size_t up_total = up.total();
  // work: coefficients, AC bit counts (unused here), histograms, codes, DHT bytes and lengths, interval lengths,
  // piece destinations, image positions, slots
  const size_t k_coef = work.add((size_t)nblocks * 128);
  const size_t k_bits = work.add((size_t)nblocks * 2);
  const size_t k_hist = work.add((size_t)ntab * kPencHist * 4);
  const size_t k_code = work.add((size_t)ntab * 256 * 4);
  const size_t k_dht = work.add((size_t)ntab * kPencDhtPitch);
  const size_t k_dhtlen = work.add((size_t)ntab * 4);
  const size_t k_ivlen = work.add((size_t)niv * 4);
  const size_t k_dst = work.add((size_t)np * 8);
  const size_t k_pos = work.add((size_t)nd * 16);
  const size_t k_slots = work.add(slot_total);
  const size_t work_total = work.total();
  uint8_t *dup = (uint8_t *)alloc(actx, 0, up_total);
  uint8_t *hst = (uint8_t *)alloc(actx, 3, std::max(up_total, (size_t)nd * 16));
  uint8_t *dwork = (uint8_t *)alloc(actx, 1, work_total);
  uint8_t *dpack = (uint8_t *)alloc(actx, 2, bound_total);
  if (!dup || !hst || !dwork || !dpack) {
    *err = "memory for the JPEG encode batch";
    return FI_ENOMEM;
  }
  memcpy(hst + o_desc, descs.data(), descs.size() * sizeof(JpegEncDesc));
  memcpy(hst + o_img, imgs.data(), imgs.size() * sizeof(PencImg));
  memcpy(hst + o_grp, grps.data(), grps.size() * sizeof(PencGrp));
  memcpy(hst + o_piece, pieces.data(), pieces.size() * sizeof(PencPiece));
  memcpy(hst + o_qt, qts.tabs.data(), qts.tabs.size() * 2);
  memcpy(hst + o_huff, huff, sizeof(huff));
  memcpy(hst + o_seg, segs.data(), segs.size());
  if (hipMemcpyAsync(dup, hst, up_total, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(dwork + k_hist, 0, (size_t)ntab * kPencHist * 4, st) != hipSuccess) {
    *err = "JPEG encode batch upload";
    return FI_EDEVICE;
  }
  const JpegEncDesc *dd = (const JpegEncDesc *)(dup + o_desc);
  const PencImg *dimg = (const PencImg *)(dup + o_img);
  const PencGrp *dgrp = (const PencGrp *)(dup + o_grp);
  const PencPiece *dpiece = (const PencPiece *)(dup + o_piece);
  int16_t *dcoef = (int16_t *)(dwork + k_coef);
  uint32_t *dhist = (uint32_t *)(dwork + k_hist);
  uint32_t *dcode = (uint32_t *)(dwork + k_code);
  uint8_t *ddht = dwork + k_dht;
  int32_t *ddhtlen = (int32_t *)(dwork + k_dhtlen);
  int32_t *divlen = (int32_t *)(dwork + k_ivlen);
  int64_t *ddst = (int64_t *)(dwork + k_dst);
  int64_t *dpos = (int64_t *)(dwork + k_pos);
  stage(actx, "k_jpeg_fdct");
  jpeg_enc_launch_fdct(st, dd, nd, nblocks, (const uint16_t *)(dup + o_qt), (const uint32_t *)(dup + o_huff), dcoef,
                       (uint16_t *)(dwork + k_bits));
  stage(actx, "k_jpeg_pstat");
  hipLaunchKernelGGL(k_jpeg_pstat, dim3((unsigned)ngrp), dim3(64), 0, st, dimg, dgrp, ngrp, dcoef, dhist);
  stage(actx, "k_jpeg_ptab");
  hipLaunchKernelGGL(k_jpeg_ptab, dim3((unsigned)((ntab + 63) / 64)), dim3(64), 0, st, dimg, nd, dhist, dcode, ddht,
                     ddhtlen);
  stage(actx, "k_jpeg_pcode");
  hipLaunchKernelGGL(k_jpeg_pcode, dim3((unsigned)ngrp), dim3(64), 0, st, dimg, dgrp, ngrp, dcoef, dcode,
                     dwork + k_slots, divlen);
  stage(actx, "k_jpeg_ppack");
  hipLaunchKernelGGL(k_jpeg_pscan, dim3(1), dim3(256), 0, st, dpiece, np, ddhtlen, divlen, ddst, dpos);
  hipLaunchKernelGGL(k_jpeg_ppack, dim3((unsigned)np), dim3(64), 0, st, dpiece, np, ddhtlen, divlen, ddst,
                     dup + o_seg, ddht, dwork + k_slots, dpack);
  stage(actx, nullptr);
  return enc_finish(st, alloc, actx, hst, dpos, nd, nullptr, dpack, bound_total, "JPEG", desc_img, out, out_cap, out_len,
                    status, true, err);
}
}  // namespace fi
