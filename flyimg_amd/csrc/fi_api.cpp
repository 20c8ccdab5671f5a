// fi_api.cpp -- what remains of the C-ABI runtime of libflyimg_hip.so
// (include/flyimg_hip.h) beside its parts: fi_context.cpp (context, buffers,
// heaps, statistics), fi_rs_plan.cpp + fi_tiles.cpp (the batch planner),
// fi_sc_plan.cpp (smartcrop), fi_batch.cpp (the batch pipeline), fi_jpeg_api.cpp
// and fi_rccl.cpp.  Here: the host-only planning entry points (fi_plan,
// fi_plan_bytes), the face-blur pixelation path and the kernel debug hooks.
#include "fi_runtime.h"

using namespace fi;

// face-blur pixelation (fi_pixelate.hip): per box, the crop's 10% ScaleImage
// into a Q16 scratch, then its 1000% ScaleImage onto the image at (X, Y).
static int pixelate_device(fi_ctx *c, uint8_t *img, int w, int h, int64_t stride, int C, const int32_t *boxes,
                           int nboxes) {
  if (!img || w <= 0 || h <= 0 || (C != 1 && C != 3) || stride < (int64_t)w * C || nboxes < 0 ||
      (nboxes > 0 && !boxes))
    return set_err(FI_EINVAL, "bad pixelate arguments");
  std::vector<int32_t> ti;
  std::vector<double> td;
  struct Box {
    PixPass down, up;
  };
  std::vector<Box> plan;
  size_t scratch = 0;
  int first_bad = -1;
  std::string why;
  auto put = [&](const ScaleList &L, int32_t *off, int32_t *idx, int32_t *wt) {
    *off = (int32_t)ti.size();
    ti.insert(ti.end(), L.off.begin(), L.off.end());
    *idx = (int32_t)ti.size();
    ti.insert(ti.end(), L.idx.begin(), L.idx.end());
    *wt = (int32_t)td.size();
    td.insert(td.end(), L.w.begin(), L.w.end());
  };
  for (int b = 0; b < nboxes; b++) {
    const int bx = boxes[4 * b], by = boxes[4 * b + 1], bw = boxes[4 * b + 2], bh = boxes[4 * b + 3];
    if (bw <= 0 || bh <= 0 || bx < 0 || by < 0 || bx >= w || by >= h) {
      first_bad = b;
      why = "geometry does not contain image";
      break;
    }
    const int rw = std::min(bw, w - bx), rh = std::min(bh, h - by);  // CropImage clip
    const int dw = im_percent_size(rw, 10.0), dh = im_percent_size(rh, 10.0);
    if (dw <= 0 || dh <= 0) {
      first_bad = b;
      why = "NegativeOrZeroImageSize (the 10% scale is empty)";
      break;
    }
    const int uw = im_percent_size(dw, 1000.0), uh = im_percent_size(dh, 1000.0);
    Box B{};
    ScaleList L;
    im_scale_rows(rh, dh, &L);
    put(L, &B.down.yoff, &B.down.yidx, &B.down.yw);
    im_scale_cols(rw, dw, &L);
    put(L, &B.down.xoff, &B.down.xidx, &B.down.xw);
    im_scale_rows(dh, uh, &L);
    put(L, &B.up.yoff, &B.up.yidx, &B.up.yw);
    im_scale_cols(dw, uw, &L);
    put(L, &B.up.xoff, &B.up.xidx, &B.up.xw);
    B.down.src8 = img + (int64_t)by * stride + (int64_t)bx * C;
    B.down.sstride = stride;
    B.down.iw = rw;
    B.down.ih = rh;
    B.down.ow = dw;
    B.down.oh = dh;
    B.down.C = C;
    B.down.dst16 = (uint16_t *)(uintptr_t)(scratch + 1);  // tagged: resolved after upload
    B.up.src16 = B.down.dst16;
    B.up.iw = dw;
    B.up.ih = dh;
    B.up.ow = uw;
    B.up.oh = uh;
    B.up.C = C;
    B.up.dst8 = img + (int64_t)by * stride + (int64_t)bx * C;
    B.up.dstride = stride;
    B.up.clip_w = w - bx;  // composite at (X, Y), clipped to the canvas
    B.up.clip_h = h - by;
    scratch += ((size_t)dw * dh * C * 2 + 255) / 256 * 256;
    plan.push_back(B);
  }
  const size_t ti_bytes = ti.size() * 4, td_off = (ti_bytes + 255) / 256 * 256;
  const size_t sc_off = (td_off + td.size() * 8 + 255) / 256 * 256;
  int rc = ensure(c, &c->pix, sc_off + scratch + 256);
  if (rc) return rc;
  uint8_t *pb = (uint8_t *)c->pix.p;
  rc = ensure_pinned(c, sc_off);
  if (rc) return rc;
  memcpy(c->pinned, ti.data(), ti_bytes);
  memcpy((uint8_t *)c->pinned + td_off, td.data(), td.size() * 8);
  if (sc_off) HIP_TRY(hipMemcpyAsync(pb, c->pinned, sc_off, hipMemcpyHostToDevice, c->stream));
  const int32_t *ai = (const int32_t *)pb;
  const double *ad = (const double *)(pb + td_off);
  for (Box &B : plan) {
    fix_ptr(B.down.dst16, pb + sc_off);
    B.up.src16 = B.down.dst16;
    launch_pix(c->stream, 0, B.down, ai, ad);
    launch_pix(c->stream, 1, B.up, ai, ad);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));  // the pinned lists are reused by the next call
  if (first_bad >= 0) return set_err(FI_EINVAL, "pixelate box %d: %s", first_bad, why.c_str());
  return FI_OK;
}

extern "C" {

int32_t fi_abi_version(void) { return FI_ABI_VERSION; }
// profiling only (not in the public header): k_rs_vm MODE 9 phase sums, 8 u64 per workgroup
int fi_debug_vm_stamps(fi_ctx *c, uint64_t *out, int32_t slots) {
  if (!c || !out) return FI_EINVAL;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return vm_read_stamps(out, slots) == 0 ? FI_OK : FI_EDEVICE;
}
int fi_debug_vr_stamps(fi_ctx *c, uint64_t *out, int32_t slots) {
  if (!c || !out) return FI_EINVAL;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return vr_read_stamps(out, slots) == 0 ? FI_OK : FI_EDEVICE;
}
// Test hook: the -monochrome kernels (fi_mono.hip) on a caller-supplied Q16
// gray image (host buffers), so the parity tests can feed the oracle the
// identical input; out is w x h (rot 0/180) or h x w (rot 90/270), 8-bit.
int fi_debug_monochrome(fi_ctx *c, const uint16_t *gray, int32_t w, int32_t h, int32_t rot, uint8_t *out,
                        int32_t out_stride) {
  if (!c || !gray || !out || w <= 0 || h <= 0) return set_err(FI_EINVAL, "bad arguments");
  if (rot != 0 && rot != 90 && rot != 180 && rot != 270) return set_err(FI_EINVAL, "rot must be 0/90/180/270");
  const int ow = (rot == 90 || rot == 270) ? h : w, oh = (rot == 90 || rot == 270) ? w : h;
  if (out_stride < ow) return set_err(FI_EINVAL, "out_stride too small");
  HIP_TRY(hipSetDevice(c->device));
  const size_t gbytes = (size_t)w * h * 2, obytes = (size_t)out_stride * oh;
  const size_t o_st = (gbytes + 255) / 256 * 256, o_desc = o_st + (sizeof(MonoState) + 255) / 256 * 256,
               o_w = o_desc + 256, o_out = o_w + 256, total = o_out + obytes;
  uint8_t *d = nullptr;
  HIP_TRY(hipMalloc(&d, total));
  MonoDesc md{};
  md.g = (const uint16_t *)d;
  md.w = w;
  md.h = h;
  md.rot = rot;
  md.dst = d + o_out;
  md.dst_stride = out_stride;
  md.st = (MonoState *)(d + o_st);
  volatile double qr1 = 65535.0 + 1.0, span = 16 - 1.0;
  const double step = exp(log((double)qr1) / (double)span);
  double weight = 1.0, wts[16];
  for (int k = 0; k < 16; k++) {
    wts[16 - k - 1] = 1.0 / weight;
    weight *= step;
  }
  int rc = FI_OK;
  if (hipMemcpy(d, gray, gbytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d + o_desc, &md, sizeof(md), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d + o_w, wts, sizeof(wts), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d + o_out, 0, obytes) != hipSuccess) {
    rc = set_err(FI_EDEVICE, "fi_debug_monochrome: upload failed");
  } else {
    launch_mono(c->stream, (const MonoDesc *)(d + o_desc), 1, (const double *)(d + o_w));
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess ||
        hipMemcpy(out, d + o_out, obytes, hipMemcpyDeviceToHost) != hipSuccess)
      rc = set_err(FI_EDEVICE, "fi_debug_monochrome: kernel failed");
  }
  (void)hipFree(d);
  return rc;
}

int fi_debug_convolve(fi_ctx *c, const uint16_t *q16, int32_t w, int32_t h, int32_t ch, const double conv[8],
                      uint32_t ops, uint8_t *out) {
  if (!c || !q16 || !conv || !out || w <= 0 || h <= 0 || (ch != 1 && ch != 3) || (ops & ~7u))
    return set_err(FI_EINVAL, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  std::vector<double> tab, kk;
  std::vector<ConvStep> st[6];
  const size_t qb = (size_t)w * h * ch * 2;
  const size_t o_b = (qb + 255) / 256 * 256, o_out = 2 * o_b, o_tab = o_out + (qb / 2 + 255) / 256 * 256;
  // host side of the steps (device pointers patched below), as run_batch builds them
  ConvStep base{};
  base.W = w;
  base.H = h;
  base.C = ch;
  int cur = 0;  // 0 = buffer A, 1 = B
  struct Pend {
    int stage, in, out, orig;
    ConvStep s;
  };
  std::vector<Pend> pend;
  auto tbl = [&](const std::vector<double> &v) {
    const int32_t off = (int32_t)tab.size();
    tab.insert(tab.end(), v.begin(), v.end());
    return off;
  };
  if (ops & 1) {
    const int kw = im_blur_kernel(conv[0], conv[1], &kk);
    if (kw < 0) return set_err(FI_EUNSUPPORTED, "unsharp kernel too wide");
    ConvStep a = base, b = base;
    a.k = b.k = tbl(kk);
    a.kw = kw, a.kh = 1;
    b.kw = 1, b.kh = kw, b.gain = conv[2], b.thr = 65535.0 * conv[3];
    pend.push_back({0, cur, 1 - cur, -1, a});
    pend.push_back({1, 1 - cur, cur, cur, b});
  }
  if (ops & 2) {
    const int kw = im_sharpen_kernel(conv[4], conv[5], &kk);
    if (kw < 0) return set_err(FI_EUNSUPPORTED, "sharpen kernel too wide");
    ConvStep a = base;
    a.k = tbl(kk);
    a.kw = a.kh = kw;
    pend.push_back({2, cur, 1 - cur, -1, a});
    cur = 1 - cur;
  }
  if (ops & 4) {
    const int kw = im_blur_kernel(conv[6], conv[7], &kk);
    if (kw < 0) return set_err(FI_EUNSUPPORTED, "blur kernel too wide");
    ConvStep a = base, b = base;
    a.k = b.k = tbl(kk);
    a.kw = kw, a.kh = 1;
    b.kw = 1, b.kh = kw;
    pend.push_back({3, cur, 1 - cur, -1, a});
    pend.push_back({4, 1 - cur, cur, -1, b});
  }
  pend.push_back({5, cur, -1, -1, base});
  const size_t o_desc = o_tab + (tab.size() * 8 + 255) / 256 * 256, o_pre = o_desc + pend.size() * 256;
  const size_t total = o_pre + 256;
  uint8_t *d = nullptr;
  HIP_TRY(hipMalloc(&d, total));
  uint16_t *buf[2] = {(uint16_t *)d, (uint16_t *)(d + o_b)};
  int rc = FI_OK;
  const int32_t pre[2] = {0, h};
  if (hipMemcpy(d, q16, qb, hipMemcpyHostToDevice) != hipSuccess ||
      (!tab.empty() && hipMemcpy(d + o_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(d + o_pre, pre, sizeof(pre), hipMemcpyHostToDevice) != hipSuccess)
    rc = set_err(FI_EDEVICE, "fi_debug_convolve: upload failed");
  static const int kMode[6] = {0, 2, 3, 0, 1, 4};
  for (size_t j = 0; rc == FI_OK && j < pend.size(); j++) {
    ConvStep s = pend[j].s;
    s.in = buf[pend[j].in];
    s.out = pend[j].out >= 0 ? buf[pend[j].out] : nullptr;
    s.orig = pend[j].orig >= 0 ? buf[pend[j].orig] : nullptr;
    s.dst8 = d + o_out;
    s.dst_stride = (int64_t)w * ch;
    uint8_t *dd = d + o_desc + 256 * j;
    if (hipMemcpy(dd, &s, sizeof(s), hipMemcpyHostToDevice) != hipSuccess) {
      rc = set_err(FI_EDEVICE, "fi_debug_convolve: upload failed");
      break;
    }
    launch_conv(c->stream, kMode[pend[j].stage], (const ConvStep *)dd, (const int32_t *)(d + o_pre), 1, h,
                (const double *)(d + o_tab));
  }
  if (rc == FI_OK && (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess ||
                      hipMemcpy(out, d + o_out, (size_t)w * h * ch, hipMemcpyDeviceToHost) != hipSuccess))
    rc = set_err(FI_EDEVICE, "fi_debug_convolve: kernel failed");
  (void)hipFree(d);
  return rc;
}

// Test hook: the rotation stage (fi_rotate.hip) on a caller-supplied Q16 HWC
// image, planned as plan_im plans it; ctx NULL: the planner's answer only.
static int debug_rotate(fi_ctx *c, bool host_model, const uint16_t *q16, int32_t w, int32_t h, int32_t ch,
                        int32_t degrees, uint32_t background, uint16_t *out_q16, uint8_t *out8, int32_t *out_w,
                        int32_t *out_h) {
  if (w <= 0 || h <= 0 || (ch != 1 && ch != 3) || !out_w || !out_h) return set_err(FI_EINVAL, "bad arguments");
  ShearPlan S;
  plan_rotate_angle(degrees, &S);
  const int rot = S.rot;
  const int iw = (rot == 90 || rot == 270) ? h : w, ih = (rot == 90 || rot == 270) ? w : h;
  *out_w = iw;
  *out_h = ih;
  if (S.on) {
    if (!plan_shear(iw, ih, &S)) return set_err(FI_EUNSUPPORTED, "-rotate: the rotated image is empty or too large");
    if (!S.contained) return set_err(FI_EUNSUPPORTED, "-rotate: shear leaves IM's canvas (tall, narrow image)");
    *out_w = S.cw;
    *out_h = S.ch;
  }
  if (!c && !host_model) return FI_OK;
  if (!q16) return set_err(FI_EINVAL, "bad arguments");
  // IntegralRotateImage on the host (the resample epilogue's job in a batch)
  std::vector<uint16_t> I((size_t)iw * ih * ch);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      int dx = x, dy = y;
      if (rot == 90) dx = h - 1 - y, dy = x;
      if (rot == 180) dx = w - 1 - x, dy = h - 1 - y;
      if (rot == 270) dx = y, dy = w - 1 - x;
      for (int k = 0; k < ch; k++) I[((size_t)dy * iw + dx) * ch + k] = q16[((size_t)y * w + x) * ch + k];
    }
  const size_t ob = (size_t)*out_w * *out_h * ch;
  if (!S.on) {
    if (out_q16) memcpy(out_q16, I.data(), ob * 2);
    if (out8)
      for (size_t e = 0; e < ob; e++) out8[e] = (uint8_t)(((I[e] + 128u) - ((I[e] + 128u) >> 8)) >> 8);
    return FI_OK;
  }
  if (host_model) {
    RotDesc r{};
    r.src = I.data();
    r.w = iw, r.h = ih, r.C = ch;
    r.bx = S.bx, r.by = S.by, r.cols = S.cols, r.rows = S.rows;
    for (int k = 0; k < 3; k++) r.sh[k] = S.sh[k];
    r.cx = S.cx, r.cy = S.cy, r.cw = S.cw, r.ch = S.ch;
    for (int k = 0; k < 3; k++) r.bg[k] = (uint16_t)(257u * ((background >> (16 - 8 * k)) & 255u));
    r.dst16 = out_q16;
    r.dst8 = out8;
    r.stride16 = r.stride8 = (int64_t)S.cw * ch;
    rot_host(r);
    return FI_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  const size_t qb = I.size() * 2;
  const size_t o_q = (qb + 255) / 256 * 256, o_8 = o_q + (ob * 2 + 255) / 256 * 256,
               o_desc = o_8 + (ob + 255) / 256 * 256, o_pre = o_desc + (sizeof(RotDesc) + 255) / 256 * 256,
               total = o_pre + 256;
  uint8_t *d = nullptr;
  HIP_TRY(hipMalloc(&d, total));
  RotDesc r{};
  r.src = (const uint16_t *)d;
  r.w = iw, r.h = ih, r.C = ch;
  r.bx = S.bx, r.by = S.by, r.cols = S.cols, r.rows = S.rows;
  for (int k = 0; k < 3; k++) r.sh[k] = S.sh[k];
  r.cx = S.cx, r.cy = S.cy, r.cw = S.cw, r.ch = S.ch;
  for (int k = 0; k < 3; k++) r.bg[k] = (uint16_t)(257u * ((background >> (16 - 8 * k)) & 255u));
  r.dst16 = (uint16_t *)(d + o_q);
  r.stride16 = (int64_t)S.cw * ch;
  r.dst8 = d + o_8;
  r.stride8 = (int64_t)S.cw * ch;
  const int32_t pre[2] = {0, rot_tiles(S.cw, S.ch)};
  int rc = FI_OK;
  if (hipMemcpy(d, I.data(), qb, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d + o_desc, &r, sizeof(r), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d + o_pre, pre, sizeof(pre), hipMemcpyHostToDevice) != hipSuccess) {
    rc = set_err(FI_EDEVICE, "fi_debug_rotate: upload failed");
  } else {
    launch_rot(c->stream, (const RotDesc *)(d + o_desc), (const int32_t *)(d + o_pre), 1, pre[1]);
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess ||
        (out_q16 && hipMemcpy(out_q16, d + o_q, ob * 2, hipMemcpyDeviceToHost) != hipSuccess) ||
        (out8 && hipMemcpy(out8, d + o_8, ob, hipMemcpyDeviceToHost) != hipSuccess))
      rc = set_err(FI_EDEVICE, "fi_debug_rotate: kernel failed");
  }
  (void)hipFree(d);
  return rc;
}

int fi_debug_rotate(fi_ctx *c, const uint16_t *q16, int32_t w, int32_t h, int32_t ch, int32_t degrees,
                    uint32_t background, uint16_t *out_q16, uint8_t *out8, int32_t *out_w, int32_t *out_h) {
  return debug_rotate(c, false, q16, w, h, ch, degrees, background, out_q16, out8, out_w, out_h);
}
// The same with the kernel's per-pixel procedure run on the host (no GPU).
int fi_debug_rotate_host(const uint16_t *q16, int32_t w, int32_t h, int32_t ch, int32_t degrees,
                         uint32_t background, uint16_t *out_q16, uint8_t *out8, int32_t *out_w, int32_t *out_h) {
  return debug_rotate(nullptr, true, q16, w, h, ch, degrees, background, out_q16, out8, out_w, out_h);
}

int fi_plan(fi_image *imgs, int32_t n) {
  if (n < 0 || (n > 0 && !imgs)) return set_err(FI_EINVAL, "bad image array");
  int first = FI_OK;
  for (int i = 0; i < n; i++) {
    ImPlan p;
    const int rc = plan_im(imgs[i], &p);
    imgs[i].status = rc;
    if (rc == FI_OK) {
      imgs[i].out_w = p.out_w;
      imgs[i].out_h = p.out_h;
      imgs[i].out_channels = p.out_c;
      imgs[i].out_stride = p.out_w * p.out_c;
    } else if (first == FI_OK) {
      first = set_err(rc, "image %d: %s", i, p.err.c_str());
    }
  }
  return first;
}

int fi_pixelate_regions_device(fi_ctx *c, uint8_t *img, int32_t w, int32_t h, int32_t stride, int32_t channels,
                               const int32_t *boxes, int32_t nboxes) {
  if (!c) return set_err(FI_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  // stream-ordered after earlier batches, including their crop applies on ap_stream
  if (order_after_apply(c) != FI_OK) return set_err(FI_EDEVICE, "hipStreamWaitEvent failed");
  return pixelate_device(c, img, w, h, stride, channels, boxes, nboxes);
}

int fi_pixelate_regions(fi_ctx *c, uint8_t *img, int32_t w, int32_t h, int32_t stride, int32_t channels,
                        const int32_t *boxes, int32_t nboxes) {
  if (!c || !img || w <= 0 || h <= 0 || (channels != 1 && channels != 3) || stride < w * channels)
    return set_err(FI_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  {
    const int rc0 = drain(c);  // the io buffer may be read by in-flight batches
    if (rc0) return rc0;
  }
  const int64_t pitch = (int64_t)w * channels;
  int rc = ensure(c, &c->io, (size_t)pitch * h + 256);
  if (rc) return rc;
  uint8_t *d = (uint8_t *)c->io.p;
  HIP_TRY(hipMemcpy2DAsync(d, pitch, img, stride, pitch, h, hipMemcpyHostToDevice, c->stream));
  rc = pixelate_device(c, d, w, h, pitch, channels, boxes, nboxes);
  // boxes before a rejected one are applied (each face is its own mogrify run)
  HIP_TRY(hipMemcpy2DAsync(img, stride, d, pitch, pitch, h, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

int fi_plan_bytes(const fi_image *imgs, int32_t n, int64_t *bytes) {
  if (n < 0 || (n > 0 && (!imgs || !bytes))) return set_err(FI_EINVAL, "bad arguments");
  int first = FI_OK;
  for (int i = 0; i < n; i++) {
    ImPlan p;
    const int rc = plan_im(imgs[i], &p);
    if (rc != FI_OK) {
      bytes[i] = -1;
      if (first == FI_OK) first = set_err(rc, "image %d: %s", i, p.err.c_str());
      continue;
    }
    int64_t rows = p.eh;  // no resample: the extent window's rows are copied
    if (p.resize) {
      AxisTable t;
      build_axis(p.filter, p.yf, p.sh, p.th, p.ey0, p.ey0 + p.eh, p.sample, p.H, &t);
      rows = t.touched;
    }
    bytes[i] = rows * (int64_t)p.W * p.C + (int64_t)p.out_w * p.out_h * p.out_c +
               ((imgs[i].flags & FI_OP_SMARTCROP) ? 16 : 0);
    // a shear rotation reads the integral Q16 image once and writes the output above
    if (p.shear.on) bytes[i] += (int64_t)p.iw * p.ih * p.out_c * 2;
  }
  return first;
}

}  // extern "C"
