// fi_rs_plan.cpp -- the batch planner of the runtime (fi_runtime.h): per image
// the geometry, descriptor, resample path and tables; the batch's smartcrop
// stage, workspace pointers and upload blob.  plan_batch and place_batch are
// the whole of it, for run_batch and for the host-only hook alike.
//   plan_image (per image: geometry, descriptor, resample path + tables)
//   -> plan_batch_sc (smartcrop stage) -> resolve_workspace (device pointers,
//   rotation / -monochrome / convolution steps, crop apply) -> build_vm_tiles (k_rs_vr /
//   k_rs_vm) / build_hv_tiles (fi_tiles.cpp) -> pack_batch (one blob)
#include "fi_runtime.h"

using namespace fi;

static const AxisTable *add_axis(fi_ctx *c, Exec &E, int filter, double factor, int in_sampled, int out_size,
                                 int o0, int o1, bool sample, int in_src, DevAxis *out,
                                 HashMap<const AxisTable *, DevAxis> &placed) {
  auto key = std::make_tuple(filter, dbits(factor), in_sampled, out_size, o0, o1, (int)sample, in_src);
  auto it = c->axis_cache.find(key);
  if (it == c->axis_cache.end()) {
    AxisTable t;
    build_axis(filter, factor, in_sampled, out_size, o0, o1, sample, in_src, &t);
    it = c->axis_cache.emplace(key, std::move(t)).first;
  }
  const AxisTable *t = &it->second;
  (void)placed;
  auto pit = c->axis_at.find(t);
  if (pit != c->axis_at.end()) {
    *out = pit->second;
    return t;
  }
  DevAxis d{};
  d.n = (int32_t)t->start.size();
  d.start = E.oi();
  E.ai.insert(E.ai.end(), t->start.begin(), t->start.end());
  d.count = E.oi();
  E.ai.insert(E.ai.end(), t->count.begin(), t->count.end());
  d.woff = E.oi();
  const int32_t wbase = E.of();
  for (int32_t w : t->woff) E.ai.push_back(w + wbase);
  E.af.insert(E.af.end(), t->w.begin(), t->w.end());
  d.maxtaps = t->maxtaps;
  d.src_lo = t->src_lo;
  d.src_hi = t->src_hi;
  d.touched = t->touched;
  d.wbase = wbase;
  d.wd = -1;
  c->axis_at[t] = d;
  *out = d;
  return t;
}

// The f64 weights of an axis (RGBA path), placed in the double heap once.
static void add_axis_f64(fi_ctx *c, Exec &E, const AxisTable *t, DevAxis *d) {
  auto it = c->axis_wd_at.find(t);
  if (it == c->axis_wd_at.end()) {
    const int32_t off = E.od();
    E.ad.insert(E.ad.end(), t->wd.begin(), t->wd.end());
    it = c->axis_wd_at.emplace(t, off).first;
  }
  d->wd = it->second;
}

// The k_rs_vm column strips of a horizontal table: <= kVmMaxNx output px,
// narrower when the strip's horizontal fragments would not leave room for two
// workgroups per CU (nullptr: no strip width fits).
static const MfmaH *vm_strips(fi_ctx *c, const AxisTable *ht, bool q16) {
  auto hit = c->vmh_cache.find({ht, q16});
  if (hit == c->vmh_cache.end()) {
    MfmaH m;
    const int first_nx = kVmMaxNx;
    for (int mx : {first_nx, 48, 32}) {
      if (!build_mfma_h(*ht, &m, mx)) {
        m = MfmaH();
        break;
      }
      bool fits = true, wide = false;
      for (const MfmaStrip &st : m.strips) {
        fits = fits && vm_lds_bytes(st.vpitch, st.nocb, st.ks, q16) <= kVmMaxLds;
        wide = wide || st.nocb > 3;
      }
      // strips of four 16-px blocks (factors below ~2.7) at 48 px instead, so
      // k_rs_vr (<= 3 blocks a strip) takes the image (FI_VR_NARROW=0: keep 64)
      if (fits && wide && c->vr_narrow && c->vr_rs && mx == first_nx) {
        MfmaH n;
        bool nfits = build_mfma_h(*ht, &n, 48);
        for (const MfmaStrip &st : n.strips) nfits = nfits && vm_lds_bytes(st.vpitch, st.nocb, st.ks, q16) <= kVmMaxLds;
        if (nfits && !n.strips.empty()) m = std::move(n);
      }
      if (fits) break;
      m = MfmaH();
    }
    hit = c->vmh_cache.emplace(std::make_pair(ht, q16), std::move(m)).first;
  }
  return hit->second.strips.empty() ? nullptr : &hit->second;
}

// Choose the resample kernel of one image (d.mode) and add its tables:
//   5  k_rs_vr / k_rs_vm: RGB, vertical first, 16-byte aligned rows (the
//      default; build_vm_tiles picks the kernel);
//   6  k_rs_hv: RGB, horizontal first, contiguous taps, 16-byte aligned rows;
//   1 / 2  the generic two-pass kernels, vertical / horizontal first (RGBA,
//      convolution inputs, unaligned sources, tables that do not fit).
// Returns the algorithmic source bytes the path reads.
static int64_t plan_resample(fi_ctx *c, Exec &E, BatchPlan &Bp, const ImPlan &P, const fi_image &im,
                             ResizeDesc &d) {
  const AxisTable *vt = add_axis(c, E, P.filter, P.yf, P.sh, P.th, P.ey0, P.ey0 + P.eh, P.sample, P.H, &d.v, Bp.placed);
  const AxisTable *ht = add_axis(c, E, P.filter, P.xf, P.sw, P.tw, P.ex0, P.ex0 + P.ew, P.sample, P.W, &d.h, Bp.placed);
  const bool rgb = P.C == 3;
  const bool fast_ok = rgb && !P.conv && !P.shear.on;  // the streaming kernels write 8-bit only
  if (!rgb) {
    // matte (RGBA) images: the alpha-weighted f64 generic passes (k_rs4_*)
    add_axis_f64(c, E, vt, &d.v);
    add_axis_f64(c, E, ht, &d.h);
  }
  const bool aligned16 = ((uintptr_t)im.src % 16) == 0 && (im.src_stride % 16) == 0;
  const int64_t strip_bytes = (int64_t)vt->touched * (d.h.src_hi - d.h.src_lo) * 3;
  const bool vfirst_fast = fast_ok && !P.hfirst && c->fast_rs && aligned16;
  if (vfirst_fast) {
    auto vit = c->vmv_cache.find(vt);
    if (vit == c->vmv_cache.end()) {
      VmV m;
      if (!build_vm_v(*vt, &m)) m = VmV();
      vit = c->vmv_cache.emplace(vt, std::move(m)).first;
    }
    // the Q16 output tile (gray / rotation) needs more LDS than the 8-bit one
    const MfmaH *hh = vm_strips(c, ht, P.gray || P.rot != 0);
    if (vit->second.nblk > 0 && hh) {
      d.mode = 5;  // streaming exact-integer MFMA, vertical first
      Bp.vm_img.push_back((int)Bp.rd.size());
      Bp.vm_v.push_back(&vit->second);
      Bp.vm_h.push_back(hh);
      Bp.vm_vt.push_back(vt);
      return strip_bytes;
    }
  }
  // horizontal first: contiguous tap ranges (no sample pre-step), 16-byte aligned rows
  if (fast_ok && P.hfirst && !P.sample && c->fast_rs && aligned16) {
    auto vit = c->hvv_cache.find(vt);
    if (vit == c->hvv_cache.end()) {
      HvV m;
      if (!build_hv_v(*vt, &m)) m = HvV();
      vit = c->hvv_cache.emplace(vt, std::move(m)).first;
    }
    auto hit = c->hvh_cache.find(ht);
    if (hit == c->hvh_cache.end()) {
      HvH m;
      if (!build_hv_h(*ht, &m)) m = HvH();
      for (const HvStrip &st : m.strips)
        if (hv_lds_bytes(st.pp, st.nocb) > kVmMaxLds) m = HvH();
      hit = c->hvh_cache.emplace(ht, std::move(m)).first;
    }
    if (vit->second.nblk > 0 && !hit->second.strips.empty()) {
      d.mode = 6;  // streaming exact-integer MFMA, horizontal first
      Bp.hv_img.push_back((int)Bp.rd.size());
      Bp.hv_v.push_back(&vit->second);
      Bp.hv_h.push_back(&hit->second);
      Bp.hv_W.push_back(P.W);
      int64_t cols = 0;
      for (const HvStrip &st : hit->second.strips) cols += std::min(st.pp, P.W - st.px0);
      return (int64_t)vit->second.nrows * cols * 3;
    }
  }
  if (!rgb && !P.hfirst) {
    d.mode = 1;  // RGBA: mid = [eh][source columns src_lo..src_hi) x 4 Q16
    d.mid_c0 = d.h.src_lo;
    d.mid_cols = d.h.src_hi - d.h.src_lo;
    d.mid_rows = P.eh;
    d.mid_stride = 4 * (int64_t)d.mid_cols;
  } else if (!rgb) {
    d.mode = 2;  // RGBA: mid = [source rows src_lo..src_hi][ew] x 4 Q16
    d.mid_r0 = d.v.src_lo;
    d.mid_rows = d.v.src_hi - d.v.src_lo;
    d.mid_cols = P.ew;
    d.mid_stride = 4 * (int64_t)P.ew;
  } else if (!P.hfirst) {
    d.mode = 1;
    const int64_t b_lo = (int64_t)3 * d.h.src_lo / 8 * 8;
    const int64_t b_hi = std::min<int64_t>((int64_t)3 * P.W, ((int64_t)3 * d.h.src_hi + 7) / 8 * 8);
    d.mid_c0 = (int32_t)b_lo;
    d.mid_cols = (int32_t)(b_hi - b_lo);
    d.mid_rows = P.eh;
    d.mid_stride = (d.mid_cols + 7) / 8 * 8;
  } else {
    d.mode = 2;
    d.mid_r0 = d.v.src_lo;
    d.mid_rows = d.v.src_hi - d.v.src_lo;
    d.mid_cols = P.ew;
    d.mid_stride = (3 * P.ew + 7) / 8 * 8;
    // k_rs_h_tile LDS row pitch: the source bytes of a 256-column chunk's windows
    for (int x0 = 0; x0 < P.ew; x0 += 256) {
      const int x1 = std::min(P.ew, x0 + 256);
      const int lo = ht->start[x0], hi = ht->start[x1 - 1] + ht->count[x1 - 1];
      Bp.h_tile_pitch = std::max(Bp.h_tile_pitch, (3 * (hi - lo) + 8 + 15) / 16 * 16);
      Bp.h_tile_taps = std::max(Bp.h_tile_taps, (int)d.h.maxtaps);
    }
  }
  d.mid = (uint16_t *)(uintptr_t)(E.work.take((size_t)d.mid_stride * d.mid_rows * 2) + 1);
  return (int64_t)vt->touched * (d.h.src_hi - d.h.src_lo) * P.C;
}

// Plan image i: geometry (plan_im), output record, the resample descriptor
// and its destination (dst, the apply / -monochrome / convolution workspace),
// and its smartcrop job.  Failures go to the image's status.
static void plan_image(fi_ctx *c, Exec &E, BatchPlan &Bp, int i) {
  fi_image &im = Bp.imgs[i];
  ImPlan &P = Bp.plans[i];
  const int rc = plan_im(im, &P);
  if (rc != FI_OK) {
    Bp.status[i] = rc;
    Bp.errs[i] = P.err;
    return;
  }
  if (!im.src) {
    Bp.status[i] = FI_EINVAL;
    Bp.errs[i] = "src is NULL";
    return;
  }
  const bool smc = (im.flags & FI_OP_SMARTCROP) != 0;
  const bool apply = smc && (im.flags & FI_OP_SMARTCROP_APPLY);
  im.out_w = P.out_w;
  im.out_h = P.out_h;
  im.out_channels = P.out_c;
  im.out_stride = P.out_w * P.out_c;
  const int64_t need = (int64_t)im.out_stride * im.out_h;
  if (!im.dst || im.dst_capacity < need) {
    Bp.status[i] = FI_ECAPACITY;
    Bp.errs[i] = "dst NULL or dst_capacity < out_stride*out_h";
    return;
  }
  ResizeDesc d{};
  d.src = im.src;
  d.src_stride = im.src_stride;
  d.C = P.C;
  d.ew = P.ew;
  d.eh = P.eh;
  d.ex0 = P.ex0;
  d.ey0 = P.ey0;
  d.gray = P.gray;
  d.rot = P.rot;
  d.out_w = P.iw;  // (the integral rotation's dims: a shear rotation follows it in its own stage)
  d.out_h = P.ih;
  d.out_c = P.out_c;
  d.dst_stride = im.out_stride;
  Bp.res_stride[i] = im.out_stride;
  if (apply) {
    // the resized image stays in the workspace for smartcrop and the crop
    // apply: rows padded to res_align bytes, so the readers' 16-byte loads
    // are aligned (the -monochrome and convolution outputs keep out_stride)
    if (!P.mono && !P.conv) {
      const int64_t a = c->res_align;
      Bp.res_stride[i] = d.dst_stride = (im.out_stride + a - 1) / a * a;
    }
    Bp.res_off[i] = E.work.take((size_t)(Bp.res_stride[i] * im.out_h));
    d.dst = (uint8_t *)(uintptr_t)(Bp.res_off[i] + 1);  // workspace, resolved later
  } else {
    d.dst = im.dst;
  }
  Bp.out_of[i] = d.dst;
  if (P.mono) {
    // the resample epilogue writes the extent window's Q16 gray, unrotated;
    // fi_mono.hip quantizes it and writes the rotated 0/255 output
    MonoItem m;
    m.img = i;
    m.g_off = E.work.take((size_t)P.ew * P.eh * 2);
    m.st_off = E.work.take(sizeof(MonoState));
    Bp.mono.push_back(m);
    d.dst = (uint8_t *)(uintptr_t)(m.g_off + 1);
    d.dst_stride = (int64_t)P.ew * 2;
    d.gray = 2;
    d.rot = 0;
  }
  if (P.conv) {
    // the epilogue writes the rotated Q16 image; the convolutions ping-pong
    // between two such buffers and the last step writes the 8-bit output
    ConvItem ci;
    ci.img = i;
    const size_t qb = (size_t)P.out_w * P.out_h * P.out_c * 2;
    ci.a_off = E.work.take(qb);
    ci.b_off = E.work.take(qb);
    Bp.conv_items.push_back(ci);
    d.dst = (uint8_t *)(uintptr_t)(ci.a_off + 1);
    d.dst_stride = (int64_t)P.out_w * P.out_c * 2;
    d.q16out = 1;
  }
  if (P.shear.on) {
    // the epilogue writes the integrally rotated Q16 image; fi_rotate.hip
    // shears it into the 8-bit output (dst or the apply's workspace copy) or
    // into the convolutions' first Q16 buffer
    RotItem ri;
    ri.img = i;
    ri.q_off = E.work.take((size_t)P.iw * P.ih * P.out_c * 2);
    ri.conv = P.conv ? (int)Bp.conv_items.size() - 1 : -1;
    Bp.rot_items.push_back(ri);
    d.dst = (uint8_t *)(uintptr_t)(ri.q_off + 1);
    d.dst_stride = (int64_t)P.iw * P.out_c * 2;
    d.q16out = 1;
    Bp.rot_bytes += (double)P.iw * P.ih * P.out_c * 2 + (double)need * (P.conv ? 2 : 1);
  }
  int64_t src_bytes;
  if (!P.resize) {
    d.mode = 0;
    src_bytes = (int64_t)P.ew * P.eh * P.C;
  } else {
    src_bytes = plan_resample(c, E, Bp, P, im, d);
  }
  Bp.resize_bytes += (double)src_bytes + (double)need;
  static const char *kPath[7] = {"path_copy", "path_generic_v", "path_generic_h", "path_none", "path_none",
                                 "path_vm", "path_hv"};
  c->stats[kPath[d.mode]].launches += 1;  // images per resample path (fi_kernel_stats)
  Bp.rd_of[i] = (int)Bp.rd.size();
  Bp.rd.push_back(d);
  if (smc) {
    ScItem it{};
    it.img = nullptr;  // the resized image: resolved with the workspace
    it.stride = Bp.res_stride[i];
    it.W = P.out_w;
    it.H = P.out_h;
    it.C = P.out_c;
    it.tw = im.smartcrop_w > 0 ? im.smartcrop_w : 100;
    it.th = im.smartcrop_h > 0 ? im.smartcrop_h : 100;
    it.result = (int)Bp.sitems.size();
    it.padded = apply && Bp.res_stride[i] % 16 == 0;  // workspace rows at a 16-B rounded pitch
    fi_smartcrop_default_options(&it.opt);
    Bp.sc_of[i] = (int)Bp.sitems.size();
    Bp.sitems.push_back(it);
  }
}

// The smartcrop stage of the batch: input = each image's resized output.
static void plan_batch_sc(fi_ctx *c, Exec &E, BatchPlan &Bp) {
  Bp.sstatus.assign(Bp.sitems.size(), FI_OK);
  Bp.serrs.assign(Bp.sitems.size(), std::string());
  for (int i = 0; i < Bp.n; i++)
    if (Bp.sc_of[i] >= 0) Bp.sitems[Bp.sc_of[i]].img = Bp.out_of[i];  // may be +1-tagged workspace
  plan_smartcrop(c, E, Bp.sitems, &Bp.SL, &Bp.sstatus, &Bp.serrs, false);
  Bp.results_off = E.work.take(sizeof(ScResult) * std::max<size_t>(Bp.sitems.size(), 1));
  Bp.scores_off = E.work.take(sizeof(CropScore) * std::max(Bp.SL.nscores, 1));
  Bp.outwh_off = E.work.take(sizeof(int32_t) * 2 * std::max(Bp.n, 1));
}

// Resolve the +1-tagged workspace offsets against the slot's workspace wb and
// build what needs device pointers: -monochrome descriptors, the forwarded
// convolution steps (per image in IM's order: unsharp, sharpen, blur; one
// launch per stage), the smartcrop descriptors' buffers and crop apply.
static void resolve_workspace(Exec &E, BatchPlan &Bp, uint8_t *wb) {
  fi_image *imgs = Bp.imgs;
  for (int i = 0; i < Bp.n; i++) {
    if (Bp.rd_of[i] < 0) continue;
    ResizeDesc &d = Bp.rd[Bp.rd_of[i]];
    if (d.mid) fix_ptr(d.mid, wb);
    const bool apply = (imgs[i].flags & FI_OP_SMARTCROP) && (imgs[i].flags & FI_OP_SMARTCROP_APPLY);
    if (apply) fix_ptr(Bp.out_of[i], wb);
    if (d.gray == 2 || d.q16out)
      fix_ptr(d.dst, wb);
    else
      d.dst = Bp.out_of[i];
  }
  for (const MonoItem &m : Bp.mono) {
    const ResizeDesc &d = Bp.rd[Bp.rd_of[m.img]];
    MonoDesc md{};
    md.g = (const uint16_t *)(wb + m.g_off);
    md.w = d.ew;
    md.h = d.eh;
    md.rot = Bp.plans[m.img].rot;
    md.dst = Bp.out_of[m.img];
    md.dst_stride = imgs[m.img].out_stride;
    md.st = (MonoState *)(wb + m.st_off);
    Bp.mdesc_mono.push_back(md);
  }
  for (const RotItem &ri : Bp.rot_items) {
    const ImPlan &P = Bp.plans[ri.img];
    const ShearPlan &S = P.shear;
    RotDesc r{};
    r.src = (const uint16_t *)(wb + ri.q_off);
    r.w = S.w, r.h = S.h, r.C = P.out_c;
    r.bx = S.bx, r.by = S.by, r.cols = S.cols, r.rows = S.rows;
    for (int k = 0; k < 3; k++) r.sh[k] = S.sh[k];
    r.cx = S.cx, r.cy = S.cy, r.cw = S.cw, r.ch = S.ch;
    // Q16 = 257 * the 8-bit channel (ScaleCharToQuantum); Gray: R = G = B (plan_im)
    for (int k = 0; k < 3; k++) r.bg[k] = (uint16_t)(257u * ((P.bg >> (16 - 8 * k)) & 255u));
    if (ri.conv >= 0) {
      r.dst16 = (uint16_t *)(wb + Bp.conv_items[ri.conv].a_off);
      r.stride16 = (int64_t)P.out_w * P.out_c;
    } else {
      r.dst8 = Bp.out_of[ri.img];
      r.stride8 = Bp.res_stride[ri.img];
    }
    Bp.rdesc_rot.push_back(r);
  }
  for (const ConvItem &ci : Bp.conv_items) {
    const ImPlan &P = Bp.plans[ci.img];
    uint16_t *A = (uint16_t *)(wb + ci.a_off), *Bf = (uint16_t *)(wb + ci.b_off);
    uint16_t *cur = A, *oth = Bf;
    ConvStep base{};
    base.W = P.out_w;
    base.H = P.out_h;
    base.C = P.out_c;
    std::vector<double> kk;
    auto table = [&](const std::vector<double> &v) {
      const int32_t off = E.od();
      E.ad.insert(E.ad.end(), v.begin(), v.end());
      return off;
    };
    if (P.conv & 1) {
      const int w = im_blur_kernel(P.cv[0], P.cv[1], &kk);
      ConvStep h = base, v = base;
      h.k = v.k = table(kk);
      h.kw = w, h.kh = 1, h.in = cur, h.out = oth;
      v.kw = 1, v.kh = w, v.in = oth, v.orig = cur, v.out = cur;
      v.gain = P.cv[2];
      v.thr = 65535.0 * P.cv[3];
      Bp.cst[0].push_back(h);
      Bp.cst[1].push_back(v);
    }
    if (P.conv & 2) {
      const int w = im_sharpen_kernel(P.cv[4], P.cv[5], &kk);
      ConvStep t = base;
      t.k = table(kk);
      t.kw = t.kh = w, t.in = cur, t.out = oth;
      Bp.cst[2].push_back(t);
      std::swap(cur, oth);
    }
    if (P.conv & 4) {
      const int w = im_blur_kernel(P.cv[6], P.cv[7], &kk);
      ConvStep h = base, v = base;
      h.k = v.k = table(kk);
      h.kw = w, h.kh = 1, h.in = cur, h.out = oth;
      v.kw = 1, v.kh = w, v.in = oth, v.out = cur;
      Bp.cst[3].push_back(h);
      Bp.cst[4].push_back(v);
    }
    ConvStep f = base;
    f.in = cur;
    f.dst8 = Bp.out_of[ci.img];
    f.dst_stride = imgs[ci.img].out_stride;
    Bp.cst[5].push_back(f);
  }
  for (ScDesc &d : Bp.SL.descs) {
    fix_ptr(d.red, wb);
    fix_ptr(d.hbuf, wb);
    fix_ptr(d.tbuf, wb);
    fix_ptr(d.pre, wb);
    fix_ptr(d.maps, wb);
  }
  for (int i = 0; i < Bp.n; i++)
    if (Bp.sc_of[i] >= 0) Bp.SL.descs[Bp.sc_of[i]].img = Bp.out_of[i];
  for (int i = 0; i < Bp.n; i++) {
    if (Bp.rd_of[i] < 0 || Bp.sc_of[i] < 0) continue;
    if (!(imgs[i].flags & FI_OP_SMARTCROP_APPLY)) continue;
    if (Bp.sstatus[Bp.sc_of[i]] != FI_OK) continue;
    const ResizeDesc &d = Bp.rd[Bp.rd_of[i]];
    ApplyDesc a{};
    a.src = Bp.out_of[i];
    a.src_stride = Bp.res_stride[i];
    a.W = Bp.plans[i].out_w;
    a.H = Bp.plans[i].out_h;
    a.C = d.out_c;
    a.result = Bp.sc_of[i];
    a.crop0 = Bp.SL.descs[Bp.sc_of[i]].crop0;
    a.dst = imgs[i].dst;
    a.out_wh = (int32_t *)(wb + Bp.outwh_off + 8 * (size_t)i);
    Bp.apply.push_back(a);
  }
}

// Pack descriptors, tiles, launch lists and the batch's new heap tables into
// the upload blob E.blob.
static void pack_batch(fi_ctx *c, Exec &E, BatchPlan &Bp, Packed &K) {
  Blob &B = E.blob;
  // one allocation for the whole blob (no regrowth copies of megabytes of tiles)
  auto bytes = [](const auto &v) { return v.size() * sizeof(v[0]) + 256; };
  B.b.reserve(B.b.size() + bytes(Bp.rd) + bytes(Bp.vdescs) + bytes(Bp.vstrips) + bytes(Bp.vtiles) +
              bytes(Bp.vrtiles) + bytes(Bp.vr_info) + bytes(Bp.hdescs) + bytes(Bp.hstrips) + bytes(Bp.htiles) +
              bytes(Bp.apply) + bytes(E.ai) + bytes(E.af) + bytes(E.ad) + 32 * sizeof(int32_t) * Bp.rd.size() +
              ((size_t)1 << 20));
  std::vector<int> m0, m1, m2, q0, q1, q2;  // q*: RGBA (matte) images of modes 0 / 1 / 2
  for (size_t k = 0; k < Bp.rd.size(); k++) {
    if (Bp.rd[k].mode >= 3) continue;
    if (Bp.rd[k].C == 4)
      (Bp.rd[k].mode == 0 ? q0 : Bp.rd[k].mode == 1 ? q1 : q2).push_back((int)k);
    else
      (Bp.rd[k].mode == 0 ? m0 : Bp.rd[k].mode == 1 ? m1 : m2).push_back((int)k);
  }
  K.all_rd_off = B.addv(Bp.rd);
  K.vdesc_off = B.addv(Bp.vdescs);
  K.vstrip_off = B.addv(Bp.vstrips);
  K.vtile_off = B.addv(Bp.vtiles);
  K.vrtile_off = B.addv(Bp.vrtiles);
  K.vrinfo_off = B.addv(Bp.vr_info);
  K.hdesc_off = B.addv(Bp.hdescs);
  K.hstrip_off = B.addv(Bp.hstrips);
  K.htile_off = B.addv(Bp.htiles);
  auto eh_tiles = [](const ResizeDesc &d) { return d.eh; };
  auto mid_tiles = [](const ResizeDesc &d) { return d.mid_rows; };
  K.L0 = add_launch(B, Bp.rd, m0, eh_tiles);
  K.L1a = add_launch(B, Bp.rd, m1, eh_tiles);
  K.h_tiled = rs_h_tile_lds(Bp.h_tile_pitch, Bp.h_tile_taps) <= 64 * 1024;
  K.L2a = K.h_tiled ? add_launch(B, Bp.rd, m2, [](const ResizeDesc &d) {
    return ((d.mid_rows + kHTileRows - 1) / kHTileRows) * ((d.ew + 255) / 256);
  }) : add_launch(B, Bp.rd, m2, mid_tiles);
  K.L2b = add_launch(B, Bp.rd, m2, eh_tiles);
  K.Q0 = add_launch(B, Bp.rd, q0, eh_tiles);
  K.Q1a = add_launch(B, Bp.rd, q1, eh_tiles);
  K.Q2a = add_launch(B, Bp.rd, q2, mid_tiles);
  K.Q2b = add_launch(B, Bp.rd, q2, eh_tiles);
  add_sc_launches(c, B, Bp.SL, Bp.sstatus, &K.SX);
  K.apply_off = B.addv(Bp.apply);
  K.mono_off = B.addv(Bp.mdesc_mono);
  for (int k = 0; k < 6; k++) {
    std::vector<int> all(Bp.cst[k].size());
    for (size_t j = 0; j < all.size(); j++) all[j] = (int)j;
    K.CL[k] = add_launch(B, Bp.cst[k], all, [](const ConvStep &st) { return st.H; });
  }
  if (!Bp.rdesc_rot.empty()) {  // (nothing is placed for a batch without a sheared image)
    std::vector<int> all(Bp.rdesc_rot.size());
    for (size_t j = 0; j < all.size(); j++) all[j] = (int)j;
    K.RL = add_launch(B, Bp.rdesc_rot, all, [](const RotDesc &r) { return rot_tiles(r.cw, r.ch); });
  }
  if (!Bp.mono.empty() && c->mono_wts_at >= 0) K.mono_wts = (size_t)c->mono_wts_at;
  if (!Bp.mono.empty() && c->mono_wts_at < 0) {
    // the Riemersma error-queue weights (quantize.c), computed with libm at run
    // time exactly as oracle/fi_oracle.c does
    K.mono_wts = (size_t)E.od();
    c->mono_wts_at = (int32_t)K.mono_wts;
    volatile double qr1 = 65535.0 + 1.0, span = 16 - 1.0;
    const double step = exp(log((double)qr1) / (double)span);
    double weight = 1.0, wts[16];
    for (int k = 0; k < 16; k++) {
      wts[16 - k - 1] = 1.0 / weight;
      weight *= step;
    }
    E.ad.insert(E.ad.end(), wts, wts + 16);
  }
  K.ai_off = B.addv(E.ai);
  K.af_off = B.addv(E.af);
  K.ad_off = B.addv(E.ad);
}

// The planning of a batch, in two halves around the point where run_batch
// needs its slot's workspace; production (run_batch) and the host-only hook
// (fi_debug_host_plan) both run exactly these.  T takes now_ms() at the end of
// each stage.
// First half: every image's geometry, descriptor, resample path and tables,
// then the smartcrop stage; E.work.size is the workspace the batch needs.
void fi::plan_batch(fi_ctx *c, Exec &E, BatchPlan &Bp, fi_image *imgs, int n, PlanTimes &T) {
  Bp.imgs = imgs;
  Bp.n = n;
  Bp.plans.resize(n);
  Bp.status.assign(n, FI_OK);
  Bp.errs.resize(n);
  Bp.rd_of.assign(n, -1);
  Bp.sc_of.assign(n, -1);
  Bp.res_off.assign(n, 0);
  Bp.res_stride.assign(n, 0);
  Bp.out_of.assign(n, nullptr);
  for (int i = 0; i < n; i++) plan_image(c, E, Bp, i);
  T.images = now_ms();
  plan_batch_sc(c, E, Bp);
  T.sc = now_ms();
}
// Second half, against the workspace base wb: device pointers, the tiles of
// the streaming kernels, and the upload blob E.blob with its offsets in K.
void fi::place_batch(fi_ctx *c, Exec &E, BatchPlan &Bp, Packed &K, uint8_t *wb, PlanTimes &T) {
  resolve_workspace(E, Bp, wb);
  T.workspace = now_ms();
  build_vm_tiles(c, E, Bp);
  T.vm = now_ms();
  build_hv_tiles(c, E, Bp);
  T.hv = now_ms();
  pack_batch(c, E, Bp, K);
  T.blob = now_ms();
}
