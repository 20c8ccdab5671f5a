// fi_batch.cpp -- the batch pipeline of the runtime (fi_runtime.h).  run_batch
// plans a batch (fi_rs_plan.cpp plan_batch, place_batch), uploads its blob into
// the next of kSlots slots, enqueues the stages (launch_batch) and the result
// readback (queue_readback); finalize_front fills the caller's records.  The
// host-buffer entry points stage sources and outputs around it, and
// fi_debug_host_plan runs the same planner with no device.
#include "fi_runtime.h"

using namespace fi;

// Enqueue the batch: resample, shear rotations, convolutions, -monochrome and
// the smartcrop stage on the main stream (sc_stream is the same stream); the crop apply on
// ap_stream behind this batch's smartcrop stage, so it runs beside the next
// batch's resample (FI_APPLY_OVERLAP=0: on the main stream).  ap_tail marks
// the last apply for the entry points that must not run before it
// (order_after_apply).
static int launch_batch(fi_ctx *c, const Exec &E, const BatchPlan &Bp, const Packed &K, uint8_t *ab, uint8_t *wb,
                        Slot &S) {
  S.tail = c->sc_stream;
  S.ap_lo = S.ap_hi = 0;
  const int32_t *ai = (const int32_t *)c->heap_i.p;
  const float *af = (const float *)c->heap_f.p;
  const double *ad = (const double *)c->heap_d.p;
  const ScParamsDev PD = to_dev(E.params);
  auto desc_p = [&](const Launch &L) { return ab + L.desc_off; };
  auto pre_p = [&](const Launch &L) { return (const int32_t *)(ab + L.prefix_off); };
  Timer tb(c, "batch", 0, c->stream, c->sc_stream);
  {
    Timer t(c, "resize", Bp.resize_bytes);
    if (K.L0.tiles)
      hipLaunchKernelGGL(k_rs_copy, dim3(K.L0.tiles), dim3(256), 0, c->stream, (const ResizeDesc *)desc_p(K.L0),
                         pre_p(K.L0), K.L0.n);
    const bool fork = c->vr_fork && c->rs2_stream && Bp.vrl.size() >= 2;
    if (fork) {
      if (!c->rs_fork) HIP_TRY(hipEventCreateWithFlags(&c->rs_fork, hipEventDisableTiming));
      if (!c->rs_join) HIP_TRY(hipEventCreateWithFlags(&c->rs_join, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(c->rs_fork, c->stream));
      HIP_TRY(hipStreamWaitEvent(c->rs2_stream, c->rs_fork, 0));
      c->stats["vr_fork"].launches += 1;
    }
    // the join, at the end of the resize scope (before its timer's end event)
    // and on every early error return, so no forked launch outlives the stage
    struct Join {
      fi_ctx *c;
      bool on;
      ~Join() {
        if (!on) return;
        if (hipEventRecord(c->rs_join, c->rs2_stream) != hipSuccess ||
            hipStreamWaitEvent(c->stream, c->rs_join, 0) != hipSuccess)
          (void)hipStreamSynchronize(c->rs2_stream);
      }
    } join{c, fork};
    for (const BatchPlan::VrLaunch &V : Bp.vrl) {
      hipStream_t vs = fork && &V != &Bp.vrl[0] ? c->rs2_stream : c->stream;
      const int vrc = launch_vr(vs, (const VDesc *)(ab + K.vdesc_off), (const MStrip *)(ab + K.vstrip_off),
                                (const VrTile *)(ab + K.vrtile_off) + V.tile0, V.ntiles,
                                (const int32_t *)(ab + K.vrinfo_off) + V.info0, V.G, ai, V.L);
      if (vrc < 0) return set_err(FI_EDEVICE, "block-major MFMA resample launch rejected (LDS %d)", V.L.total);
      if (vrc == 1) c->stats["vr_ablation"].launches += 1;  // FI_VR_VARIANT ablation: wrong pixels
      c->stats["path_vr"].launches += V.images;
      c->stats["path_vm"].launches -= V.images;
    }
    if (!Bp.vtiles.empty() &&
               launch_vm(c->stream, (const VDesc *)(ab + K.vdesc_off), (const MStrip *)(ab + K.vstrip_off),
                         (const VTile *)(ab + K.vtile_off), (int)Bp.vtiles.size(), ai, Bp.vm_lds) != 0)
      return set_err(FI_EDEVICE, "streaming MFMA resample launch rejected (LDS %zu)", Bp.vm_lds);
    // (k_rs_hv on a stream of its own beside k_rs_vm was measured: cfg4 102.1
    // vs 102.5 ms/step -- k_rs_vm's LDS leaves no CU room to overlap into)
    if (!Bp.htiles.empty() &&
        launch_hv(c->stream, (const HvDesc *)(ab + K.hdesc_off), (const HvStripD *)(ab + K.hstrip_off),
                  (const HvTile *)(ab + K.htile_off), (int)Bp.htiles.size(), ai, Bp.hv_lds) != 0)
      return set_err(FI_EDEVICE, "horizontal-first MFMA resample launch rejected (LDS %zu)", Bp.hv_lds);
    if (K.Q0.tiles || K.Q1a.tiles || K.Q2a.tiles) {
      const ResizeDesc *dq0 = (const ResizeDesc *)desc_p(K.Q0), *dq1 = (const ResizeDesc *)desc_p(K.Q1a),
                       *dq2a = (const ResizeDesc *)desc_p(K.Q2a), *dq2b = (const ResizeDesc *)desc_p(K.Q2b);
      launch_rs4(c->stream, 0, dq0, pre_p(K.Q0), K.Q0.n, K.Q0.tiles, nullptr, nullptr, 0, 0, ai, ad);
      launch_rs4(c->stream, 1, dq1, pre_p(K.Q1a), K.Q1a.n, K.Q1a.tiles, dq1, pre_p(K.Q1a), K.Q1a.n, K.Q1a.tiles, ai,
                 ad);
      launch_rs4(c->stream, 2, dq2a, pre_p(K.Q2a), K.Q2a.n, K.Q2a.tiles, dq2b, pre_p(K.Q2b), K.Q2b.n, K.Q2b.tiles,
                 ai, ad);
    }
    if (K.L1a.tiles) {
      hipLaunchKernelGGL(k_rs_v_u8, dim3(K.L1a.tiles), dim3(256), 0, c->stream, (const ResizeDesc *)desc_p(K.L1a),
                         pre_p(K.L1a), K.L1a.n, ai, af);
      hipLaunchKernelGGL(k_rs_h_final, dim3(K.L1a.tiles), dim3(256), 0, c->stream,
                         (const ResizeDesc *)desc_p(K.L1a), pre_p(K.L1a), K.L1a.n, ai, af);
    }
    if (K.L2a.tiles) {
      if (K.h_tiled)
        launch_rs_h_tile(c->stream, (const ResizeDesc *)desc_p(K.L2a), pre_p(K.L2a), K.L2a.n, K.L2a.tiles, ai, af,
                         Bp.h_tile_pitch, Bp.h_tile_taps);
      else
        hipLaunchKernelGGL(k_rs_h_u8, dim3(K.L2a.tiles), dim3(256), 0, c->stream, (const ResizeDesc *)desc_p(K.L2a),
                           pre_p(K.L2a), K.L2a.n, ai, af);
      hipLaunchKernelGGL(k_rs_v_final, dim3(K.L2b.tiles), dim3(256), 0, c->stream,
                         (const ResizeDesc *)desc_p(K.L2b), pre_p(K.L2b), K.L2b.n, ai, af);
    }
  }
  if (K.RL.tiles) {
    // shear rotations, between the epilogue's integral rotation and the convolutions
    Timer t(c, "rotate", Bp.rot_bytes);
    launch_rot(c->stream, (const RotDesc *)desc_p(K.RL), pre_p(K.RL), K.RL.n, K.RL.tiles);
  }
  if (!Bp.conv_items.empty()) {
    Timer t(c, "conv", 0);
    static const int kMode[6] = {0, 2, 3, 0, 1, 4};
    for (int k = 0; k < 6; k++)
      launch_conv(c->stream, kMode[k], (const ConvStep *)desc_p(K.CL[k]), pre_p(K.CL[k]), K.CL[k].n, K.CL[k].tiles,
                  ad);
  }
  if (!Bp.mono.empty()) {
    Timer t(c, "mono", 0);
    (void)launch_mono(c->stream, (const MonoDesc *)(ab + K.mono_off), (int)Bp.mono.size(), ad + K.mono_wts);
  }
  HIP_TRY(hipGetLastError());
  // a smartcrop stage made only of co-resident kernels (k_sc_hx / k_sc_vx, the
  // score, the apply) runs on ap_stream behind this batch's resample, beside
  // the next batch's
  const bool beside = c->sc_cx == 3 && c->apply_overlap && c->ap_stream && K.SX.ncx > 0 && K.SX.ncx == K.SX.nok;
  hipStream_t scs = c->sc_stream;
  if (c->sc_stream != c->stream || beside) {
    if (beside) scs = c->ap_stream;
    if (!S.rs_done) HIP_TRY(hipEventCreateWithFlags(&S.rs_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(S.rs_done, c->stream));
    HIP_TRY(hipStreamWaitEvent(scs, S.rs_done, 0));
  }
  if (K.SX.nsl + K.SX.nsg + K.SX.ns3 > 0) {
    const int rc = enqueue_sc(c, scs, ab, K.SX, ai, ad, (CropScore *)(wb + Bp.scores_off),
                              (ScResult *)(wb + Bp.results_off), PD);
    if (rc) return rc;
    if (beside) {
      S.tail = scs;
      tb.sb = scs;
    }
    if (!Bp.apply.empty()) {
      hipStream_t as = scs;
      int pw = 0;
      if (beside) {
        pw = c->n_cu;
      } else if (c->apply_overlap && c->ap_stream) {
        if (!S.sc_done) HIP_TRY(hipEventCreateWithFlags(&S.sc_done, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(S.sc_done, c->sc_stream));
        HIP_TRY(hipStreamWaitEvent(c->ap_stream, S.sc_done, 0));
        as = c->ap_stream;
        pw = c->n_cu;
        S.tail = as;
        tb.sb = as;  // the batch range ends with its apply
      }
      {
        Timer t(c, "crop_apply", 0, as, as);
        (void)launch_crop_apply(as, (const ApplyDesc *)(ab + K.apply_off), (int)Bp.apply.size(),
                                (const DevCrop *)(ab + K.SX.crops_off), (const ScResult *)(wb + Bp.results_off), pw);
      }
      if (as == c->ap_stream) {
        if (!c->ap_tail) HIP_TRY(hipEventCreateWithFlags(&c->ap_tail, hipEventDisableTiming));
        // (as in the overlapped apply; the smartcrop kernels beside it write only the slot's workspace)
        HIP_TRY(hipEventRecord(c->ap_tail, as));
        c->ap_pending = true;
        // the bytes this apply writes (a crop is at most the resized image)
        S.ap_lo = UINTPTR_MAX;
        S.ap_hi = 0;
        for (const ApplyDesc &a : Bp.apply) {
          S.ap_lo = std::min(S.ap_lo, (uintptr_t)a.dst);
          S.ap_hi = std::max(S.ap_hi, (uintptr_t)a.dst + (uintptr_t)a.W * a.H * a.C);
        }
      }
    } else if (beside) {
      if (!c->ap_tail) HIP_TRY(hipEventCreateWithFlags(&c->ap_tail, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(c->ap_tail, scs));
      c->ap_pending = true;
    }
    HIP_TRY(hipGetLastError());
  }
  return FI_OK;
}

// Per-image result records into the slot's pinned readback; the batch joins
// the in-flight list (finalize_front fills the caller's records).
static int queue_readback(fi_ctx *c, BatchPlan &Bp, int slot, uint8_t *wb, double t_start,
                          std::shared_ptr<HostIo> host) {
  Slot &S = c->slots[slot];
  // device outputs: the few result bytes go back on the batch's own stream
  // (a cross-stream event costs the next batch's first kernel ~20-30 us of
  // idle GPU, measured in round 5's kernel trace); host outputs (image bytes)
  // on the readback stream, so the next batch's kernels overlap their copies
  hipStream_t tail = S.tail ? S.tail : c->sc_stream;
  hipStream_t rs = host ? c->rb_stream : tail;
  if (rs != tail) {
    if (!S.sc_end) HIP_TRY(hipEventCreateWithFlags(&S.sc_end, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(S.sc_end, tail));
    HIP_TRY(hipStreamWaitEvent(rs, S.sc_end, 0));
  }
  if (host) {
    // outputs to the host, behind the batch's last kernel on sc_stream: the
    // planned (pre-apply) bytes cover the applied crop, which is never larger
    double obytes = 0;
    for (int i = 0; i < Bp.n; i++)
      if (Bp.status[i] == FI_OK && host->user[i].dst) obytes += (double)Bp.imgs[i].out_stride * Bp.imgs[i].out_h;
    Timer t(c, "d2h_out", obytes, rs, rs);
    for (int i = 0; i < Bp.n; i++) {
      const fi_image &d = Bp.imgs[i];
      if (Bp.status[i] != FI_OK || !host->user[i].dst) continue;
      const size_t bytes = (size_t)d.out_stride * d.out_h;
      uint8_t *to = host->pin_off[i] < 0 ? host->user[i].dst : (uint8_t *)S.hpin + host->pin_off[i];
      HIP_TRY(hipMemcpyAsync(to, (uint8_t *)S.hio.p + host->dev_dst_off[i], bytes, hipMemcpyDeviceToHost,
                             rs));
    }
  }
  uint8_t *rp = (uint8_t *)S.res;
  const size_t res_bytes = sizeof(ScResult) * Bp.sitems.size();
  const size_t outwh_bytes = sizeof(int32_t) * 2 * (size_t)Bp.n;
  if (!Bp.sitems.empty())
    HIP_TRY(hipMemcpyAsync(rp, wb + Bp.results_off, res_bytes, hipMemcpyDeviceToHost, rs));
  if (!Bp.apply.empty())
    HIP_TRY(hipMemcpyAsync(rp + res_bytes, wb + Bp.outwh_off, outwh_bytes, hipMemcpyDeviceToHost, rs));
  if (!S.done) HIP_TRY(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(S.done, rs));
  S.busy = true;
  c->next_slot = (slot + 1) % kSlots;
  PendingBatch pb;
  pb.imgs = Bp.imgs;
  pb.n = Bp.n;
  pb.slot = slot;
  pb.t_start = t_start;
  pb.status = std::move(Bp.status);
  pb.errs = std::move(Bp.errs);
  pb.sc_of = std::move(Bp.sc_of);
  pb.sstatus = std::move(Bp.sstatus);
  pb.serrs = std::move(Bp.serrs);
  pb.crop0.resize(Bp.SL.descs.size());
  for (size_t k = 0; k < Bp.SL.descs.size(); k++) pb.crop0[k] = Bp.SL.descs[k].crop0;
  pb.crops = std::move(Bp.SL.crops);
  pb.nres = Bp.sitems.size();
  pb.any_apply = !Bp.apply.empty();
  pb.timers.swap(c->pending);  // waited for when this batch is finalized
  pb.host = std::move(host);
  c->inflight.push_back(std::move(pb));
  return FI_OK;
}

static int wait_slot(fi_ctx *c, int slot);
static int run_batch(fi_ctx *c, fi_image *imgs, int32_t n, bool async, std::shared_ptr<HostIo> host = nullptr) {
  const double t_start = now_ms();
  Exec E;
  E.c = c;
  fi_smartcrop_default_params(&E.params);
  int rc = heap_prepare(c, E);
  if (rc) return rc;
  BatchPlan Bp;
  PlanTimes T;
  plan_batch(c, E, Bp, imgs, n, T);
  // the batch's slot: pinned staging + device blob/workspace (the batch that
  // used it last must be done before anything here is overwritten)
  const int slot = c->next_slot;
  rc = wait_slot(c, slot);
  if (rc) return rc;
  Slot &S = c->slots[slot];
  rc = ensure(c, &S.work, E.work.size + 256);
  if (rc) return rc;
  uint8_t *wb = (uint8_t *)S.work.p;
  Packed K;
  place_batch(c, E, Bp, K, wb, T);
  host_stat(c, "host_plan_hv", T.hv - T.vm);
  if (!heap_fits(c, E)) {
    // the batch's new tables overflow the heaps: start them empty and plan again
    if (c->heap_retry) return set_err(FI_ENOMEM, "batch tables exceed the device table heap");
    heap_reset(c);
    c->heap_retry = true;
    const int rrc = run_batch(c, imgs, n, async, host);
    c->heap_retry = false;
    return rrc;
  }
  // ---- upload (pinned slot: the previous batch may still be running)
  const Blob &B = E.blob;
  rc = ensure(c, &S.arena, B.b.size() + 256);
  if (rc) return rc;
  rc = ensure_pinned_buf(&S.blob, &S.blob_cap, B.b.size() + 256);
  if (rc) return rc;
  rc = ensure_pinned_buf(&S.res, &S.res_cap, sizeof(ScResult) * Bp.sitems.size() + sizeof(int32_t) * 2 * (size_t)n + 64);
  if (rc) return rc;
  memcpy(S.blob, B.b.data(), B.b.size());
  HIP_TRY(hipMemcpyAsync(S.arena.p, S.blob, B.b.size(), hipMemcpyHostToDevice, c->up_stream));
  if (!S.up_done) HIP_TRY(hipEventCreateWithFlags(&S.up_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(S.up_done, c->up_stream));
  // device-resident batches: the upload stream carries only this small blob,
  // and the host runs batches ahead of the GPU, so it waits for the copy
  // itself rather than putting a wait packet between the previous batch's
  // score and this batch's resample (measured: that gap 18 -> 11 us per cfg2
  // step); host-buffer batches upload their sources on that stream too
  if (c->up_hostsync && !host)
    HIP_TRY(hipEventSynchronize(S.up_done));
  else
    HIP_TRY(hipStreamWaitEvent(c->stream, S.up_done, 0));
  const double t_planned = now_ms();
  host_stat(c, "host_plan", t_planned - t_start);
  host_stat(c, "host_plan_images", T.images - t_start);
  host_stat(c, "host_plan_sc", T.workspace - T.images);  // with the wait for the slot
  host_stat(c, "host_plan_tiles", T.hv - T.workspace);
  host_stat(c, "host_plan_vmtiles", T.hv - T.workspace);
  host_stat(c, "host_plan_blob", t_planned - T.hv);
  if (c->timing) c->stats["host_plan"].bytes += (double)B.b.size();
  uint8_t *ab = (uint8_t *)S.arena.p;
  // a source that an earlier batch's overlapped crop apply is still writing
  // (a chained request: this batch resizes that batch's output): the resample
  // waits for the applies (bounding ranges: a false hit only costs the overlap)
  for (const Slot &o : c->slots) {
    if (&o == &S || o.ap_hi <= o.ap_lo) continue;
    bool hit = false;
    for (int i = 0; i < n && !hit; i++) {
      const fi_image &im = imgs[i];
      if (!im.src || im.src_h <= 0 || im.src_stride <= 0) continue;
      const uintptr_t s0 = (uintptr_t)im.src, s1 = s0 + (uintptr_t)im.src_stride * (uintptr_t)im.src_h;
      hit = s0 < o.ap_hi && o.ap_lo < s1;
    }
    if (hit && order_after_apply(c) != FI_OK) return set_err(FI_EDEVICE, "hipStreamWaitEvent failed");
  }
  rc = heap_commit(c, E, ab, K.ai_off, K.af_off, K.ad_off);
  if (rc) return rc;
  rc = launch_batch(c, E, Bp, K, ab, wb, S);
  if (rc) return rc;
  rc = queue_readback(c, Bp, slot, wb, t_start, host);
  if (rc) return rc;
  host_stat(c, "host_launch", now_ms() - t_planned);
  if (async) return FI_OK;
  return drain(c);
}

// Wait for the oldest in-flight batch and fill its fi_image records.
static int finalize_front(fi_ctx *c) {
  PendingBatch pb = std::move(c->inflight.front());
  c->inflight.erase(c->inflight.begin());
  Slot &S = c->slots[pb.slot];
  const double t_wait = now_ms();
  HIP_TRY(hipEventSynchronize(S.done));
  S.busy = false;
  S.ap_lo = S.ap_hi = 0;  // its apply is done (S.done follows it on the tail stream)
  if (c->inflight.empty()) c->ap_pending = false;
  collect_ranges(c, pb.timers);
  const double t_done = now_ms();
  host_stat(c, "host_wait", t_done - t_wait);
  const ScResult *res = (const ScResult *)S.res;
  const int32_t *outwh = (const int32_t *)((const uint8_t *)S.res + sizeof(ScResult) * pb.nres);
  int first_bad = FI_OK;
  std::string first_err;
  for (int i = 0; i < pb.n; i++) {
    fi_image &im = pb.imgs[i];
    im.n_candidates = 0;
    if (pb.status[i] == FI_OK && pb.sc_of[i] >= 0) {
      const int k = pb.sc_of[i];
      if (pb.sstatus[k] != FI_OK) {
        pb.status[i] = pb.sstatus[k];
        pb.errs[i] = pb.serrs[k];
      } else {
        const ScResult &r = res[k];
        if (r.top < 0) {
          pb.status[i] = FI_EUNSUPPORTED;
          pb.errs[i] = "smartcrop: too many crop windows for the scoring kernel";
        } else {
          const DevCrop &dc = pb.crops[pb.crop0[k] + r.top];
          im.crop_x = dc.rx;
          im.crop_y = dc.ry;
          im.crop_w = dc.rw;
          im.crop_h = dc.rh;
          im.crop_score = r.total;
          im.n_candidates = r.n_candidates;
          if ((im.flags & FI_OP_SMARTCROP_APPLY) && pb.any_apply) {
            im.out_w = outwh[2 * i];
            im.out_h = outwh[2 * i + 1];
            im.out_stride = im.out_w * im.out_channels;
          }
        }
      }
    }
    im.status = pb.status[i];
    if (pb.status[i] != FI_OK && first_bad == FI_OK) {
      first_bad = pb.status[i];
      first_err = "image " + std::to_string(i) + ": " + pb.errs[i];
    }
    if (pb.host) {  // host-buffer batch: the caller's record, and its staged output
      fi_image &o = pb.host->user[i];
      o.out_w = im.out_w;
      o.out_h = im.out_h;
      o.out_channels = im.out_channels;
      o.out_stride = im.out_stride;
      o.crop_x = im.crop_x;
      o.crop_y = im.crop_y;
      o.crop_w = im.crop_w;
      o.crop_h = im.crop_h;
      o.crop_score = im.crop_score;
      o.status = im.status;
      o.n_candidates = im.n_candidates;
      if (im.status == FI_OK && o.dst && pb.host->pin_off[i] >= 0)
        memcpy(o.dst, (const uint8_t *)S.hpin + pb.host->pin_off[i], (size_t)im.out_stride * im.out_h);
    }
  }
  host_stat(c, "host_total", now_ms() - pb.t_start);
  if (first_bad != FI_OK) return set_err(first_bad, "%s", first_err.c_str());
  return FI_OK;
}
// Finalize every in-flight batch (in order); returns the first error.
int fi::drain(fi_ctx *c) {
  int first = FI_OK;
  while (!c->inflight.empty()) {
    const int rc = finalize_front(c);
    if (rc != FI_OK && first == FI_OK) first = rc;
  }
  if (first != FI_OK) return first;  // message of the first failure is in g_err... of the last
  return FI_OK;
}
static int wait_slot(fi_ctx *c, int slot) {
  int first = FI_OK;
  while (c->slots[slot].busy && !c->inflight.empty()) {
    const int rc = finalize_front(c);
    if (rc != FI_OK && first == FI_OK) first = rc;
  }
  return first;
}

extern "C" {

// Test hook (host only, needs no GPU): run_batch's planner -- plan_batch and
// place_batch, the functions run_batch calls -- over `imgs` `iters` times on one host-only
// context (device pointers are planned, never dereferenced; caches and heap
// offsets persist across iterations as across a serving run's batches).
// ms[0..6] += images, smartcrop, workspace, vm + vr tiles, of which vr, hv
// tiles, blob (milliseconds, summed over the iterations).
int fi_debug_host_plan(const fi_image *imgs, int32_t n, int32_t iters, double *ms) {
  static fi_ctx *c = nullptr;  // one host-only context across calls (its caches, as a serving context's)
  // the last planned batch, for (NULL, 3, ...): its blob, workspace size and counts
  static std::vector<uint8_t> last_blob;
  static size_t last_work = 0;
  static double last[7] = {0, 0, 0, 0, 0, 0, 0};
  if (!imgs && n == 0) {       // (NULL, 0, ...): drop it
    if (c && getenv("FI_PLAN_PROF"))
      for (const auto &kv : c->stats) fprintf(stderr, "%s %.1f ms (%lld)\n", kv.first.c_str(), kv.second.ms, (long long)kv.second.launches);
    delete c;
    c = nullptr;
    std::vector<uint8_t>().swap(last_blob);
    return FI_OK;
  }
  if (!imgs && n == 1) {  // (NULL, 1, ...): reset the stage stats (after a warm-up pass)
    if (c) c->stats.clear();
    return FI_OK;
  }
  if (!imgs && n == 2) {  // (NULL, 2, 0, ms): the resample plan's counters
    if (!ms) return set_err(FI_EINVAL, "ms is NULL");
    ms[0] = ms[1] = ms[2] = 0;
    if (c) {
      ms[0] = (double)c->stats["plan_path_vr"].launches;
      ms[1] = (double)c->stats["plan_vertical_first"].launches;
      ms[2] = (double)c->stats["plan_vr_launches"].launches;
    }
    return FI_OK;
  }
  if (!imgs && n == 3) {  // (NULL, 3, 0, ms): what the last planned batch emitted
    if (!ms) return set_err(FI_EINVAL, "ms is NULL");
    // FNV-1a over the upload blob, then the workspace size: every descriptor
    // field, tile, launch list and heap offset the planner emitted
    uint64_t h = 1469598103934665603ull;
    for (uint8_t x : last_blob) h = (h ^ x) * 1099511628211ull;
    for (int k = 0; k < 8; k++) h = (h ^ (((uint64_t)last_work >> (8 * k)) & 255)) * 1099511628211ull;
    last[0] = (double)(uint32_t)h;
    last[1] = (double)(uint32_t)(h >> 32);
    for (int k = 0; k < 7; k++) ms[k] = last[k];
    return FI_OK;
  }
  if (!imgs || n <= 0 || iters <= 0 || !ms) return set_err(FI_EINVAL, "bad arguments");
  if (!c) {
    c = new fi_ctx();
    c->host_only = true;
    c->timing = true;
    if (const char *e = getenv("FI_VR_RS")) c->vr_rs = e[0] == '1';
  }
  std::vector<fi_image> v(imgs, imgs + n);
  uint8_t *wb = reinterpret_cast<uint8_t *>((uintptr_t)1 << 40);  // a stand-in workspace base
  int rc = FI_OK;
  for (int it = 0; it < iters && rc == FI_OK; it++) {
    const double t0 = now_ms();
    Exec E;
    E.c = c;
    fi_smartcrop_default_params(&E.params);
    rc = heap_prepare(c, E);
    if (rc) break;
    BatchPlan Bp;
    PlanTimes T;
    Packed K;
    const double vr0 = c->stats["host_plan_vr"].ms;
    plan_batch(c, E, Bp, v.data(), n, T);
    place_batch(c, E, Bp, K, wb, T);
    // images per resample kernel (FI_PLAN_PROF lists them; (NULL, 2, ...) reads them)
    int nvr = 0;
    for (const BatchPlan::VrLaunch &V : Bp.vrl) nvr += V.images;
    c->stats["plan_path_vr"].launches += nvr;
    // (build_vr_tiles appends a second descriptor for each of its images)
    c->stats["plan_vertical_first"].launches += (int64_t)Bp.vdescs.size() - nvr;
    c->stats["plan_vr_launches"].launches += (int64_t)Bp.vrl.size();
    // kept for (NULL, 3, ...): the blob is hashed only when a caller asks
    last_blob.swap(E.blob.b);
    last[2] = (double)last_blob.size();
    last[3] = (double)Bp.vtiles.size();
    last[4] = (double)Bp.vrtiles.size();
    last[5] = (double)Bp.htiles.size();
    last[6] = (double)Bp.sitems.size();
    last_work = E.work.size;
    if (!heap_fits(c, E)) heap_reset(c);
    else {
      c->heap_i.used = (size_t)E.bi + (E.ai.size() + 15) / 16 * 16;
      c->heap_f.used = (size_t)E.bf + (E.af.size() + 15) / 16 * 16;
      c->heap_d.used = (size_t)E.bd + (E.ad.size() + 15) / 16 * 16;
    }
    ms[0] += T.images - t0;
    ms[1] += T.sc - T.images;
    ms[2] += T.workspace - T.sc;
    ms[3] += T.vm - T.workspace;
    ms[4] += c->stats["host_plan_vr"].ms - vr0;
    ms[5] += T.hv - T.vm;
    ms[6] += T.blob - T.hv;
  }
  return rc;
}

int fi_process_batch_device(fi_ctx *c, fi_image *imgs, int32_t n) {
  if (!c || n < 0 || (n > 0 && !imgs)) return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return run_batch(c, imgs, n, false);
}

int fi_submit_batch_device(fi_ctx *c, fi_image *imgs, int32_t n) {
  if (!c || n < 0 || (n > 0 && !imgs)) return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return run_batch(c, imgs, n, true);
}

int fi_wait(fi_ctx *c, int32_t keep) {
  if (!c || keep < 0) return set_err(FI_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  int first = FI_OK;
  while ((int32_t)c->inflight.size() > keep) {
    const int rc = finalize_front(c);
    if (rc != FI_OK && first == FI_OK) first = rc;
  }
  return first;
}

// Host-buffer batch, asynchronous: sources into the batch slot's device
// buffer (pinned sources DMA directly; pageable ones through the slot's pinned
// staging), run_batch, outputs back behind the batch (queue_readback).  The
// slot's previous batch is finalized first, so two host batches are in flight.
static bool host_pinned(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // clear the sticky "invalid value" of a pageable pointer
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
static int submit_host(fi_ctx *c, fi_image *imgs, int32_t n) {
  const int slot = c->next_slot;
  {
    const int rc0 = wait_slot(c, slot);  // per-image failures of that batch stay in its records
    if (rc0 == FI_EDEVICE) return rc0;
  }
  Slot &S = c->slots[slot];
  auto host = std::make_shared<HostIo>();
  host->user = imgs;
  host->dev.assign(imgs, imgs + n);
  host->dev_dst_off.assign(n, 0);
  host->pin_off.assign(n, -1);
  std::vector<size_t> soff(n, 0);
  std::vector<int64_t> spin(n, -1);  // pageable source: offset of its packed rows in the staging
  std::vector<uint8_t> src_pinned(n, 0);
  size_t total = 0, pin_total = 0;
  for (int i = 0; i < n; i++) {
    const fi_image &im = imgs[i];
    const int C = im.src_channels == 4 ? 4 : 3;
    const int64_t sstride = ((int64_t)im.src_w * C + 15) / 16 * 16;
    soff[i] = total;
    total += (size_t)std::max<int64_t>(sstride * im.src_h, 0);
    total = (total + 255) / 256 * 256;
    host->dev_dst_off[i] = total;
    total += (size_t)std::max<int64_t>(im.dst_capacity, 0);
    total = (total + 255) / 256 * 256;
    host->dev[i].src_stride = (int32_t)sstride;
    const bool ok = im.src && im.src_w > 0 && im.src_h > 0 && (im.src_channels == 3 || im.src_channels == 4) &&
                    im.src_stride >= im.src_w * im.src_channels;
    if (ok && !(src_pinned[i] = host_pinned(im.src))) {
      spin[i] = (int64_t)pin_total;
      pin_total += ((size_t)im.src_w * im.src_channels * im.src_h + 255) / 256 * 256;
    }
    if (im.dst && im.dst_capacity > 0 && !host_pinned(im.dst)) {
      host->pin_off[i] = (int64_t)pin_total;
      pin_total += ((size_t)im.dst_capacity + 255) / 256 * 256;
    }
  }
  int rc = ensure(c, &S.hio, total + 256);
  if (rc) return rc;
  rc = ensure_pinned_buf(&S.hpin, &S.hpin_cap, pin_total + 256);
  if (rc) return rc;
  uint8_t *io = (uint8_t *)S.hio.p;
  double sbytes = 0;
  for (int i = 0; i < n; i++)
    if (imgs[i].src && imgs[i].src_w > 0 && imgs[i].src_h > 0)
      sbytes += (double)imgs[i].src_w * imgs[i].src_channels * imgs[i].src_h;
  {
  const double t_pack = now_ms();
  Timer t(c, "h2d_src", sbytes, c->up_stream, c->up_stream);
  for (int i = 0; i < n; i++) {
    const fi_image &im = imgs[i];
    fi_image &d = host->dev[i];
    const int C = im.src_channels;
    const bool ok = im.src && im.src_w > 0 && im.src_h > 0 && (C == 3 || C == 4) && im.src_stride >= im.src_w * C;
    d.dst = im.dst ? io + host->dev_dst_off[i] : nullptr;
    if (!ok) {
      d.src = nullptr;
      continue;
    }
    const size_t row = (size_t)im.src_w * C;
    const uint8_t *from = im.src;
    int64_t from_stride = im.src_stride;
    if (!src_pinned[i]) {  // pageable: pack the rows into the pinned staging first
      uint8_t *pin = (uint8_t *)S.hpin + spin[i];
      for (int y = 0; y < im.src_h; y++) memcpy(pin + (size_t)y * row, im.src + (int64_t)y * im.src_stride, row);
      from = pin;
      from_stride = (int64_t)row;
    }
    HIP_TRY(hipMemcpy2DAsync(io + soff[i], d.src_stride, from, from_stride, row, im.src_h, hipMemcpyHostToDevice,
                             c->up_stream));
    d.src = io + soff[i];
  }
  host_stat(c, "host_src_stage", now_ms() - t_pack);  // pageable rows packed into pinned staging + copy issue
  }
  return run_batch(c, host->dev.data(), n, true, host);
}

int fi_submit_batch(fi_ctx *c, fi_image *imgs, int32_t n) {
  if (!c || n < 0 || (n > 0 && !imgs)) return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return submit_host(c, imgs, n);
}

int fi_process_batch(fi_ctx *c, fi_image *imgs, int32_t n) {
  if (!c || n < 0 || (n > 0 && !imgs)) return set_err(FI_EINVAL, "bad arguments");
  if (n == 0) return FI_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  {
    const int rc0 = drain(c);  // synchronous call: earlier batches complete first
    if (rc0 == FI_EDEVICE) return rc0;
  }
  const int rc = submit_host(c, imgs, n);
  const int rd = drain(c);
  return rc != FI_OK ? rc : rd;
}

int fi_query(fi_ctx *c, int32_t *running) {
  if (!c || !running) return set_err(FI_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  int n = 0;
  for (const PendingBatch &pb : c->inflight) {
    const hipError_t e = hipEventQuery(c->slots[pb.slot].done);
    if (e == hipErrorNotReady) {
      n++;
    } else if (e != hipSuccess) {
      return set_err(FI_EDEVICE, "hipEventQuery: %s", hipGetErrorString(e));
    }
  }
  *running = n;
  return FI_OK;
}

}  // extern "C"
