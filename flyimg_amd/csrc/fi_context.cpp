// fi_context.cpp -- the context of the C-ABI runtime (fi_runtime.h): errors,
// fi_create / fi_destroy, device and pinned buffers, the event pool and HIP-event
// timers, statistics, the device-resident table heaps, and the plain device /
// host memory entry points.
#include "fi_runtime.h"

using namespace fi;

static thread_local std::string g_err;
int fi::set_err(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
void fi::sync_streams(fi_ctx *c) {
  if (c->host_only) return;
  (void)hipStreamSynchronize(c->stream);
  if (c->sc_stream != c->stream) (void)hipStreamSynchronize(c->sc_stream);
  if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
  if (c->rb_stream) (void)hipStreamSynchronize(c->rb_stream);
  if (c->ap_stream) (void)hipStreamSynchronize(c->ap_stream);
  if (c->rs2_stream) (void)hipStreamSynchronize(c->rs2_stream);
  if (c->gx_stream) (void)hipStreamSynchronize(c->gx_stream);
}
// Work about to run on c->stream that may read or write an earlier batch's
// dst waits for the crop applies still running beside it on ap_stream.
int fi::order_after_apply(fi_ctx *c) {
  if (!c->ap_pending) return FI_OK;
  if (hipStreamWaitEvent(c->stream, c->ap_tail, 0) != hipSuccess) return FI_EDEVICE;
  c->ap_pending = false;
  for (Slot &s : c->slots) s.ap_lo = s.ap_hi = 0;
  return FI_OK;
}
int fi::ensure(fi_ctx *c, DevBuf *b, size_t bytes) {
  if (b->cap >= bytes) return FI_OK;
  sync_streams(c);  // in-flight batches may still read it
  if (b->p) (void)hipFree(b->p);
  b->p = nullptr;
  b->cap = 0;
  size_t cap = std::max(bytes + bytes / 4, (size_t)1 << 20);
  if (hipMalloc(&b->p, cap) != hipSuccess) {
    b->p = nullptr;
    return set_err(FI_ENOMEM, "hipMalloc(%zu) failed on device %d", cap, c->device);
  }
  b->cap = cap;
  return FI_OK;
}
int fi::ensure_pinned_buf(void **p, size_t *cap_io, size_t bytes) {
  if (*cap_io >= bytes) return FI_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap_io = 0;
  size_t cap = std::max(bytes + bytes / 4, (size_t)1 << 16);
  if (hipHostMalloc(p, cap, hipHostMallocDefault) != hipSuccess) {
    *p = nullptr;
    return set_err(FI_ENOMEM, "hipHostMalloc(%zu) failed", cap);
  }
  *cap_io = cap;
  return FI_OK;
}
int fi::ensure_pinned(fi_ctx *c, size_t bytes) {
  if (c->pinned_cap >= bytes) return FI_OK;
  if (c->pinned) (void)hipHostFree(c->pinned);
  c->pinned = nullptr;
  c->pinned_cap = 0;
  size_t cap = std::max(bytes + bytes / 4, (size_t)1 << 20);
  if (hipHostMalloc(&c->pinned, cap, hipHostMallocDefault) != hipSuccess)
    return set_err(FI_ENOMEM, "hipHostMalloc(%zu) failed", cap);
  c->pinned_cap = cap;
  return FI_OK;
}

hipEvent_t fi::get_event(fi_ctx *c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
void fi::collect_ranges(fi_ctx *c, std::vector<TimedRange> &ranges) {
  for (auto &r : ranges) {
    float ms = 0;
    (void)hipEventSynchronize(r.b);
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    Stat &s = c->stats[r.name];
    s.ms += ms;
    s.launches += 1;
    s.bytes += r.bytes;
    c->event_pool.push_back(r.a);
    c->event_pool.push_back(r.b);
  }
  ranges.clear();
}
void fi::collect_timers(fi_ctx *c) { collect_ranges(c, c->pending); }

// ---- device table heaps (fi_ctx::Heap) ------------------------------------
constexpr size_t kHeapI = (size_t)1 << 30, kHeapF = (size_t)128 << 20, kHeapD = (size_t)128 << 20;  // elements
constexpr size_t kAxisCacheMax = 8192, kScCacheMax = 4096, kImpCacheMax = 1024;

void fi::heap_reset(fi_ctx *c) {
  // work queued on either stream may still read tables the next batch overwrites
  sync_streams(c);
  c->heap_i.used = c->heap_f.used = c->heap_d.used = 0;
  c->axis_at.clear();
  c->axis_wd_at.clear();
  c->sc_at.clear();
  c->imp_at.clear();
  c->imp2_at.clear();
  c->sgb_at.clear();
  c->vv_at.clear();
  c->vr_at.clear();
  c->mh_at.clear();
  c->hvv_at.clear();
  c->hvh_at.clear();
  c->mono_wts_at = -1;
}
// Before a batch places anything: evict oversized host caches (only here, so
// no cached object a batch holds a pointer to is ever freed under it; the
// heap placements keyed by those objects go with them), reset heaps past
// three-quarters full, and hand the batch the heaps' used marks.
int fi::heap_prepare(fi_ctx *c, Exec &E) {
  if (c->axis_cache.size() > kAxisCacheMax || c->sc_cache.size() > kScCacheMax ||
      c->imp_cache.size() > kImpCacheMax) {
    c->axis_cache.clear();
    c->vmv_cache.clear();
    c->vrv_cache.clear();
    c->vmh_cache.clear();
    c->hvv_cache.clear();
    c->hvh_cache.clear();
    c->sc_cache.clear();
    c->imp_cache.clear();
    heap_reset(c);
  }
  struct H {
    fi_ctx::Heap *h;
    size_t cap, esz;
  } hs[3] = {{&c->heap_i, kHeapI, 4}, {&c->heap_f, kHeapF, 4}, {&c->heap_d, kHeapD, 8}};
  for (auto &x : hs) {
    if (c->host_only) {  // planner timing: offsets only, nothing is written through the heaps
      x.h->cap = x.cap;
      continue;
    }
    if (!x.h->p) {
      if (hipMalloc(&x.h->p, x.cap * x.esz) != hipSuccess) {
        x.h->p = nullptr;
        return set_err(FI_ENOMEM, "hipMalloc(%zu) of the table heap failed on device %d", x.cap * x.esz,
                       c->device);
      }
      x.h->cap = x.cap;
      x.h->used = 0;
    }
  }
  if (c->heap_i.used > c->heap_i.cap / 4 * 3 || c->heap_f.used > c->heap_f.cap / 4 * 3 ||
      c->heap_d.used > c->heap_d.cap / 4 * 3)
    heap_reset(c);
  E.bi = (int64_t)c->heap_i.used;
  E.bf = (int64_t)c->heap_f.used;
  E.bd = (int64_t)c->heap_d.used;
  return FI_OK;
}
bool fi::heap_fits(const fi_ctx *c, const Exec &E) {
  return (size_t)E.bi + E.ai.size() <= c->heap_i.cap && (size_t)E.bf + E.af.size() <= c->heap_f.cap &&
         (size_t)E.bd + E.ad.size() <= c->heap_d.cap;
}
// Enqueue the copies of the batch's new tables (already uploaded in the blob
// at ab + *_off) behind the heaps' used marks; advance the marks (16-element
// aligned, so 16-byte aligned fragment tables stay aligned).
int fi::heap_commit(fi_ctx *c, Exec &E, const uint8_t *ab, size_t ai_off, size_t af_off, size_t ad_off) {
  static const bool heap_debug = getenv("FI_HEAP_DEBUG") != nullptr;
  if (heap_debug)
    fprintf(stderr, "heap: ai %zu af %zu ad %zu\n", E.ai.size(), E.af.size(), E.ad.size());
  if (!E.ai.empty())
    HIP_TRY(hipMemcpyAsync((int32_t *)c->heap_i.p + E.bi, ab + ai_off, E.ai.size() * 4, hipMemcpyDeviceToDevice,
                           c->stream));
  if (!E.af.empty())
    HIP_TRY(hipMemcpyAsync((float *)c->heap_f.p + E.bf, ab + af_off, E.af.size() * 4, hipMemcpyDeviceToDevice,
                           c->stream));
  if (!E.ad.empty())
    HIP_TRY(hipMemcpyAsync((double *)c->heap_d.p + E.bd, ab + ad_off, E.ad.size() * 8, hipMemcpyDeviceToDevice,
                           c->stream));
  c->heap_i.used = ((size_t)E.bi + E.ai.size() + 15) / 16 * 16;
  c->heap_f.used = ((size_t)E.bf + E.af.size() + 15) / 16 * 16;
  c->heap_d.used = ((size_t)E.bd + E.ad.size() + 15) / 16 * 16;
  if (c->timing) c->stats["heap_upload"].bytes += (double)(E.ai.size() * 4 + E.af.size() * 4 + E.ad.size() * 8);
  return FI_OK;
}

double fi::now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
void fi::host_stat(fi_ctx *c, const char *name, double ms) {
  if (!c->timing) return;
  Stat &s = c->stats[name];
  s.ms += ms;
  s.launches += 1;
}

extern "C" {

const char *fi_last_error(void) { return g_err.c_str(); }

int fi_device_count(int32_t *count) {
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  *count = n;
  return FI_OK;
}

int fi_create(fi_ctx **out, int32_t device) {
  if (!out) return set_err(FI_EINVAL, "out is NULL");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return set_err(FI_EINVAL, "device %d out of range (%d visible)", device, n);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_err(FI_EDEVICE, "device %d is %s; libflyimg_hip.so is built for gfx950 only", device, prop.gcnArchName);
  fi_ctx *c = new fi_ctx();
  c->device = device;
  // Kernel selection is by geometry and LDS fit; three switches keep the
  // fallbacks testable on geometries that would not reach them otherwise:
  //   FI_FORCE_GENERIC=1   the generic two-pass resample and per-row smartcrop kernels
  //   FI_VR_RS=0           k_rs_vm instead of k_rs_vr (vertical-first)
  //   FI_VR_NL=2|4, FI_VR_PBUF=1|2  k_rs_vr's loader waves / plane buffers (where valid)
  //   FI_DISABLE_SC_FZ=1   k_sc_hmfma + k_sc_vq instead of the fused k_sc_fz
  if (const char *e = getenv("FI_FORCE_GENERIC")) c->fast_rs = c->sc_prep = !(e[0] == '1');
  if (const char *e = getenv("FI_VR_RS")) c->vr_rs = e[0] == '1';
  if (const char *e = getenv("FI_VR_NL")) c->vr_nl = atoi(e);
  if (const char *e = getenv("FI_VR_SPLIT")) c->vr_split = e[0] == '1';
  if (const char *e = getenv("FI_VR_NARROW")) c->vr_narrow = e[0] == '1';
  if (const char *e = getenv("FI_UP_SYNC")) c->up_hostsync = e[0] == '1';
  if (const char *e = getenv("FI_VR_PBUF")) c->vr_pbuf = atoi(e);
  if (const char *e = getenv("FI_DISABLE_SC_FZ")) c->sc_fz = !(e[0] == '1');
  if (const char *e = getenv("FI_SC_FD")) c->sc_fd = e[0] == '1';
  if (const char *e = getenv("FI_SC_CX")) c->sc_cx = atoi(e);
  if (const char *e = getenv("FI_SC_MFMA")) c->sc_mf = e[0] == '1';
  if (const char *e = getenv("FI_VR_MAX_CLASSES")) c->vr_max_classes = atoi(e);
  if (const char *e = getenv("FI_VM_LPT")) c->vm_lpt = e[0] == '1';
  if (const char *e = getenv("FI_RES_ALIGN")) c->res_align = std::max(1, atoi(e));
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // (the smartcrop stage on a stream of its own beside the next batch's
  // resample was measured in round 2: the resample fills every CU, so the
  // overlap only stretched both -- one stream)
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return set_err(FI_EDEVICE, "hipStreamCreate failed");
  }
  c->sc_stream = c->stream;
  if (const char *e = getenv("FI_APPLY_OVERLAP")) c->apply_overlap = e[0] == '1';
  if (const char *e = getenv("FI_VR_FORK")) c->vr_fork = e[0] == '1';
  // ap_stream at the higher priority: its score / apply take the CUs the
  // resample frees before the next resample's workgroups do
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->rb_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithPriority(&c->ap_stream, hipStreamNonBlocking, prio_hi) != hipSuccess ||
      hipStreamCreateWithFlags(&c->rs2_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->gx_stream, hipStreamNonBlocking) != hipSuccess) {
    fi_destroy(c);
    return set_err(FI_EDEVICE, "hipStreamCreate failed");
  }
  *out = c;
  return FI_OK;
}

void fi_destroy(fi_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)drain(c);
  sync_streams(c);
  if (c->comm) ncclCommDestroy(c->comm);
  for (DevBuf *b : {&c->arena, &c->work, &c->io, &c->gather, &c->pix, &c->skinsat, &c->jpeg[0], &c->jpeg[1],
                    &c->jpeg[2], &c->jpeg_enc[0], &c->jpeg_enc[1], &c->jpeg_enc[2]})
    if (b->p) (void)hipFree(b->p);
  // the table heaps (5.5 GiB of device memory a context; a host-only planner context has none)
  for (fi_ctx::Heap *h : {&c->heap_i, &c->heap_f, &c->heap_d})
    if (h->p) (void)hipFree(h->p);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->jpeg_host) (void)hipHostFree(c->jpeg_host);
  if (c->jpeg_enc_host) (void)hipHostFree(c->jpeg_enc_host);
  for (Slot &sl : c->slots) {
    if (sl.blob) (void)hipHostFree(sl.blob);
    if (sl.res) (void)hipHostFree(sl.res);
    if (sl.hpin) (void)hipHostFree(sl.hpin);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.rs_done) (void)hipEventDestroy(sl.rs_done);
    if (sl.up_done) (void)hipEventDestroy(sl.up_done);
    if (sl.sc_end) (void)hipEventDestroy(sl.sc_end);
    if (sl.sc_done) (void)hipEventDestroy(sl.sc_done);
    for (DevBuf *b : {&sl.arena, &sl.work, &sl.hio})
      if (b->p) (void)hipFree(b->p);
  }
  for (auto e : c->event_pool) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(c->stream);
  if (c->sc_stream != c->stream) (void)hipStreamDestroy(c->sc_stream);
  if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
  if (c->rb_stream) (void)hipStreamDestroy(c->rb_stream);
  if (c->ap_stream) (void)hipStreamDestroy(c->ap_stream);
  if (c->rs2_stream) (void)hipStreamDestroy(c->rs2_stream);
  if (c->gx_stream) (void)hipStreamDestroy(c->gx_stream);
  if (c->rs_fork) (void)hipEventDestroy(c->rs_fork);
  if (c->rs_join) (void)hipEventDestroy(c->rs_join);
  if (c->ap_tail) (void)hipEventDestroy(c->ap_tail);
  if (c->gx_done) (void)hipEventDestroy(c->gx_done);
  if (c->gx_pin) (void)hipHostFree(c->gx_pin);
  delete c;
}

void *fi_host_alloc(fi_ctx *c, size_t bytes) {
  if (!c || bytes == 0) return nullptr;
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
    set_err(FI_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return p;
}

int fi_host_free(fi_ctx *c, void *p) {
  if (!c) return set_err(FI_EINVAL, "bad arguments");
  if (p) HIP_TRY(hipHostFree(p));
  return FI_OK;
}

int fi_device_malloc(fi_ctx *c, void **ptr, uint64_t bytes) {
  if (!c || !ptr) return set_err(FI_EINVAL, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  if (hipMalloc(ptr, bytes) != hipSuccess) return set_err(FI_ENOMEM, "hipMalloc(%llu) failed", (unsigned long long)bytes);
  return FI_OK;
}
int fi_device_free(fi_ctx *c, void *ptr) {
  if (!c) return set_err(FI_EINVAL, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipFree(ptr));
  return FI_OK;
}
int fi_memcpy_h2d(fi_ctx *c, void *dst, const void *src, uint64_t bytes) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return FI_OK;
}
int fi_memcpy_d2h(fi_ctx *c, void *dst, const void *src, uint64_t bytes) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return FI_OK;
}
int fi_fill_synthetic(fi_ctx *c, uint8_t *dev, int32_t w, int32_t h, int32_t stride, uint32_t seed) {
  if (!c || !dev || w <= 0 || h <= 0 || stride < 3 * w) return set_err(FI_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (order_after_apply(c) != FI_OK) return set_err(FI_EDEVICE, "hipStreamWaitEvent failed");
  const int64_t n = (int64_t)w * h;
  hipLaunchKernelGGL(k_synth, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, dev, w, h, (int64_t)stride,
                     seed);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return FI_OK;
}

int fi_set_timing(fi_ctx *c, int32_t enable) {
  if (!c) return set_err(FI_EINVAL, "ctx is NULL");
  c->timing = enable != 0;
  c->timing_resize_only = enable == 2;
  return FI_OK;
}
int fi_reset_stats(fi_ctx *c) {
  if (!c) return set_err(FI_EINVAL, "ctx is NULL");
  c->stats.clear();
  return FI_OK;
}
int fi_kernel_stats(fi_ctx *c, const char *name, double *total_ms, int64_t *launches, double *bytes) {
  if (!c || !name) return set_err(FI_EINVAL, "bad arguments");
  auto it = c->stats.find(name);
  const Stat s = it == c->stats.end() ? Stat{} : it->second;
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.launches;
  if (bytes) *bytes = s.bytes;
  return FI_OK;
}

}  // extern "C"
