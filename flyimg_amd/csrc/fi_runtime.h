// fi_runtime.h -- internal to the C-ABI runtime of libflyimg_hip.so
// (include/flyimg_hip.h): what more than one of its files needs.  The files:
// fi_context.cpp, fi_rs_plan.cpp, fi_tiles.cpp, fi_sc_plan.cpp, fi_batch.cpp,
// fi_jpeg_api.cpp, fi_rccl.cpp, fi_api.cpp.
//
// One fi_ctx per process per GPU.  A batch call:
//   1. plans every image on the host (fi_plan*.cpp): ImageMagick geometry,
//      merged tap tables, Pillow prescale tables, smartcrop crop windows and
//      importance tables -- deduplicated per geometry and cached across calls;
//   2. packs descriptors + tables into ONE pinned blob and uploads it with
//      one hipMemcpyAsync;
//   3. launches the kernels of each stage once for the whole batch (per-image
//      descriptors, flat tile index -> image by prefix search);
//   4. reads back the per-image result records.
#ifndef FI_RUNTIME_H
#define FI_RUNTIME_H
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "fi_internal.h"
#include "fi_plan.h"

namespace fi {
// kernels (fi_kernels.hip)
__global__ void k_rs_v_u8(const ResizeDesc *, const int32_t *, int, const int32_t *, const float *);
__global__ void k_rs_h_final(const ResizeDesc *, const int32_t *, int, const int32_t *, const float *);
__global__ void k_rs_h_u8(const ResizeDesc *, const int32_t *, int, const int32_t *, const float *);
__global__ void k_rs_v_final(const ResizeDesc *, const int32_t *, int, const int32_t *, const float *);
__global__ void k_rs_copy(const ResizeDesc *, const int32_t *, int);
__global__ void k_sc_reduce(const ScDesc *, const int32_t *, int);
__global__ void k_sc_hpass(const ScDesc *, const int32_t *, int, const int32_t *);
__global__ void k_sc_vpass(const ScDesc *, const int32_t *, int, const int32_t *);
__global__ void k_sc_maps(const ScDesc *, const int32_t *, int, const ScParamsDev);
// per-image smartcrop kernels (fi_sc_prep.hip; launch_sc_score* in fi_sc_score.hip, launch_crop_apply in fi_sc_apply.hip)
int launch_sc_h(hipStream_t s, const ScDesc *descs, int n, int chunks, int lds, const int32_t *ai);
int launch_sc_v(hipStream_t s, const ScDesc *descs, int n, int chunks, int lds, const int32_t *ai,
                const ScParamsDev &P);
int launch_sc_vq(hipStream_t s, const ScDesc *descs, int n, int chunks, int lds, const int32_t *ai,
                 const ScParamsDev &P);
int launch_sc_fz(hipStream_t s, const ScDesc *descs, int n, int lds, const int32_t *ai, const ScParamsDev &P,
                 const uint16_t *skinsat);
int launch_sc_fd(hipStream_t s, const ScDesc *descs, int n, int lds, const int32_t *ai, const ScParamsDev &P,
                 const uint16_t *skinsat);
int launch_sc_hx(hipStream_t s, int ks, int nch, const ScDesc *descs, const int32_t *tiles, int ntiles,
                 const int32_t *ai);
int launch_sc_vx(hipStream_t s, int kv, int nch, const ScDesc *descs, const int32_t *tiles, int ntiles,
                 const int32_t *ai, const ScParamsDev &P, const uint16_t *skinsat);
int launch_sc_skinsat(hipStream_t s, uint16_t *table, const ScParamsDev &P);
int jpeg_decode_batch(hipStream_t st, const uint8_t *const *data, const size_t *len, int n, uint8_t *const *dst,
                      const int64_t *dst_stride, int out_channels, uint32_t flags, const fi_jpeg_view *views,
                      int32_t *status, void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *),
                      void *actx, std::string *err);
int jpeg_encode_batch(hipStream_t st, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                      const int32_t *channels, const int64_t *src_stride, const int32_t *quality,
                      const int32_t *subsampling, int n, uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                      int32_t *status, void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *),
                      void *actx, std::string *err);
// the same batch as progressive files with optimal tables (fi_jpeg_penc.hip)
int jpeg_pencode_batch(hipStream_t st, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                       const int32_t *channels, const int64_t *src_stride, const int32_t *quality,
                       const int32_t *subsampling, int n, uint8_t *const *out, const size_t *out_cap, size_t *out_len,
                       int32_t *status, void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *),
                       void *actx, std::string *err);
int png_encode_batch(hipStream_t st, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                     const int32_t *channels, const int64_t *src_stride, const int32_t *filter, int n,
                     uint8_t *const *out, const size_t *out_cap, size_t *out_len, int32_t *status,
                     void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *), void *actx,
                     std::string *err);
int webp_encode_batch(hipStream_t st, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                      const int32_t *channels, const int64_t *src_stride, const int32_t *predictor, int n,
                      uint8_t *const *out, const size_t *out_cap, size_t *out_len, int32_t *status,
                      void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *), void *actx,
                      std::string *err);
int png_decode_batch(hipStream_t st, const uint8_t *const *data, const size_t *len, int n, uint8_t *const *dst,
                     const int64_t *dst_stride, const int32_t *out_channels, int32_t *status,
                     void *(*alloc)(void *, int, size_t), void (*stage)(void *, const char *), void *actx,
                     std::string *err);
int launch_sc_score(hipStream_t s, int mode, const ScDesc *descs, int n, size_t lds, const DevCrop *crops,
                    const double *ad, CropScore *scores, ScResult *results, const ScParamsDev &P, const int32_t *ai);
int launch_sc_score3(hipStream_t s, const ScDesc *descs, int n, size_t lds, const DevCrop *crops, const ScGroup *groups,
                     const double *ad, CropScore *scores, ScResult *results, const ScParamsDev &P, const int32_t *ai);
int launch_crop_apply(hipStream_t s, const ApplyDesc *descs, int n, const DevCrop *crops, const ScResult *results,
                      int persistent_wgs);
__global__ void k_synth(uint8_t *, int, int, int64_t, uint32_t);
// tiled horizontal-first pass 1 (fi_kernels.hip)
constexpr int kHTileRows = 16;  // fi_kernels.hip kHTRows
size_t rs_h_tile_lds(int pitch, int taps);
int launch_conv(hipStream_t s, int mode, const ConvStep *steps, const int32_t *prefix, int n, int tiles,
                const double *ad);
int launch_rs4(hipStream_t s, int mode, const ResizeDesc *d1, const int32_t *p1, int n1, int tiles1,
               const ResizeDesc *d2, const int32_t *p2, int n2, int tiles2, const int32_t *ai, const double *ad);
int launch_rs_h_tile(hipStream_t s, const ResizeDesc *descs, const int32_t *prefix, int n, int tiles,
                     const int32_t *ai, const float *af, int pitch, int taps);
// shear rotation (fi_rotate.hip)
int launch_rot(hipStream_t s, const RotDesc *descs, const int32_t *prefix, int n, int tiles);
void rot_host(const RotDesc &D);  // the kernel's per-pixel procedure on the host (host pointers)
// -monochrome (fi_mono.hip)
size_t mono_lds_bytes();
int launch_mono(hipStream_t s, const MonoDesc *descs, int n, const double *wts);
// streaming exact-integer MFMA resample (fi_vm.hip)
size_t vm_lds_bytes(int vpitch, int nocb, int ks, bool q16);
int vm_read_stamps(uint64_t *out, int slots);
int launch_vm(hipStream_t s, const VDesc *descs, const MStrip *strips, const VTile *tiles, int ntiles,
              const int32_t *ai, size_t lds);
// its persistent block-major form (fi_vr.hip)
VrLayout vr_lds_layout(int vpitch, bool q16, int pbuf);
int launch_vr(hipStream_t s, const VDesc *descs, const MStrip *strips, const VrTile *tiles, int ntiles,
              const int32_t *wginfo, int G, const int32_t *ai, VrLayout L);
int vr_read_stamps(uint64_t *out, int slots);
// streaming exact-integer MFMA resample, horizontal first (fi_hv.hip)
size_t hv_lds_bytes(int pp, int nocb);
int launch_hv(hipStream_t s, const HvDesc *descs, const HvStripD *strips, const HvTile *tiles, int ntiles,
              const int32_t *ai, size_t lds);
// face-blur pixelation (fi_pixelate.hip)
int launch_pix(hipStream_t s, int mode, const PixPass &P, const int32_t *ai, const double *ad);

struct Exec;
struct Timer;
int set_err(int code, const char *fmt, ...);
}  // namespace fi

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fi::set_err(FI_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                         __LINE__);                                                                \
  } while (0)

namespace fi {
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
};
struct Stat {
  double ms = 0;
  int64_t launches = 0;
  double bytes = 0;
};
struct TimedRange {
  std::string name;
  hipEvent_t a, b;
  double bytes;
};

// A host-buffer batch (fi_submit_batch / fi_process_batch): the caller's
// records, the device-side records run_batch fills, and where each output
// goes -- straight into a pinned caller dst, or through the slot's pinned
// staging (pageable dst) with one memcpy at fi_wait.
struct HostIo {
  fi_image *user = nullptr;
  std::vector<fi_image> dev;
  std::vector<size_t> dev_dst_off;  // per image: its device dst in the slot's hio buffer
  std::vector<int64_t> pin_off;     // per image: offset in the slot's pinned staging, -1 = dst is pinned
};
// One in-flight batch (fi_submit_batch[_device]): what fi_wait needs to fill
// the caller's fi_image records once the stream has drained.
struct PendingBatch {
  fi_image *imgs = nullptr;
  int n = 0;
  int slot = 0;
  double t_start = 0;
  std::vector<int> status, sc_of;
  std::vector<std::string> errs;
  std::vector<int> sstatus;
  std::vector<std::string> serrs;
  std::vector<int32_t> crop0;   // per smartcrop item: first crop of its list
  std::vector<fi::DevCrop> crops;
  size_t nres = 0;              // ScResult records in the slot's pinned readback
  bool any_apply = false;
  std::vector<TimedRange> timers;  // this batch's HIP-event ranges
  std::shared_ptr<HostIo> host;    // host-buffer batches only
};
// Pinned host staging of one in-flight batch: the upload blob and the result
// readback.  Two slots: batch k+1 is planned and uploaded while batch k runs.
struct Slot {
  void *blob = nullptr;
  size_t blob_cap = 0;
  void *res = nullptr;
  size_t res_cap = 0;
  hipEvent_t done = nullptr;  // recorded after the batch's last readback (rb_stream for host outputs, else the batch stream)
  hipEvent_t rs_done = nullptr;  // resample stage of the batch done (main stream)
  hipEvent_t up_done = nullptr;  // the batch's sources / blob uploaded (up_stream)
  hipEvent_t sc_end = nullptr;   // the batch's last kernel done (on its tail stream)
  hipEvent_t sc_done = nullptr;  // the batch's smartcrop stage done (sc_stream; the crop apply waits for it)
  hipStream_t tail = nullptr;    // the stream of the batch's last kernel (sc_stream, or ap_stream with the apply)
  uintptr_t ap_lo = 0, ap_hi = 0;  // bytes its overlapped crop apply writes (empty: none pending)
  bool busy = false;
  // device buffers of the in-flight batch: the uploaded blob (descriptors) and
  // the workspace (intermediates, smartcrop scratch, scores, results).  Per
  // slot, because batch k+1's upload and resample run while batch k's
  // smartcrop stage still reads its own.
  DevBuf arena, work;
  // host-buffer batches: device copies of the sources / outputs, and the pinned
  // staging of pageable sources and outputs
  DevBuf hio;
  void *hpin = nullptr;
  size_t hpin_cap = 0;
};
// three batches in flight: with the smartcrop stage beside the next resample,
// batch k's stage finishes after batch k+1's resample, and batch k+2's must
// already be queued behind it (two slots serialise the host on batch k)
constexpr int kSlots = 3;
// hash of the planner's cache keys (tuples / pairs of ints, doubles' bits and
// pointers): the per-image lookups of a mixed batch run in O(1) (a std::map
// over thousands of tables cost ~1 us per lookup in cache misses)
struct KeyHash {
  template <class T>
  static void mix(size_t &h, const T &v) {
    h ^= std::hash<T>()(v) + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
  }
  template <class... A>
  size_t operator()(const std::tuple<A...> &t) const {
    size_t h = 0;
    std::apply([&](const auto &...x) { (mix(h, x), ...); }, t);
    return h;
  }
  template <class A, class B>
  size_t operator()(const std::pair<A, B> &p) const {
    size_t h = 0;
    mix(h, p.first);
    mix(h, p.second);
    return h;
  }
  template <class T>
  size_t operator()(T *p) const {
    size_t h = 0;
    mix(h, (uintptr_t)p);
    return h;
  }
};
template <class K, class V>
using HashMap = std::unordered_map<K, V, KeyHash>;
}  // namespace fi

// (fi_ctx is the C ABI's opaque type, so it is global; the runtime's files all
// work inside namespace fi's names)
using namespace fi;

struct fi_ctx {
  int device = 0;
  Slot slots[kSlots];
  int next_slot = 0;
  std::vector<PendingBatch> inflight;  // submission order
  hipStream_t stream = nullptr;     // upload, resample, mono
  hipStream_t sc_stream = nullptr;  // smartcrop stage + crop apply of a batch (waits for its resample)
  // copies off the kernel streams: batch k+1's uploads run during batch k's
  // kernels, batch k's readback during batch k+1's (the main stream waits for
  // up_done, the readback for sc_end; one slot's buffers per batch)
  hipStream_t up_stream = nullptr, rb_stream = nullptr;
  // the crop apply of batch k beside batch k+1's resample (one workgroup per
  // CU, no LDS: it fits next to k_rs_vr's); FI_APPLY_OVERLAP=0: on sc_stream
  hipStream_t ap_stream = nullptr;
  bool apply_overlap = true;
  // a batch with two or more k_rs_vr launches (mixed strip widths) runs the
  // second and later ones on rs2_stream, forked from and joined back into
  // `stream` inside the resize stage, so each persistent launch's tail (its
  // unevenly loaded workgroups finishing) is filled by the other's workgroups
  // instead of idling the CUs it frees; FI_VR_FORK=0: all on `stream`
  hipStream_t rs2_stream = nullptr;
  hipEvent_t rs_fork = nullptr, rs_join = nullptr;
  bool vr_fork = true;
  // recorded on ap_stream after every overlapped apply: entry points that
  // launch on `stream` and may touch a batch's dst (face-blur, JPEG decode,
  // synthetic fill, a later batch whose sources are an earlier batch's
  // outputs) wait for it (order_after_apply), so the stream order the header
  // promises holds across the two streams
  hipEvent_t ap_tail = nullptr;
  bool ap_pending = false;
  // RCCL record gather: its own stream (no dependency on the batch streams),
  // pinned staging, at most one gather in flight (fi_rccl_gather_start / _finish)
  hipStream_t gx_stream = nullptr;
  hipEvent_t gx_done = nullptr;
  void *gx_pin = nullptr;
  size_t gx_pin_cap = 0;
  bool gx_pending = false;
  fi_record *gx_recv = nullptr;  // caller's receive buffer of the gather in flight (rank 0)
  size_t gx_recv_bytes = 0;
  std::mutex mu;
  DevBuf arena, work, io;
  DevBuf gather;  // RCCL record gather staging
  DevBuf pix;     // face-blur pixelation: lists + 10% scratch
  void *pinned = nullptr;
  size_t pinned_cap = 0;
  bool timing = false;
  std::map<std::string, Stat> stats;
  std::vector<hipEvent_t> event_pool;
  std::vector<TimedRange> pending;
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  // caches (host planning is deterministic, keyed by geometry)
  HashMap<std::tuple<int, uint64_t, int, int, int, int, int, int>, AxisTable> axis_cache;
  HashMap<std::tuple<int, int, int, int, uint64_t>, ScPlan> sc_cache;
  std::map<std::tuple<uint64_t, uint64_t, int, int, uint64_t>, std::vector<double>> imp_cache;
  bool fast_rs = true;  // FI_FORCE_GENERIC=1: the generic two-pass resample (and smartcrop) kernels only
  bool vr_rs = true;     // images with block-major tables take the persistent k_rs_vr (FI_VR_RS=0: k_rs_vm)
  int vr_nl = 0;         // k_rs_vr loader waves forced (FI_VR_NL=2 / 4; 0: by geometry)
  bool vr_split = true;  // k_rs_vr: one-block strips in a launch of their own (FI_VR_SPLIT=0: one launch)
  bool vr_narrow = true;  // 48-px strips where 64-px ones would have four blocks (FI_VR_NARROW=0: off)
  bool up_hostsync = true;  // device batches' blob upload waited for on the host (FI_UP_SYNC=0: by the main stream)
  int vr_pbuf = 0;       // k_rs_vr plane buffers forced (FI_VR_PBUF=1 / 2; 0: by ring room)
  int vr_max_classes = 1 << 30;  // batches with more vertical tables stay on k_rs_vm (FI_VR_MAX_CLASSES)
  bool vm_lpt = true;      // k_rs_vm tiles: LPT images -> XCDs, longest tiles first (FI_VM_LPT=0: round robin)
  int res_align = 16;      // row pitch alignment of the resized image kept for smartcrop apply (FI_RES_ALIGN)
  bool timing_resize_only = false;  // fi_set_timing(2): stage timing events around the resample only
  int n_cu = 256;        // compute units (k_rs_vr: one persistent workgroup per CU)
  bool sc_fz = true;        // FI_DISABLE_SC_FZ=1: k_sc_hmfma + k_sc_vq instead of the fused k_sc_fz
  bool sc_fd = true;        // FI_SC_FD=0: k_sc_fz instead of its LDS-DMA form k_sc_fd
  // k_sc_hx + k_sc_vx (no LDS, <= 64 VGPRs; gray sources, two-k-step
  // vertical windows): FI_SC_CX=0 never; 1 (default) for the gray images none
  // of k_sc_fd / k_sc_fz takes (cfg5's 400 -> 111, which otherwise
  // runs k_sc_hmfma + k_sc_vmaps); 2 for every image it fits; 3 the same, and a
  // batch whose smartcrop images all take them runs the stage on ap_stream
  // beside the next batch's resample (measured a loss on cfg2: DESIGN.md §3.2)
  int sc_cx = 1;
  bool sc_mf = true;        // FI_SC_MFMA=0: k_sc_score2 (f64 VALU fast pass) instead of k_sc_score3
  DevBuf skinsat;           // k_sc_skinsat table: 2^24 colours x u16, built for skinsat_key's parameters
  DevBuf jpeg[3];           // GPU JPEG decode: upload (compressed data + tables), -, coefficients + planes
  void *jpeg_host = nullptr;  // its pinned staging
  size_t jpeg_host_cap = 0;
  DevBuf jpeg_enc[3];       // GPU JPEG / PNG encode: upload (tables + headers), coefficients + slots, packed streams
  void *jpeg_enc_host = nullptr;  // its pinned staging (upload, then download)
  size_t jpeg_enc_host_cap = 0;
  struct Timer *jpeg_enc_timer = nullptr;  // the encode kernel being timed (fi_jpeg_encode_device)
  std::string skinsat_key;
  HashMap<const AxisTable *, VmV> vmv_cache;   // ok iff nblk > 0
  HashMap<const AxisTable *, VrV> vrv_cache;   // ok iff nblk > 0
  HashMap<std::pair<const AxisTable *, bool>, MfmaH> vmh_cache; // strips of <= kVmMaxNx px; ok iff !strips.empty()
  HashMap<const AxisTable *, HvV> hvv_cache;  // ok iff nblk > 0
  HashMap<const AxisTable *, HvH> hvh_cache;  // ok iff !strips.empty()
  bool sc_prep = true;  // FI_DISABLE_SC_PREP=1 forces the generic per-row smartcrop kernels
  // Device-resident table heaps: every per-geometry table (tap tables, MFMA
  // fragments, Pillow coefficients, importance tables) is uploaded once and
  // stays at a fixed offset; a batch uploads only the tables it adds.  The
  // heaps are append-only between resets, and a reset only ever happens
  // between batches: work queued earlier on the (in-order) stream has read
  // its tables before any later copy overwrites them.
  struct Heap {
    void *p = nullptr;
    size_t cap = 0, used = 0;  // elements
  };
  Heap heap_i, heap_f, heap_d;  // int32 / float / double
  // absolute heap offsets of placed tables, keyed by the cached host object
  struct ScTabs {
    int32_t hb = 0, hk = 0, hkT = 0, vb = 0, vk = 0;
    int32_t hmB = 0, hmC = 0, hmS0 = 0, vqA = 0, vqC = 0, vqK0 = 0;
    int32_t cxA = -1, cxK0 = -1;
  };
  HashMap<const AxisTable *, DevAxis> axis_at;
  HashMap<const AxisTable *, int32_t> axis_wd_at;  // f64 weights (RGBA path) in heap_d
  HashMap<const ScPlan *, ScTabs> sc_at;
  std::map<std::pair<const std::vector<double> *, int>, std::pair<int32_t, double>> imp_at;
  std::map<std::pair<const std::vector<double> *, int>, std::pair<int32_t, double>> imp2_at;  // importance - oi
  // k_sc_score3 B fragments: (table, nx, nslot, step) -> heap offset + the table's digit sums / q
  std::map<std::tuple<const std::vector<double> *, int, int, int>, std::pair<int32_t, ScoreBTab>> sgb_at;
  HashMap<const VmV *, std::array<int32_t, 8>> vv_at;
  HashMap<const VrV *, std::array<int32_t, 4>> vr_at;    // rows, bmeta, w128, frag
  // horizontal tables placed: the strips' device descriptors (heap offsets
  // resolved) and the k_rs_vm LDS of their widest strip, kept with the
  // placement so a batch copies them contiguously instead of re-deriving them
  // from the (cold) MfmaH per batch
  struct MhPlaced {
    int32_t hwsum = 0, hwsum2 = 0;
    size_t lds8 = 0, lds16 = 0;  // k_rs_vm LDS with an 8-bit / Q16 output tile
    std::vector<MStrip> strips;
  };
  HashMap<const MfmaH *, MhPlaced> mh_at;
  HashMap<const HvV *, std::array<int32_t, 3>> hvv_at;   // k0ks, frag, wsum
  HashMap<const HvH *, std::array<int32_t, 3>> hvh_at;   // w128, frag, s0
  int32_t mono_wts_at = -1;
  bool heap_retry = false;
  bool host_only = false;  // fi_debug_host_plan: planner only, no device (no allocation, no stream)
};


namespace fi {
hipEvent_t get_event(fi_ctx *c);
struct Timer {  // HIP-event range: starts on stream sa, ends on stream sb
  fi_ctx *c;
  TimedRange r;
  bool on;
  hipStream_t sb;
  Timer(fi_ctx *c_, const char *name, double bytes) : Timer(c_, name, bytes, c_->stream, c_->stream) {}
  Timer(fi_ctx *c_, const char *name, double bytes, hipStream_t sa, hipStream_t sb_)
      : c(c_), on(c_->timing && (!c_->timing_resize_only || strcmp(name, "resize") == 0)), sb(sb_) {
    if (!on) return;
    r.name = name;
    r.bytes = bytes;
    r.a = get_event(c);
    r.b = get_event(c);
    (void)hipEventRecord(r.a, sa);
  }
  ~Timer() {
    if (!on) return;
    (void)hipEventRecord(r.b, sb);
    c->pending.push_back(r);
  }
};
struct Blob {
  std::vector<uint8_t> b;
  size_t add(const void *p, size_t n, size_t align = 256) {
    size_t off = (b.size() + align - 1) / align * align;
    b.resize(off + n);
    if (n) memcpy(b.data() + off, p, n);
    return off;
  }
  template <class T>
  size_t addv(const std::vector<T> &v) {
    return add(v.data(), v.size() * sizeof(T));
  }
};
struct Work {  // workspace sub-allocator (device offsets)
  size_t size = 0;
  size_t take(size_t n, size_t align = 256) {
    size_t off = (size + align - 1) / align * align;
    size = off + n;
    return off;
  }
};

inline uint64_t dbits(double d) {
  uint64_t u;
  memcpy(&u, &d, 8);
  return u;
}

struct ScItem {       // one smartcrop job
  const uint8_t *img;  // device
  int64_t stride;
  int W, H, C;
  int tw, th;
  int result;          // index into results
  fi_smartcrop_options opt;
  bool padded = false; // every row readable to fd_rp(W) bytes (library-owned buffers)
};

struct Exec {
  fi_ctx *c;
  Blob blob;
  Work work;
  // tables this batch adds to the device heaps (uploaded behind the heaps'
  // used marks bi / bf / bd, which are multiples of 16 elements)
  std::vector<int32_t> ai;
  std::vector<float> af;
  std::vector<double> ad;
  int64_t bi = 0, bf = 0, bd = 0;
  int32_t oi() const { return (int32_t)(bi + (int64_t)ai.size()); }
  int32_t of() const { return (int32_t)(bf + (int64_t)af.size()); }
  int32_t od() const { return (int32_t)(bd + (int64_t)ad.size()); }
  void align4() {  // the next int32 table starts on 16 bytes
    while (ai.size() % 4) ai.push_back(0);
  }
  int32_t put(const std::vector<int32_t> &v) {  // append an int32 table; its heap offset
    const int32_t o = oi();
    ai.insert(ai.end(), v.begin(), v.end());
    return o;
  }
  fi_smartcrop_params params;
};

struct ScLaunchData {
  std::vector<ScDesc> descs;
  std::vector<DevCrop> crops;  // one list per distinct plan, shared by its images
  std::vector<ScGroup> groups; // k_sc_score3 groups, shared like the crops
  int nscores = 0;             // per-image CropScore slots
  std::vector<const ScPlan *> plans;
};

template <class D>
inline void fix_ptr(D *&p, uint8_t *base) {
  if (p) p = reinterpret_cast<D *>(base + ((uintptr_t)p - 1));
}

struct Launch {  // one kernel launch over a subset of descriptors
  size_t desc_off = 0, prefix_off = 0;
  int n = 0, tiles = 0;
};
template <class Desc, class TileFn>
inline Launch add_launch(Blob &blob, const std::vector<Desc> &all, const std::vector<int> &members, TileFn tiles) {
  Launch L;
  std::vector<Desc> sub;
  std::vector<int32_t> prefix;
  int32_t acc = 0;
  for (int m : members) {
    const int t = tiles(all[m]);
    if (t <= 0) continue;
    sub.push_back(all[m]);
    prefix.push_back(acc);
    acc += t;
  }
  prefix.push_back(acc);
  L.n = (int)sub.size();
  L.tiles = acc;
  L.desc_off = blob.addv(sub);
  L.prefix_off = blob.addv(prefix);
  return L;
}

// Launch lists of a planned smartcrop stage: the per-image kernels where the
// plan fits them (k_sc_prep, k_sc_score2), the generic per-row kernels
// otherwise.
struct ScLaunches {
  Launch red, hp, vp, maps;        // generic (fi_kernels.hip)
  size_t hm_off = 0, vq_off = 0, vm_off = 0;   // k_sc_hmfma / k_sc_vq / k_sc_vmaps
  int nhm = 0, hm_chunks = 0, hm_lds = 0, nvm = 0, v_chunks = 0, v_lds = 0;
  size_t fz_off = 0, fd_off = 0;  // k_sc_fz, k_sc_fd
  int nfz = 0, fz_lds = 0, nfd = 0, fd_lds = 0;
  // k_sc_hx / k_sc_vx: descriptors, tile lists per variant v = 2 (k-steps - 1) + (channels == 3)
  size_t cx_off = 0, hxt_off[4] = {0, 0, 0, 0}, vxt_off[4] = {0, 0, 0, 0};
  int ncx = 0, hx_tiles[4] = {0, 0, 0, 0}, vx_tiles[4] = {0, 0, 0, 0};
  int nok = 0;  // descriptors planned OK (ncx == nok: the whole stage is co-resident work)
  int nvq = 0, vq_chunks = 0, vq_lds = 0;
  size_t sl_off = 0, sg_off = 0;   // k_sc_score2 with maps in LDS / global
  int nsl = 0, nsg = 0, sl_px = 0;
  size_t s3_off = 0, groups_off = 0;  // k_sc_score3 (exact-integer MFMA fast pass)
  int ns3 = 0, s3_lds = 0;
  size_t crops_off = 0;
};
struct MonoItem {
  int img;
  size_t g_off, st_off;
};
struct ConvItem {
  int img;
  size_t a_off, b_off;
};
struct RotItem {   // a sheared image: the integral Q16 image in the workspace
  int img;
  size_t q_off;
  int conv;        // index into conv_items when convolutions follow, else -1
};
// Everything a batch plans before it is packed and uploaded.
struct BatchPlan {
  fi_image *imgs = nullptr;
  int n = 0;
  std::vector<ImPlan> plans;
  std::vector<int> status;
  std::vector<std::string> errs;
  std::vector<ResizeDesc> rd;  // resample descriptors of the images that plan
  std::vector<int> rd_of;      // image -> rd index (-1: the image failed)
  std::vector<ScItem> sitems;  // smartcrop jobs
  std::vector<int> sc_of;      // image -> sitems index (-1: none)
  HashMap<const AxisTable *, DevAxis> placed;
  // resample path members (indices into rd) and their tables
  std::vector<int> vm_img;
  std::vector<const VmV *> vm_v;
  std::vector<const MfmaH *> vm_h;
  std::vector<const AxisTable *> vm_vt;  // their vertical axes (k_rs_vr tables)
  std::vector<int> hv_img;
  std::vector<const HvV *> hv_v;
  std::vector<const HvH *> hv_h;
  std::vector<int32_t> hv_W;  // source widths
  int h_tile_pitch = 0;  // k_rs_h_tile: max staged row bytes over the mode-2 images
  int h_tile_taps = 0;   // k_rs_h_tile: max horizontal window over the mode-2 images
  std::vector<size_t> res_off;    // per image: resized buffer in the workspace (smartcrop apply)
  std::vector<int64_t> res_stride;  // per image: the row pitch of out_of (out_stride, or padded in the workspace)
  std::vector<uint8_t *> out_of;  // per image: the final 8-bit output (dst, or the workspace +1-tagged)
  std::vector<MonoItem> mono;
  std::vector<ConvItem> conv_items;
  std::vector<RotItem> rot_items;
  double resize_bytes = 0, rot_bytes = 0;
  // smartcrop stage
  ScLaunchData SL;
  std::vector<int> sstatus;
  std::vector<std::string> serrs;
  size_t results_off = 0, scores_off = 0, outwh_off = 0;
  // resolved against the slot's workspace
  std::vector<MonoDesc> mdesc_mono;
  std::vector<ConvStep> cst[6];  // U-H, U-V+combine, S-2D, B-H, B-V, to8
  std::vector<ApplyDesc> apply;
  std::vector<RotDesc> rdesc_rot;
  // tiles
  std::vector<VDesc> vdescs;
  std::vector<MStrip> vstrips;
  std::vector<VTile> vtiles;
  // k_rs_vr: persistent block-major tiles, per-workgroup {phases, stream rows}, LDS layout
  // (one or more launches: their tiles and per-workgroup info back to back)
  struct VrLaunch {
    int32_t tile0, ntiles, info0, G, images;
    VrLayout L;
  };
  std::vector<VrTile> vrtiles;
  std::vector<int32_t> vr_info;
  std::vector<VrLaunch> vrl;
  size_t vm_lds = 0;
  std::vector<HvDesc> hdescs;
  std::vector<HvStripD> hstrips;
  std::vector<HvTile> htiles;
  size_t hv_lds = 0;
};
// Blob offsets and launch lists of a packed batch.
struct Packed {
  size_t all_rd_off = 0, vdesc_off = 0, vstrip_off = 0, vtile_off = 0, apply_off = 0, mono_off = 0;
  size_t vrtile_off = 0, vrinfo_off = 0;
  size_t hdesc_off = 0, hstrip_off = 0, htile_off = 0;
  size_t ai_off = 0, af_off = 0, ad_off = 0, mono_wts = 0;
  Launch L0, L1a, L2a, L2b, Q0, Q1a, Q2a, Q2b, CL[6];
  Launch RL;  // the rotation stage (placed only when the batch has a sheared image)
  bool h_tiled = false;
  ScLaunches SX;
};
// now_ms() at the end of each planning stage of a batch (plan_batch, place_batch).
struct PlanTimes {
  double images = 0, sc = 0, workspace = 0, vm = 0, hv = 0, blob = 0;
};


// ---- functions that cross the runtime's files ----
// fi_context.cpp
int set_err(int code, const char *fmt, ...);  // sets fi_last_error's thread-local message; returns code
void sync_streams(fi_ctx *c);
int order_after_apply(fi_ctx *c);
int ensure(fi_ctx *c, DevBuf *b, size_t bytes);
int ensure_pinned_buf(void **p, size_t *cap_io, size_t bytes);
int ensure_pinned(fi_ctx *c, size_t bytes);
hipEvent_t get_event(fi_ctx *c);
void collect_ranges(fi_ctx *c, std::vector<TimedRange> &ranges);
void collect_timers(fi_ctx *c);
double now_ms();
void host_stat(fi_ctx *c, const char *name, double ms);
void heap_reset(fi_ctx *c);
int heap_prepare(fi_ctx *c, Exec &E);
bool heap_fits(const fi_ctx *c, const Exec &E);
int heap_commit(fi_ctx *c, Exec &E, const uint8_t *ab, size_t ai_off, size_t af_off, size_t ad_off);
// fi_sc_plan.cpp
ScParamsDev to_dev(const fi_smartcrop_params &p);
void plan_smartcrop(fi_ctx *c, Exec &E, const std::vector<ScItem> &items, ScLaunchData *L, std::vector<int> *status,
                    std::vector<std::string> *errs, bool want_pre);
void add_sc_launches(fi_ctx *c, Blob &B, const ScLaunchData &SL, const std::vector<int> &sstatus, ScLaunches *X);
int enqueue_sc(fi_ctx *c, hipStream_t st, uint8_t *ab, const ScLaunches &X, const int32_t *ai, const double *ad,
               CropScore *scores, ScResult *results, const ScParamsDev &PD);
// fi_rs_plan.cpp
void plan_batch(fi_ctx *c, Exec &E, BatchPlan &Bp, fi_image *imgs, int n, PlanTimes &T);
void place_batch(fi_ctx *c, Exec &E, BatchPlan &Bp, Packed &K, uint8_t *wb, PlanTimes &T);
// fi_tiles.cpp
void build_vm_tiles(fi_ctx *c, Exec &E, BatchPlan &Bp);
void build_hv_tiles(fi_ctx *c, Exec &E, BatchPlan &Bp);
// fi_batch.cpp
int drain(fi_ctx *c);
}  // namespace fi
#endif  // FI_RUNTIME_H
