// fi_rccl.cpp -- the multi-GPU record gather of the runtime (fi_runtime.h) over RCCL.
#include "fi_runtime.h"

using namespace fi;

extern "C" {

int fi_rccl_get_unique_id(uint8_t id[128]) {
  ncclUniqueId u;
  const ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) return set_err(FI_EDEVICE, "ncclGetUniqueId: %s", ncclGetErrorString(r));
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  memcpy(id, &u, 128);
  return FI_OK;
}
int fi_rccl_init(fi_ctx *c, int32_t rank, int32_t world, const uint8_t id[128]) {
  if (!c || rank < 0 || world < 1 || rank >= world) return set_err(FI_EINVAL, "bad rank/world");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  ncclUniqueId u;
  memcpy(&u, id, 128);
  const ncclResult_t r = ncclCommInitRank(&c->comm, world, u, rank);
  if (r != ncclSuccess) return set_err(FI_EDEVICE, "ncclCommInitRank: %s", ncclGetErrorString(r));
  c->rank = rank;
  c->world = world;
  return FI_OK;
}
// The record gather runs on gx_stream, a stream of its own: the records are on
// the host once fi_wait has filled them, so nothing orders the gather after
// the batch streams, and a gather started while the next batch runs returns
// at once (fi_rccl_gather_start); fi_rccl_gather_finish waits for it.  Send
// and receive go through the context's pinned staging, so the caller's
// buffers are plain host memory.
static int gather_finish(fi_ctx *c) {
  if (!c->gx_pending) return FI_OK;
  c->gx_pending = false;
  HIP_TRY(hipEventSynchronize(c->gx_done));
  if (c->gx_recv && c->gx_recv_bytes)
    memcpy(c->gx_recv, (const uint8_t *)c->gx_pin + c->gx_pin_cap / 2, c->gx_recv_bytes);
  c->gx_recv = nullptr;
  c->gx_recv_bytes = 0;
  return FI_OK;
}
static int gather_start(fi_ctx *c, const fi_record *send, int32_t count, fi_record *recv) {
  int rc = gather_finish(c);  // one gather in flight: its staging is reused
  if (rc) return rc;
  const size_t bytes = sizeof(fi_record) * (size_t)count;
  const size_t rbytes = c->rank == 0 ? bytes * (size_t)c->world : 0;
  const size_t total = bytes * (1 + (c->rank == 0 ? c->world : 0));
  if (c->gather.cap < total + 256) {  // its own buffer: batches never read it (no stream drain to grow it)
    if (c->gx_stream) HIP_TRY(hipStreamSynchronize(c->gx_stream));
    if (c->gather.p) HIP_TRY(hipFree(c->gather.p));
    c->gather.p = nullptr;
    c->gather.cap = 0;
    const size_t cap = std::max(total + total / 4 + 256, (size_t)1 << 16);
    if (hipMalloc(&c->gather.p, cap) != hipSuccess) {
      c->gather.p = nullptr;
      return set_err(FI_ENOMEM, "hipMalloc(%zu) for the record gather failed", cap);
    }
    c->gather.cap = cap;
  }
  // pinned staging: send in the first half, receive in the second
  const size_t half = std::max(bytes, rbytes);
  if (c->gx_pin_cap < 2 * half + 64) {
    if (c->gx_pin) HIP_TRY(hipHostFree(c->gx_pin));
    c->gx_pin = nullptr;
    c->gx_pin_cap = 0;
    const size_t cap = 2 * std::max(half + half / 4, (size_t)4096);
    if (hipHostMalloc(&c->gx_pin, cap, hipHostMallocDefault) != hipSuccess) {
      c->gx_pin = nullptr;
      return set_err(FI_ENOMEM, "hipHostMalloc(%zu) for the record gather failed", cap);
    }
    c->gx_pin_cap = cap;
  }
  if (!c->gx_done) HIP_TRY(hipEventCreateWithFlags(&c->gx_done, hipEventDisableTiming));
  uint8_t *pin_s = (uint8_t *)c->gx_pin, *pin_r = pin_s + c->gx_pin_cap / 2;
  hipStream_t st = c->gx_stream;
  uint8_t *sb = (uint8_t *)c->gather.p, *rb = sb + bytes;  // device: send, then world x count receive
  if (c->rank == 0) {
    if (bytes) memcpy(pin_r, send, bytes);  // rank 0's own records: no device round trip
  } else if (bytes) {
    memcpy(pin_s, send, bytes);
    HIP_TRY(hipMemcpyAsync(sb, pin_s, bytes, hipMemcpyHostToDevice, st));
  }
  // nothing between ncclGroupStart and ncclGroupEnd may return early: the
  // group is always closed, then the first error is reported
  ncclResult_t r = ncclGroupStart();
  if (r != ncclSuccess) return set_err(FI_EDEVICE, "ncclGroupStart: %s", ncclGetErrorString(r));
  if (c->rank == 0) {
    for (int p = 1; p < c->world && r == ncclSuccess; p++)
      r = ncclRecv(rb + bytes * p, bytes, ncclUint8, p, c->comm, st);
  } else {
    r = ncclSend(sb, bytes, ncclUint8, 0, c->comm, st);
  }
  const ncclResult_t re = ncclGroupEnd();
  if (r != ncclSuccess || re != ncclSuccess)
    return set_err(FI_EDEVICE, "RCCL gather: %s", ncclGetErrorString(r != ncclSuccess ? r : re));
  if (c->rank == 0 && recv && rbytes > bytes)
    HIP_TRY(hipMemcpyAsync(pin_r + bytes, rb + bytes, rbytes - bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(c->gx_done, st));
  c->gx_pending = true;
  c->gx_recv = c->rank == 0 ? recv : nullptr;
  c->gx_recv_bytes = c->rank == 0 && recv ? rbytes : 0;
  return FI_OK;
}
int fi_rccl_gather_start(fi_ctx *c, const fi_record *send, int32_t count, fi_record *recv) {
  if (!c || !c->comm || count < 0 || (count > 0 && !send)) return set_err(FI_EINVAL, "RCCL not initialised");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return gather_start(c, send, count, recv);
}
int fi_rccl_gather_finish(fi_ctx *c) {
  if (!c) return set_err(FI_EINVAL, "ctx is NULL");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return gather_finish(c);
}
int fi_rccl_gather_records(fi_ctx *c, const fi_record *send, int32_t count, fi_record *recv) {
  if (!c || !c->comm || count < 0 || (count > 0 && !send)) return set_err(FI_EINVAL, "RCCL not initialised");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const int rc = gather_start(c, send, count, recv);
  return rc ? rc : gather_finish(c);
}

}  // extern "C"
