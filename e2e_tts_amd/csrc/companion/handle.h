// What every companion library of libe2etts_hip.so (csrc/align, csrc/mel) keeps behind its handle: the device, one stream, the profiling
// events, the error text, the device buffers and the protocol of a computing call (validate, begin_call, enqueue, finish).  Header-only
// and in a directory of its own: the main library's source hash does not see it, every companion's does.
//
// A companion's handle derives from Handle and declares its buffers as members `Buf x{this}` (workspace) or `Buf w{this, Buf::WEIGHTS}`:
// that declaration is the one place a buffer is named.  Teardown frees all of them, the test hook poisons the workspaces.  Its
// extern "C" entry points take the handle's mutex; the functions below that say so take it themselves, all others expect it held.
// Before including this header a test build defines E2E_COMPANION_TEST_HOOKS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

namespace e2etts {
namespace companion {

// the error codes of every companion's public header (each library static_asserts that its own are these)
constexpr int E_OK = 0, E_INVAL = -1, E_HIP = -2, E_STATE = -3, E_NOMEM = -4;

struct Handle;

struct Buf {
  enum Kind { WORKSPACE, WEIGHTS };
  void* p = nullptr;
  size_t bytes = 0;
  Buf() = default;   // a free-standing buffer (staging): whoever declares it releases it or moves it into a member
  inline explicit Buf(Handle* owner, Kind kind = WORKSPACE);   // a member of `owner`
};

struct Handle {
  int device = 0;
  std::mutex mu;
  std::string err;
  bool open = false;
  hipStream_t stream = nullptr;
  hipEvent_t ev[6] = {};
  hipEvent_t order_ev = nullptr;
  bool profile = false;
  double last_ms[3] = {0, 0, 0};
  size_t dev_bytes = 0;
  bool unfinished = false;               // a call returned on an error before its stream was drained
  std::vector<Buf*> bufs, workspaces;   // every member buffer; those of them a call may overwrite

  int fail(int code, const std::string& msg) {
    err = msg;
    return code;
  }
};

Buf::Buf(Handle* owner, Kind kind) {
  owner->bufs.push_back(this);
  if (kind == WORKSPACE) owner->workspaces.push_back(this);
}

#define HIPCHK(h, call)                                                                                                   \
  do {                                                                                                                    \
    hipError_t e_ = (call);                                                                                               \
    if (e_ != hipSuccess) return (h)->fail(::e2etts::companion::E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define KCHK(h, call)                                                                              \
  do {                                                                                             \
    const char* m_ = (call);                                                                       \
    if (m_) return (h)->fail(::e2etts::companion::E_HIP, std::string("launch refused: ") + m_); \
  } while (0)
#define RET(call)                                         \
  do {                                                    \
    int rc_ = (call);                                     \
    if (rc_ != ::e2etts::companion::E_OK) return rc_; \
  } while (0)

inline bool is_device_pointer(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice;
}

inline int open_device(Handle* h) {
  HIPCHK(h, hipSetDevice(h->device));
  if (h->open) return E_OK;
  HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  for (auto& e : h->ev) HIPCHK(h, hipEventCreate(&e));
  HIPCHK(h, hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming));
  h->open = true;
  return E_OK;
}

inline int reserve(Handle* h, Buf& b, size_t bytes) {
  bytes = (bytes + 255) / 256 * 256;
  if (b.bytes >= bytes) return E_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b.p) {
    HIPCHK(h, hipFree(b.p));
    h->dev_bytes -= b.bytes;
    b.p = nullptr;
    b.bytes = 0;
  }
  if (hipMalloc(&b.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    return h->fail(E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
  }
  b.bytes = bytes;
  h->dev_bytes += bytes;
  return E_OK;
}

// frees a buffer (the stream must be drained)
inline void release(Handle* h, Buf& b) {
  if (!b.p) return;
  (void)hipFree(b.p);
  h->dev_bytes -= b.bytes;
  b.p = nullptr;
  b.bytes = 0;
}

// host copy of `count` elements behind a host or device pointer
template <typename T>
int fetch_host(Handle* h, const T* p, size_t count, std::vector<T>& out) {
  out.resize(count);
  if (is_device_pointer(p)) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(out.data(), p, count * sizeof(T), hipMemcpyDefault));
  } else {
    memcpy(out.data(), p, count * sizeof(T));
  }
  return E_OK;
}

// after validation, before the first thing a computing call enqueues
inline int begin_call(Handle* h) {
  RET(open_device(h));
  if (h->unfinished) HIPCHK(h, hipStreamSynchronize(h->stream));
  h->unfinished = true;
  return E_OK;
}

inline int copy_out(Handle* h, void* dst, const void* src, size_t bytes) {
  if (dst) HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
  return E_OK;
}

// the events around one profiled phase of a call; from < 0: the call did not run that phase (its time reads 0)
struct Phase {
  int from, to;
};

// the end of a computing call: drains the stream and, when profiling, reads the three phases' times
inline int finish(Handle* h, const Phase (&phases)[3]) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->unfinished = false;
  if (h->profile) {
    for (int i = 0; i < 3; ++i) {
      float ms = 0.f;
      if (phases[i].from >= 0) HIPCHK(h, hipEventElapsedTime(&ms, h->ev[phases[i].from], h->ev[phases[i].to]));
      h->last_ms[i] = ms;
    }
  }
  return E_OK;
}

// ---- the bodies of the entry points every companion has (NULL handle and mutex included)

inline void* stream(Handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  if (open_device(h) != E_OK) return nullptr;
  return (void*)h->stream;
}

inline int order_after(Handle* h, void* caller_stream) {
  if (!h) return E_INVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(open_device(h));
  HIPCHK(h, hipEventRecord(h->order_ev, (hipStream_t)caller_stream));
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->order_ev, 0));
  return E_OK;
}

inline int sync(Handle* h) {
  if (!h) return E_INVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->open) return E_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return E_OK;
}

inline size_t device_bytes(const Handle* h) { return h ? h->dev_bytes : 0; }

inline int profile_enable(Handle* h, int on) {
  if (!h) return E_INVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  h->profile = on != 0;
  return E_OK;
}

inline int profile_read(Handle* h, double ms_out[3]) {
  if (!h) return E_INVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!ms_out) return h->fail(E_INVAL, "ms_out is NULL");
  for (int i = 0; i < 3; ++i) ms_out[i] = h->last_ms[i];
  return E_OK;
}

// drains the stream, frees every member buffer and the handle
template <typename H>
void destroy(H* h) {
  if (!h) return;
  if (h->open && hipSetDevice(h->device) == hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    for (Buf* b : h->bufs)
      if (b->p) (void)hipFree(b->p);
    for (auto& e : h->ev)
      if (e) (void)hipEventDestroy(e);
    if (h->order_ev) (void)hipEventDestroy(h->order_ev);
    (void)hipStreamDestroy(h->stream);
  }
  delete h;
}

#ifdef E2E_COMPANION_TEST_HOOKS
__global__ void companion_poison_kernel(uint32_t* p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0x7fc00000u | (uint32_t)(i & 0xffff);
}

// NaN patterns over every workspace (the mutex held); the caller forgets what it held resident
inline int poison_workspaces(Handle* h) {
  if (!h->open) return E_OK;
  HIPCHK(h, hipSetDevice(h->device));
  for (Buf* b : h->workspaces) {
    if (!b->p) continue;
    const size_t n = b->bytes / 4;
    hipLaunchKernelGGL(companion_poison_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (uint32_t*)b->p, n);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return E_OK;
}
#endif

}  // namespace companion
}  // namespace e2etts
