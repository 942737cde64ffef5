// libe2etts_resample.so: a batched, streaming, rational-ratio polyphase FIR resampler behind the C ABI of include/e2etts_resample.h.
// A companion of libe2etts_hip.so; it is linked with its kernel objects as every companion is, and uses none of them.
//
// One kernel.  A workgroup produces a tile of S * L * nrep consecutive outputs of one row (plan.h: choose_tile): it stages the tile's
// input window, S * nrep * M + P samples, into LDS once as fp32 (int16 / 32768 at staging; samples outside the row as zeros), then every
// thread runs the P-term FMA chain of its outputs, k ascending.  The S lanes of a group compute outputs L apart: they share the row
// G[r] of the coefficient table (one address per group: a broadcast in the vector memory pipe, served from L1 / L2) and read the window
// M samples apart, at an odd LDS stride for every M (plan.h: pad_index), so a group's 32-lane halves are free of bank conflicts.
// One-shot calls and stream pushes are the same launch: a push computes outputs [E, E') from the history buffer [k_off, N).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../../include/e2etts_resample.h"
#ifdef E2ERS_TEST_HOOKS
#define E2E_COMPANION_TEST_HOOKS
#endif
#include "../companion/handle.h"
#include "plan.h"

#ifndef E2ERS_SRC_HASH
#define E2ERS_SRC_HASH "unknown"
#endif

using namespace e2etts;
using namespace e2etts::companion;
namespace pl = e2ers_plan;

static_assert(E2ERS_OK == E_OK && E2ERS_EINVAL == E_INVAL && E2ERS_EHIP == E_HIP && E2ERS_ESTATE == E_STATE && E2ERS_ENOMEM == E_NOMEM,
              "include/e2etts_resample.h and csrc/companion/handle.h disagree on the error codes");
static_assert(E2ERS_MAX_B == pl::MAX_B && E2ERS_MAX_RATIO == pl::MAX_RATIO && E2ERS_MAX_PHASE_TAPS == pl::MAX_PHASE_TAPS,
              "include/e2etts_resample.h and csrc/resample/plan.h disagree on the limits");

namespace {

struct KernelArgs {
  const void* x;             // row b at x + b * x_stride elements; element 0 of a row is sample k_off of the signal
  long long x_stride, k_off;
  const int64_t* lens;       // [B][2] = (n_valid, n_out) per row, or NULL: every row has (n_valid_all, n_out_all)
  long long n_valid_all, n_out_all;
  const float* G;            // [L][P]
  pl::Filter f;
  float* wav;                // row b at + b * out_stride; element 0 of a row is output m_off
  int16_t* pcm;
  long long out_stride, m_off, width;   // outputs [m_off, m_off + width) of every row are written
  int S, nrep, shift, window;
};

__device__ __forceinline__ int16_t to_pcm(float y) {   // trunc(y * 32768) saturated (e2etts_denoise's rule)
  const float s = truncf(y * 32768.0f);
  return (int16_t)(int)fminf(fmaxf(s, -32768.0f), 32767.0f);
}

template <typename TIn>
__global__ void __launch_bounds__(pl::THREADS) resample_kernel(const KernelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_win[];   // the window, sample t at pad_index(t)
  const int tid = threadIdx.x;
  const long long b = blockIdx.y;
  const long long tile = (long long)a.S * a.f.L * a.nrep;
  const long long j0 = (long long)blockIdx.x * tile;               // offset of the tile inside the launch
  const long long m0 = a.m_off + j0;
  const long long in_tile = min(tile, a.width - j0);               // outputs of this tile that the launch writes
  const long long nv = a.lens ? a.lens[2 * b] : a.n_valid_all;
  const long long n_out = a.lens ? a.lens[2 * b + 1] : a.n_out_all;
  float* wrow = a.wav + b * a.out_stride + j0;
  int16_t* prow = a.pcm + b * a.out_stride + j0;
  if (m0 >= n_out) {   // uniform over the workgroup: the whole tile lies past the row's outputs
    for (long long j = tid; j < in_tile; j += pl::THREADS) {
      wrow[j] = 0.f;
      prow[j] = 0;
    }
    return;
  }
  const long long kb = pl::window_start(m0, a.f);
  const TIn* row = (const TIn*)a.x + b * a.x_stride;
  for (int t = tid; t < a.window; t += pl::THREADS) {
    const long long k = kb + t;
    float v = 0.f;
    // k < k_off happens only below k_lo(m0), where every tap of the table is a zero: the stream's history starts at k_lo of its first output
    if (k >= 0 && k >= a.k_off && k < nv) {
      if (sizeof(TIn) == 2) v = (float)row[k - a.k_off] * (1.0f / 32768.0f);   // exact: a power of two
      else v = (float)row[k - a.k_off];
    }
    rs_win[pl::pad_index(t, a.shift)] = v;
  }
  __syncthreads();
  const int P = a.f.P;
  for (long long o = tid; o < tile; o += pl::THREADS) {
    const long long j = pl::tile_offset(o, a.S, a.f.L);
    if (j >= in_tile) continue;
    const long long m = m0 + j;
    float y = 0.f;
    if (m < n_out) {
      const long long c = pl::centre(m, a.f);
      const float* g = a.G + (c % a.f.L) * P;
      const int top = (int)(c / a.f.L - kb);   // window index of x[k_hi(m)]; P - 1 <= top < window
      for (int i = P - 1; i >= 0; --i) y = fmaf(rs_win[pl::pad_index(top - i, a.shift)], g[i], y);   // k = k_hi - i ascending
    }
    wrow[j] = y;
    prow[j] = to_pcm(y);
  }
}

thread_local std::string g_create_error;

}  // namespace

struct e2ers_handle : Handle {
  bool loaded = false;
  pl::Filter f;
  pl::Tile tile;
  Buf G{this, Buf::WEIGHTS};
  Buf in{this}, lens{this}, wav{this}, pcm{this};   // one-shot: staged host input, (n_valid, n_out) per row, the resident outputs
  Buf hist[2] = {Buf{this}, Buf{this}};              // stream: the input history, ping-pong
  Buf swav[2] = {Buf{this}, Buf{this}}, spcm[2] = {Buf{this}, Buf{this}};   // stream: the outputs of up to two unfetched pushes
  std::vector<int64_t> host_lens;                    // outlives the asynchronous copy of a call
  long long rB = 0, rW = 0;                          // batch and width of the resident outputs (0: nothing resident)
  // the stream
  bool s_open = false, s_closed = false;
  int sB = 0, s_dtype = 0, cur = 0;
  long long N = 0, E = 0;                            // samples pushed, outputs enqueued
  long long kbuf = 0, hcap[2] = {0, 0};              // hist[cur] row = samples [kbuf, N), rows hcap[cur] elements apart
  long long slot_cnt[2] = {0, 0};
  int head = 0, pending = 0;                         // slots head, head ^ 1 hold the unfetched pushes, oldest first (their kernels' ends: ev[4 + slot])
  hipStream_t copy_stream = nullptr;                 // e2ers_stream_fetch copies on it while a later push computes
};

namespace {

size_t elem_size(int dtype) { return dtype == E2ERS_I16 ? 2 : 4; }

// `rows` rows of `width` bytes, between host and / or device memory
int copy_rows(e2ers_handle* h, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipStream_t s = nullptr) {
  if (!s) s = h->stream;
  if (!width || !rows) return E2ERS_OK;
  if (rows == 1 || (dpitch == width && spitch == width)) HIPCHK(h, hipMemcpyAsync(dst, src, width * rows, hipMemcpyDefault, s));
  else HIPCHK(h, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDefault, s));
  return E2ERS_OK;
}

int launch(e2ers_handle* h, const KernelArgs& a, int B, int dtype) {
  const long long tiles = pl::ceil_div(a.width, h->tile.outputs);
  if (tiles < 1 || tiles > (1LL << 23)) return h->fail(E2ERS_EHIP, "launch refused: the tile count does not fit a grid");
  const dim3 grid((unsigned)tiles, (unsigned)B);
  const size_t lds = (size_t)h->tile.lds_floats * 4;
  if (dtype == E2ERS_I16) hipLaunchKernelGGL(resample_kernel<int16_t>, grid, dim3(pl::THREADS), lds, h->stream, a);
  else hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(pl::THREADS), lds, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return E2ERS_OK;
}

KernelArgs base_args(const e2ers_handle* h) {
  KernelArgs a = {};
  a.G = (const float*)h->G.p;
  a.f = h->f;
  a.S = h->tile.S;
  a.nrep = h->tile.nrep;
  a.shift = h->tile.shift;
  a.window = h->tile.window;
  return a;
}

int stage_table(e2ers_handle* h, Buf& nb, const std::vector<float>& G) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  RET(reserve(h, nb, G.size() * 4));
  HIPCHK(h, hipMemcpyAsync(nb.p, G.data(), G.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return E2ERS_OK;
}

void close_stream(e2ers_handle* h) {
  h->s_open = h->s_closed = false;
  h->pending = 0;
  h->slot_cnt[0] = h->slot_cnt[1] = 0;
}

// the enqueueing half of e2ers_stream_push (validated: N2 samples in total afterwards, outputs [E, E2) to make)
int push_enqueue(e2ers_handle* h, const void* chunk, long long chunk_stride, long long n, long long N2, long long E2) {
  const pl::Filter f = h->f;
  const int B = h->sB;
  const size_t esz = elem_size(h->s_dtype);
  const long long cnt = E2 - h->E;
  RET(open_device(h));
  h->unfinished = true;
  hipStream_t s = h->stream;
  // the new history: what the outputs from E on still read of the old one, then the chunk
  const long long keep_from = std::max<long long>(h->kbuf, pl::history_keep(h->E, h->N, f));
  const long long tail = h->N - keep_from;
  const int nx = h->cur ^ 1;
  const long long need = tail + n;
  if (need > h->hcap[nx]) {
    const long long cap = std::max(need, 2 * h->hcap[nx]);
    RET(reserve(h, h->hist[nx], (size_t)B * cap * esz));
    h->hcap[nx] = cap;
  }
  if (need > 0) {
    char* dst = (char*)h->hist[nx].p;
    const size_t dp = (size_t)h->hcap[nx] * esz;
    if (tail > 0)
      RET(copy_rows(h, dst, dp, (const char*)h->hist[h->cur].p + (size_t)(keep_from - h->kbuf) * esz, (size_t)h->hcap[h->cur] * esz, (size_t)tail * esz, B));
    if (n > 0) {
      RET(copy_rows(h, dst + (size_t)tail * esz, dp, chunk, (size_t)chunk_stride * esz, (size_t)n * esz, B));
      if (!is_device_pointer(chunk)) HIPCHK(h, hipStreamSynchronize(s));   // a host chunk has been consumed when the push returns
    }
  }
  h->cur = nx;
  h->kbuf = keep_from;
  h->N = N2;
  if (cnt > 0) {
    const int slot = h->head ^ h->pending;   // pending 0: head; pending 1: the other
    RET(reserve(h, h->swav[slot], (size_t)B * cnt * 4));
    RET(reserve(h, h->spcm[slot], (size_t)B * cnt * 2));
    KernelArgs a = base_args(h);
    a.x = h->hist[nx].p;
    a.x_stride = h->hcap[nx];
    a.k_off = keep_from;
    a.n_valid_all = N2;
    a.n_out_all = E2;
    a.wav = (float*)h->swav[slot].p;
    a.pcm = (int16_t*)h->spcm[slot].p;
    a.out_stride = a.width = cnt;
    a.m_off = h->E;
    RET(launch(h, a, B, h->s_dtype));
    HIPCHK(h, hipEventRecord(h->ev[4 + slot], s));
    h->slot_cnt[slot] = cnt;
    h->pending += 1;
    h->E = E2;
  }
  return E2ERS_OK;
}

}  // namespace

extern "C" {

const char* e2ers_version(void) { return "e2etts-resample 1 E2ERS_SRC_HASH=" E2ERS_SRC_HASH; }
int e2ers_abi_version(void) { return E2ERS_ABI_VERSION; }

const char* e2ers_last_error(const e2ers_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int e2ers_create(int device_id, e2ers_handle** out) {
  if (!out) {
    g_create_error = "e2ers_create: out is NULL";
    return E2ERS_EINVAL;
  }
  *out = nullptr;
  if (device_id < 0) {
    g_create_error = "e2ers_create: device_id must not be negative";
    return E2ERS_EINVAL;
  }
  e2ers_handle* h = new (std::nothrow) e2ers_handle();
  if (!h) {
    g_create_error = "out of host memory";
    return E2ERS_ENOMEM;
  }
  h->device = device_id;
  *out = h;
  return E2ERS_OK;
}

void e2ers_destroy(e2ers_handle* h) {
  if (h && h->copy_stream && hipSetDevice(h->device) == hipSuccess) {
    (void)hipStreamSynchronize(h->copy_stream);
    (void)hipStreamDestroy(h->copy_stream);
  }
  companion::destroy(h);
}

int e2ers_load(e2ers_handle* h, const float* taps, int n_taps, int L, int M) {
  if (!h) return E2ERS_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!taps) return h->fail(E2ERS_EINVAL, "taps must not be NULL");
  if (const char* m = pl::filter_check(n_taps, L, M))
    return h->fail(E2ERS_EINVAL, std::string(m) + " (n_taps " + std::to_string(n_taps) + ", L " + std::to_string(L) + ", M " + std::to_string(M) + ")");
  std::vector<float> ht;
  RET(fetch_host(h, taps, (size_t)n_taps, ht));
  for (int j = 0; j < n_taps; ++j)
    if (!std::isfinite(ht[j])) return h->fail(E2ERS_EINVAL, "taps[" + std::to_string(j) + "] is not finite");
  const pl::Filter f = pl::make_filter(n_taps, L, M);
  std::vector<float> G((size_t)pl::table_floats(f));
  pl::build_table(ht.data(), f, G.data());
  RET(open_device(h));
  Buf nb;   // free-standing until it replaces the member
  const int rc = stage_table(h, nb, G);
  if (rc != E2ERS_OK) {
    release(h, nb);
    return rc;
  }
  release(h, h->G);   // the stream is drained: nothing reads the old table
  h->G.p = nb.p;
  h->G.bytes = nb.bytes;
  h->f = f;
  h->tile = pl::choose_tile(f);
  h->loaded = true;
  h->unfinished = false;
  h->rB = 0;
  close_stream(h);
  return E2ERS_OK;
}

void* e2ers_stream(e2ers_handle* h) { return companion::stream(h); }
int e2ers_order_after(e2ers_handle* h, void* caller_stream) { return companion::order_after(h, caller_stream); }
int e2ers_sync(e2ers_handle* h) { return companion::sync(h); }
size_t e2ers_device_bytes(const e2ers_handle* h) { return companion::device_bytes(h); }

int e2ers_forward(e2ers_handle* h, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n, float* wav_out,
                  int16_t* pcm_out, long long out_stride, int64_t* n_out_lens, long long* n_out_max) {
  if (!h) return E2ERS_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  // ---- validation: nothing is enqueued before the last check
  if (!audio) return h->fail(E2ERS_EINVAL, "audio must not be NULL");
  if (const char* m = pl::forward_check(dtype, audio_stride, B, n))
    return h->fail(E2ERS_EINVAL, std::string(m) + " (dtype " + std::to_string(dtype) + ", B " + std::to_string(B) + ", n " + std::to_string(n) + ", audio_stride " +
                                     std::to_string(audio_stride) + ")");
  const size_t esz = elem_size(dtype);
  if ((uintptr_t)audio % esz) return h->fail(E2ERS_EINVAL, "audio is not aligned to its element size");
  std::vector<int64_t> nv((size_t)B, (int64_t)n);
  if (n_valid) RET(fetch_host(h, n_valid, (size_t)B, nv));
  for (int b = 0; b < B; ++b)
    if (nv[b] < 0 || nv[b] > n)
      return h->fail(E2ERS_EINVAL, "n_valid[" + std::to_string(b) + "] = " + std::to_string((long long)nv[b]) + ": need 0 <= n_valid <= n = " + std::to_string(n));
  if (!h->loaded) return h->fail(E2ERS_ESTATE, "e2ers_forward before e2ers_load");
  const pl::Filter f = h->f;
  const long long W = pl::n_out(n, f.L, f.M);
  if ((wav_out || pcm_out) && out_stride < W)
    return h->fail(E2ERS_EINVAL, "out_stride must be at least ceil(n * L / M) = " + std::to_string(W) + " (got " + std::to_string(out_stride) + ")");
  // ---- enqueue
  RET(begin_call(h));
  h->rB = 0;
  std::vector<int64_t>& hl = h->host_lens;   // [B][2] (n_valid, n_out) | [B] n_out
  hl.resize((size_t)3 * B);
  for (int b = 0; b < B; ++b) {
    hl[2 * b] = nv[b];
    hl[2 * b + 1] = hl[(size_t)2 * B + b] = pl::n_out(nv[b], f.L, f.M);
  }
  RET(reserve(h, h->lens, (size_t)2 * B * 8));
  RET(reserve(h, h->wav, (size_t)B * W * 4));
  RET(reserve(h, h->pcm, (size_t)B * W * 2));
  hipStream_t s = h->stream;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[0], s));
  HIPCHK(h, hipMemcpyAsync(h->lens.p, hl.data(), (size_t)2 * B * 8, hipMemcpyHostToDevice, s));
  KernelArgs a = base_args(h);
  a.x = audio;
  a.x_stride = audio_stride;
  if (!is_device_pointer(audio)) {   // host samples: only the n samples of each row travel
    RET(reserve(h, h->in, (size_t)B * n * esz));
    RET(copy_rows(h, h->in.p, (size_t)n * esz, audio, (size_t)audio_stride * esz, (size_t)n * esz, B));
    a.x = h->in.p;
    a.x_stride = n;
  }
  a.lens = (const int64_t*)h->lens.p;
  a.wav = (float*)h->wav.p;
  a.pcm = (int16_t*)h->pcm.p;
  a.out_stride = a.width = W;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[1], s));
  RET(launch(h, a, B, dtype));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[2], s));
  if (wav_out) RET(copy_rows(h, wav_out, (size_t)out_stride * 4, h->wav.p, (size_t)W * 4, (size_t)W * 4, B));
  if (pcm_out) RET(copy_rows(h, pcm_out, (size_t)out_stride * 2, h->pcm.p, (size_t)W * 2, (size_t)W * 2, B));
  if (n_out_lens) {
    if (is_device_pointer(n_out_lens)) HIPCHK(h, hipMemcpyAsync(n_out_lens, hl.data() + (size_t)2 * B, (size_t)B * 8, hipMemcpyHostToDevice, s));
    else memcpy(n_out_lens, hl.data() + (size_t)2 * B, (size_t)B * 8);
  }
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[3], s));
  const Phase phases[3] = {{0, 1}, {1, 2}, {2, 3}};   // upload, filter, fetch
  RET(finish(h, phases));
  h->rB = B;
  h->rW = W;
  if (n_out_max) *n_out_max = W;
  return E2ERS_OK;
}

const float* e2ers_wav_dev(e2ers_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB ? (const float*)h->wav.p : nullptr;
}

const int16_t* e2ers_pcm_dev(e2ers_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB ? (const int16_t*)h->pcm.p : nullptr;
}

int e2ers_stream_begin(e2ers_handle* h, int B, int dtype) {
  if (!h) return E2ERS_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (dtype != E2ERS_F32 && dtype != E2ERS_I16) return h->fail(E2ERS_EINVAL, "dtype must be E2ERS_F32 or E2ERS_I16 (got " + std::to_string(dtype) + ")");
  if (B < 1 || B > E2ERS_MAX_B) return h->fail(E2ERS_EINVAL, "B must lie in [1, " + std::to_string(E2ERS_MAX_B) + "] (got " + std::to_string(B) + ")");
  if (!h->loaded) return h->fail(E2ERS_ESTATE, "e2ers_stream_begin before e2ers_load");
  if (h->unfinished) {   // an abandoned stream's pushes may still run
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->unfinished = false;
  }
  close_stream(h);
  h->s_open = true;
  h->sB = B;
  h->s_dtype = dtype;
  h->N = h->E = h->kbuf = 0;
  h->cur = h->head = 0;
  return E2ERS_OK;
}

int e2ers_stream_push(e2ers_handle* h, const void* chunk, long long chunk_stride, long long n, int last, long long* n_ready) {
  if (!h) return E2ERS_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  // ---- validation
  if (n < 0 || n > pl::MAX_N - h->N) return h->fail(E2ERS_EINVAL, "n must not be negative, and a stream holds at most 2^40 samples (got n " + std::to_string(n) + ")");
  const size_t esz = elem_size(h->s_dtype);
  if (n > 0) {
    if (!chunk) return h->fail(E2ERS_EINVAL, "chunk must not be NULL when n > 0");
    if (chunk_stride < n) return h->fail(E2ERS_EINVAL, "chunk_stride must be at least n (got " + std::to_string(chunk_stride) + " < " + std::to_string(n) + ")");
    if ((uintptr_t)chunk % esz) return h->fail(E2ERS_EINVAL, "chunk is not aligned to its element size");
  }
  if (!h->s_open) return h->fail(E2ERS_ESTATE, "e2ers_stream_push without an open stream (e2ers_stream_begin)");
  if (h->s_closed) return h->fail(E2ERS_ESTATE, "e2ers_stream_push after the last chunk");
  const pl::Filter f = h->f;
  const long long N2 = h->N + n, E2 = pl::emitted(N2, last, f), cnt = E2 - h->E;
  if (cnt > 0 && h->pending == 2) return h->fail(E2ERS_ESTATE, "two pushes are unfetched: e2ers_stream_fetch first");
  // ---- enqueue (no drain: the next push follows on the same stream, the fetch waits for its own push only)
  const int rc = push_enqueue(h, chunk, chunk_stride, n, N2, E2);
  if (rc != E2ERS_OK) {   // a failure after validation: the stream's state is gone
    close_stream(h);
    return rc;
  }
  if (last) h->s_closed = true;
  if (n_ready) *n_ready = cnt;
  return E2ERS_OK;
}

int e2ers_stream_fetch(e2ers_handle* h, float* wav_out, int16_t* pcm_out, long long out_stride, size_t capacity) {
  if (!h) return E2ERS_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->s_open || h->pending == 0) return h->fail(E2ERS_ESTATE, "e2ers_stream_fetch: no unfetched push");
  const int slot = h->head, B = h->sB;
  const long long cnt = h->slot_cnt[slot];
  if (out_stride < cnt || capacity < (size_t)(B - 1) * (size_t)out_stride + (size_t)cnt)
    return h->fail(E2ERS_EINVAL, "the oldest unfetched push holds " + std::to_string(cnt) + " samples per row: need out_stride >= that and capacity >= (B - 1) * out_stride + that");
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->copy_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  hipStream_t cs = h->copy_stream;
  HIPCHK(h, hipStreamWaitEvent(cs, h->ev[4 + slot], 0));   // the end of that push's kernel; a later push goes on computing
  if (wav_out) RET(copy_rows(h, wav_out, (size_t)out_stride * 4, h->swav[slot].p, (size_t)cnt * 4, (size_t)cnt * 4, B, cs));
  if (pcm_out) RET(copy_rows(h, pcm_out, (size_t)out_stride * 2, h->spcm[slot].p, (size_t)cnt * 2, (size_t)cnt * 2, B, cs));
  HIPCHK(h, hipStreamSynchronize(cs));
  h->slot_cnt[slot] = 0;
  h->head ^= 1;
  h->pending -= 1;
  return E2ERS_OK;
}

long long e2ers_tile_outputs(const e2ers_handle* h) { return h && h->loaded ? (long long)h->tile.outputs : 0; }

int e2ers_profile_enable(e2ers_handle* h, int on) { return companion::profile_enable(h, on); }
int e2ers_profile_read(e2ers_handle* h, double ms_out[3]) { return companion::profile_read(h, ms_out); }

#ifdef E2ERS_TEST_HOOKS
int e2ers_debug_poison_workspace(e2ers_handle* h) {
  if (!h) return E2ERS_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(poison_workspaces(h));
  h->unfinished = false;
  h->rB = 0;
  close_stream(h);
  return E2ERS_OK;
}
#endif

}  // extern "C"
