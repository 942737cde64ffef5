// libe2etts_condition.so: silence trim and loudness of int16 recordings behind the C ABI of include/e2etts_condition.h.
// A companion of libe2etts_hip.so; it is linked with its kernel objects as every companion is, and uses none of them.
//
// Five passes over a ragged batch, all integer or double arithmetic (no float sums: nothing depends on an order of summation):
//   bins     sum of squares per millisecond bin [pos(p), pos(p + 1)): a workgroup owns BIN_TILE bins, reads their samples with 16-byte
//            loads where a whole aligned chunk lies inside the row (2-byte loads at the edges), and adds runs into uint64 LDS counters
//            (integer atomics: the result does not depend on their order).  Samples past N are the zero tail: they are skipped.
//   window   a workgroup takes a tile of T starts: the T + W - 1 bins it needs go to LDS, an LDS prefix scan turns them into P, and the
//            window sum of start t is P[t + W] - P[t].  One wavefront ballot per 64 starts is one word of the row's flag bitmap.
//   ranges   one wavefront per row walks the flag words in order and carries (last silent start, ranges so far): a lane finds its silent
//            predecessor from the word's bits below it (or the carry), openers are numbered by popcount of the opener ballot.  Lane 0
//            ends the walk, decides the kept span (plan.h: kept_span) and writes the row's record.
//   span     the kept span's sum of squares = the sum of its bins, wavefront-reduced, one uint64 atomic per workgroup.
//   apply    gather from pos(s), multiply by the row's gain in double, floor and saturate (audioop.mul), 16-byte stores of int16 and fp32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../../include/e2etts_condition.h"
#ifdef E2ECOND_TEST_HOOKS
#define E2E_COMPANION_TEST_HOOKS
#endif
#include "../companion/handle.h"
#include "plan.h"

#ifndef E2ECOND_SRC_HASH
#define E2ECOND_SRC_HASH "unknown"
#endif

using namespace e2etts;
using namespace e2etts::companion;
namespace pl = e2econd_plan;

static_assert(E2ECOND_OK == E_OK && E2ECOND_EINVAL == E_INVAL && E2ECOND_EHIP == E_HIP && E2ECOND_ESTATE == E_STATE && E2ECOND_ENOMEM == E_NOMEM,
              "include/e2etts_condition.h and csrc/companion/handle.h disagree on the error codes");
static_assert(E2ECOND_MAX_B == pl::MAX_B && E2ECOND_MIN_RATE == pl::MIN_RATE && E2ECOND_MAX_RATE == pl::MAX_RATE && E2ECOND_MAX_W == pl::MAX_W,
              "include/e2etts_condition.h and csrc/condition/plan.h disagree on the limits");
static_assert(E2ECOND_TRIM_NONE == pl::TRIM_NONE && E2ECOND_TRIM_REFERENCE == pl::TRIM_REFERENCE && E2ECOND_TRIM_BOTH == pl::TRIM_BOTH,
              "include/e2etts_condition.h and csrc/condition/plan.h disagree on the trim modes");
static_assert(sizeof(e2econd_row) == 32, "e2econd_row is 32 bytes");

namespace {

typedef unsigned long long u64;
constexpr long long MAX_LEN_MS = 1LL << 30;

struct RowIn {
  long long N;   // frames of the row
  int len_ms;
  int nb;        // bins (plan.h: n_bins)
};

__device__ __forceinline__ u64 lanes_below(int lane) { return ((u64)1 << lane) - 1; }

// samples [j0, j0 + 8) of a row, zeros outside [lo, hi); 0 <= lo <= hi <= N.  row + j0 is 16-byte aligned whenever the whole chunk is inside.
__device__ __forceinline__ void load8(const int16_t* row, long long j0, long long lo, long long hi, int v[8], bool aligned = true) {
  if (aligned && j0 >= lo && j0 + 8 <= hi) {
    const int4 q = *reinterpret_cast<const int4*>(row + j0);
    v[0] = (int16_t)(q.x & 0xffff), v[1] = q.x >> 16;
    v[2] = (int16_t)(q.y & 0xffff), v[3] = q.y >> 16;
    v[4] = (int16_t)(q.z & 0xffff), v[5] = q.z >> 16;
    v[6] = (int16_t)(q.w & 0xffff), v[7] = q.w >> 16;
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long j = j0 + u;
      v[u] = (j >= lo && j < hi) ? (int)row[j] : 0;
    }
  }
}

__global__ void __launch_bounds__(pl::THREADS) bins_kernel(const int16_t* x, long long stride, const RowIn* rows, u64* bins, long long bstride, int rate) {
  __shared__ u64 acc[pl::BIN_TILE];
  const int tid = threadIdx.x;
  const long long b = blockIdx.y;
  const RowIn r = rows[b];
  const long long p0 = (long long)blockIdx.x * pl::BIN_TILE;
  if (p0 >= r.nb) return;   // uniform over the workgroup
  const long long p1 = min(p0 + pl::BIN_TILE, (long long)r.nb);
  if (tid < pl::BIN_TILE) acc[tid] = 0;
  __syncthreads();
  const long long lo = min((long long)pl::pos(p0, rate), r.N), hi = min((long long)pl::pos(p1, rate), r.N);
  if (lo < hi) {
    const int16_t* row = x + b * stride;
    const long long mis = (long long)(((uintptr_t)row >> 1) & 7);   // chunk c holds samples [8 c - mis, 8 c - mis + 8): 16-byte aligned
    const long long c0 = (lo + mis) >> 3, c1 = (hi - 1 + mis) >> 3;
    for (long long c = c0 + tid; c <= c1; c += pl::THREADS) {
      const long long j0 = 8 * c - mis;
      int v[8];
      load8(row, j0, lo, hi, v);
      const long long jf = max(j0, lo);
      long long p = pl::bin_of(jf, rate), nxt = pl::pos(p + 1, rate);
      u64 run = 0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const long long j = j0 + u;
        if (j < lo || j >= hi) continue;
        while (j >= nxt) {
          if (run) atomicAdd(&acc[p - p0], run);
          run = 0;
          ++p;
          nxt = pl::pos(p + 1, rate);
        }
        run += (u64)(unsigned)(v[u] * v[u]);
      }
      if (run) atomicAdd(&acc[p - p0], run);
    }
  }
  __syncthreads();
  if (tid < p1 - p0) bins[b * bstride + p0 + tid] = acc[tid];
}

__global__ void __launch_bounds__(pl::THREADS) window_kernel(const u64* bins, long long bstride, const RowIn* rows, u64* flags, long long fstride, int W, int k,
                                                             int rate, int T) {
  extern __shared__ __attribute__((aligned(16))) u64 P[];   // T + W entries
  __shared__ u64 part[2][pl::THREADS];
  const int tid = threadIdx.x;
  const long long b = blockIdx.y;
  const long long starts = pl::n_starts(rows[b].len_ms, W);
  const long long i0 = (long long)blockIdx.x * T;
  if (i0 >= starts) return;   // uniform over the workgroup
  const int cnt = (int)min((long long)T, starts - i0);
  const int need = cnt + W - 1;   // bins i0 .. i0 + need - 1 <= len_ms - 1
  const u64* rb = bins + b * bstride + i0;
  for (int t = tid; t < need; t += pl::THREADS) P[t] = rb[t];
  __syncthreads();
  const int per = (need + pl::THREADS - 1) / pl::THREADS;
  const int a = min(tid * per, need), z = min(a + per, need);
  u64 sum = 0;
  for (int t = a; t < z; ++t) sum += P[t];
  part[0][tid] = sum;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < pl::THREADS; d <<= 1) {
    u64 v = part[cur][tid];
    if (tid >= d) v += part[cur][tid - d];
    part[cur ^ 1][tid] = v;
    __syncthreads();
    cur ^= 1;
  }
  u64 run = part[cur][tid] - sum;   // the sum of the chunks before this thread's
  for (int t = a; t < z; ++t) {
    const u64 v = P[t];
    P[t] = run;
    run += v;
  }
  if (a < z && z == need) P[need] = run;   // the thread that owns the last bin
  __syncthreads();
  const int lane = tid & 63;
  for (int t = tid; t - lane < cnt; t += pl::THREADS) {   // whole wavefronts: t - lane is the wavefront's first start
    const bool silent = t < cnt && pl::window_silent(P[t + W] - P[t], i0 + t, W, k, rate);
    const u64 m = __ballot(silent);
    if (lane == 0) flags[b * fstride + ((i0 + t) >> 6)] = m;
  }
}

__global__ void __launch_bounds__(64) ranges_kernel(const u64* flags, long long fstride, const RowIn* rows, int32_t* ranges, int cap, e2econd_row* recs, int2* spans,
                                                    int W, int rate, int trim) {
  const int lane = threadIdx.x;
  const long long b = blockIdx.x;
  const RowIn r = rows[b];
  const long long starts = pl::n_starts(r.len_ms, W);
  const long long nwords = (starts + 63) >> 6;
  const u64* fw = flags + b * fstride;
  int32_t* rg = ranges + b * (long long)cap * 2;
  long long last = -1, count = 0, first_start = 0, first_end = 0, last_start = 0;   // uniform over the wavefront
  constexpr int AHEAD = 8;   // words per lane and round, loaded back to back: the walk is serial, the loads' latencies overlap
  for (long long w0 = 0; w0 < nwords; w0 += 64 * AHEAD) {
    u64 words[AHEAD];
#pragma unroll
    for (int q = 0; q < AHEAD; ++q) words[q] = w0 + 64 * q + lane < nwords ? fw[w0 + 64 * q + lane] : 0;
#pragma unroll
    for (int q = 0; q < AHEAD; ++q) {
      const u64 word = words[q];
      u64 nz = __ballot(word != 0);
      while (nz) {
        const int wi = __ffsll((long long)nz) - 1;
        nz &= nz - 1;
        const u64 m = __shfl(word, wi);
        const long long base = (w0 + 64 * q + wi) << 6;
        const long long bp = base + lane;
        const u64 below = m & lanes_below(lane);
        const long long prev = below ? base + 63 - __clzll((long long)below) : last;
        const bool op = ((m >> lane) & 1) && pl::opens(bp, prev, W);
        const u64 om = __ballot(op);
        if (om) {
          const int n_op = __popcll(om);
          if (op) {
            const long long rr = count + __popcll(om & lanes_below(lane));
            if (rr < cap) rg[2 * rr] = (int32_t)bp;
            if (rr >= 1 && rr - 1 < cap) rg[2 * (rr - 1) + 1] = (int32_t)(prev + W);
          }
          if (count == 0) first_start = base + __ffsll((long long)om) - 1;
          if (count <= 1 && count + n_op >= 2) {   // the opener of range 1 ends range 0
            const u64 o2 = count == 1 ? om : (om & (om - 1));
            first_end = __shfl(prev, __ffsll((long long)o2) - 1) + W;
          }
          last_start = base + 63 - __clzll((long long)om);
          count += n_op;
        }
        last = base + 63 - __clzll((long long)m);
      }
    }
  }
  if (lane == 0) {
    const long long last_end = last + W;
    if (count >= 1 && count - 1 < cap) rg[2 * (count - 1) + 1] = (int32_t)last_end;
    if (count == 1) first_end = last_end;
    const pl::Span sp = pl::kept_span(count, first_start, first_end, last_start, last_end, trim, r.len_ms, r.N, rate);
    e2econd_row rec;
    rec.len_ms = r.len_ms;
    rec.n_ranges = (int32_t)count;
    rec.s_ms = (int32_t)sp.s_ms;
    rec.e_ms = (int32_t)sp.e_ms;
    rec.n_out = sp.n_out;
    rec.sumsq = 0;   // span_kernel adds to it
    recs[b] = rec;
    spans[b] = make_int2((int)sp.bin_lo, (int)sp.bin_hi);
  }
}

__global__ void __launch_bounds__(pl::THREADS) span_kernel(const u64* bins, long long bstride, const int2* spans, e2econd_row* recs) {
  __shared__ u64 part[pl::THREADS / 64];
  const int tid = threadIdx.x;
  const long long b = blockIdx.y;
  const int2 sp = spans[b];
  const long long lo = sp.x + (long long)blockIdx.x * pl::SPAN_TILE, hi = min(lo + pl::SPAN_TILE, (long long)sp.y);
  if (lo >= hi) return;   // uniform over the workgroup
  u64 sum = 0;
  for (long long t = lo + tid; t < hi; t += pl::THREADS) sum += bins[b * bstride + t];
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d);
  if ((tid & 63) == 0) part[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    u64 total = 0;
    for (int w = 0; w < pl::THREADS / 64; ++w) total += part[w];
    if (total) atomicAdd((u64*)&recs[b].sumsq, total);
  }
}

// 8 outputs per thread; rows `ostride` (a multiple of 8) apart in buffers aligned to 256 bytes: whole 16-byte stores
__global__ void __launch_bounds__(pl::THREADS) apply_kernel(const int16_t* x, long long stride, const RowIn* rows, const e2econd_row* recs, const double* gain,
                                                            int16_t* pcm, float* wav, long long ostride, int rate) {
  const long long b = blockIdx.y;
  const long long j0 = 8 * ((long long)blockIdx.x * pl::THREADS + threadIdx.x);
  if (j0 >= ostride) return;
  const long long N = rows[b].N, n_out = recs[b].n_out, o = pl::pos(recs[b].s_ms, rate);
  const double g = gain[b];
  const int16_t* row = x + b * stride;
  int y[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const long long j = j0 + u;
    int s = 0;
    if (j < n_out && o + j < N) s = (int)floor(fmin(fmax((double)row[o + j] * g, -32768.0), 32767.0));
    y[u] = s;
  }
  if (pcm) {
    int4 q;
    q.x = (int)((unsigned)(y[0] & 0xffff) | ((unsigned)y[1] << 16));
    q.y = (int)((unsigned)(y[2] & 0xffff) | ((unsigned)y[3] << 16));
    q.z = (int)((unsigned)(y[4] & 0xffff) | ((unsigned)y[5] << 16));
    q.w = (int)((unsigned)(y[6] & 0xffff) | ((unsigned)y[7] << 16));
    *reinterpret_cast<int4*>(pcm + b * ostride + j0) = q;
  }
  if (wav) {
    float4* w = reinterpret_cast<float4*>(wav + b * ostride + j0);
    const float sc = 1.0f / 32768.0f;   // exact
    w[0] = make_float4(y[0] * sc, y[1] * sc, y[2] * sc, y[3] * sc);
    w[1] = make_float4(y[4] * sc, y[5] * sc, y[6] * sc, y[7] * sc);
  }
}

// 4 frames per thread: mono = floor((l + r) / 2)
__global__ void __launch_bounds__(pl::THREADS) downmix_kernel(const int16_t* x, long long stride, int16_t* mono, long long n) {
  const long long b = blockIdx.y;
  const long long f0 = 4 * ((long long)blockIdx.x * pl::THREADS + threadIdx.x);
  if (f0 >= n) return;
  const int16_t* row = x + b * stride;
  int v[8];
  load8(row, 2 * f0, 0, 2 * n, v, (((uintptr_t)row) & 15) == 0);   // (a row off the 16-byte grid takes the 2-byte loads throughout)
  int16_t* out = mono + b * n + f0;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (f0 + u < n) out[u] = (int16_t)((v[2 * u] + v[2 * u + 1]) >> 1);
}

thread_local std::string g_create_error;

}  // namespace

struct e2econd_handle : Handle {
  bool configured = false;
  int rate = 0, W = 0, k = 0;
  pl::Tile tile;
  Buf in{this}, mono{this};                                            // staged host input; the resident downmix
  Buf rows{this}, bins{this}, flags{this}, ranges{this}, recs{this}, spans{this}, gain{this};
  Buf pcm{this}, wav{this};                                            // the resident outputs
  std::vector<RowIn> host_rows;                                        // outlive the asynchronous copies of a call
  std::vector<e2econd_row> host_recs;
  std::vector<double> host_gain;
  long long mB = 0, mN = 0;                                            // the resident downmix (0: none)
  bool analyzed = false;                                               // a completed analysis: apply may run
  int aB = 0;
  const int16_t* src = nullptr;                                        // what it read: rows src_stride elements apart
  long long src_stride = 0, width = 0;
  long long rB = 0, rS = 0;                                            // batch and row stride of the resident outputs (0: none)
  int rwant = 0;
};

namespace {

int copy_rows(e2econd_handle* h, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
  if (!width || !rows) return E2ECOND_OK;
  if (rows == 1 || (dpitch == width && spitch == width)) HIPCHK(h, hipMemcpyAsync(dst, src, width * rows, hipMemcpyDefault, h->stream));
  else HIPCHK(h, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDefault, h->stream));
  return E2ECOND_OK;
}

unsigned grid_x(long long items, long long per) { return (unsigned)pl::ceil_div(items, per); }

}  // namespace

extern "C" {

const char* e2econd_version(void) { return "e2etts-condition 1 E2ECOND_SRC_HASH=" E2ECOND_SRC_HASH; }
int e2econd_abi_version(void) { return E2ECOND_ABI_VERSION; }

const char* e2econd_last_error(const e2econd_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int e2econd_create(int device_id, e2econd_handle** out) {
  if (!out) {
    g_create_error = "e2econd_create: out is NULL";
    return E2ECOND_EINVAL;
  }
  *out = nullptr;
  if (device_id < 0) {
    g_create_error = "e2econd_create: device_id must not be negative";
    return E2ECOND_EINVAL;
  }
  e2econd_handle* h = new (std::nothrow) e2econd_handle();
  if (!h) {
    g_create_error = "out of host memory";
    return E2ECOND_ENOMEM;
  }
  h->device = device_id;
  *out = h;
  return E2ECOND_OK;
}

void e2econd_destroy(e2econd_handle* h) { companion::destroy(h); }

int e2econd_configure(e2econd_handle* h, int rate, int min_silence_len, int k) {
  if (!h) return E2ECOND_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (const char* m = pl::config_check(rate, min_silence_len, k))
    return h->fail(E2ECOND_EINVAL, std::string(m) + " (rate " + std::to_string(rate) + ", min_silence_len " + std::to_string(min_silence_len) + ", k " + std::to_string(k) + ")");
  h->rate = rate;
  h->W = min_silence_len;
  h->k = k;
  h->tile = pl::choose_tile(min_silence_len);
  h->configured = true;
  h->analyzed = false;
  h->rB = 0;
  return E2ECOND_OK;
}

void* e2econd_stream(e2econd_handle* h) { return companion::stream(h); }
int e2econd_order_after(e2econd_handle* h, void* caller_stream) { return companion::order_after(h, caller_stream); }
int e2econd_sync(e2econd_handle* h) { return companion::sync(h); }
size_t e2econd_device_bytes(const e2econd_handle* h) { return companion::device_bytes(h); }

int e2econd_downmix(e2econd_handle* h, const int16_t* stereo, long long stride, int B, long long n, int16_t* mono_out, long long out_stride) {
  if (!h) return E2ECOND_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!stereo) return h->fail(E2ECOND_EINVAL, "stereo must not be NULL");
  if (const char* m = pl::batch_check(B, n, stride / 2))
    return h->fail(E2ECOND_EINVAL, std::string(m) + " (B " + std::to_string(B) + ", n " + std::to_string(n) + " frames, stride " + std::to_string(stride) + " elements: need 2 n)");
  if ((uintptr_t)stereo % 2) return h->fail(E2ECOND_EINVAL, "stereo is not aligned to its element size");
  if (mono_out && out_stride < n) return h->fail(E2ECOND_EINVAL, "out_stride must be at least n (got " + std::to_string(out_stride) + ")");
  RET(begin_call(h));
  h->mB = 0;
  h->analyzed = false;   // it may have read the downmix this call replaces
  h->rB = 0;
  RET(reserve(h, h->mono, (size_t)B * n * 2));
  hipStream_t s = h->stream;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[0], s));
  const int16_t* x = stereo;
  long long xs = stride;
  if (!is_device_pointer(stereo)) {
    RET(reserve(h, h->in, (size_t)B * n * 4));
    RET(copy_rows(h, h->in.p, (size_t)n * 4, stereo, (size_t)stride * 2, (size_t)n * 4, B));
    x = (const int16_t*)h->in.p;
    xs = 2 * n;
  }
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[1], s));
  hipLaunchKernelGGL(downmix_kernel, dim3(grid_x(n, 4 * pl::THREADS), (unsigned)B), dim3(pl::THREADS), 0, s, x, xs, (int16_t*)h->mono.p, n);
  HIPCHK(h, hipGetLastError());
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[2], s));
  if (mono_out) RET(copy_rows(h, mono_out, (size_t)out_stride * 2, h->mono.p, (size_t)n * 2, (size_t)n * 2, B));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[3], s));
  const Phase phases[3] = {{0, 1}, {1, 2}, {2, 3}};   // upload, compute, fetch
  RET(finish(h, phases));
  h->mB = B;
  h->mN = n;
  return E2ECOND_OK;
}

const int16_t* e2econd_mono_dev(e2econd_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->mB ? (const int16_t*)h->mono.p : nullptr;
}

int e2econd_analyze(e2econd_handle* h, const int16_t* pcm, long long stride, const int64_t* lens, int B, long long n, int trim, int cap, e2econd_row* rows_out,
                    int32_t* ranges_out) {
  if (!h) return E2ECOND_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  // ---- validation: nothing is enqueued before the last check
  if (!pcm) return h->fail(E2ECOND_EINVAL, "pcm must not be NULL");
  if (const char* m = pl::analyze_check(B, n, stride, trim, cap))
    return h->fail(E2ECOND_EINVAL, std::string(m) + " (B " + std::to_string(B) + ", n " + std::to_string(n) + ", stride " + std::to_string(stride) + ", trim " +
                                       std::to_string(trim) + ", cap " + std::to_string(cap) + ")");
  if ((uintptr_t)pcm % 2) return h->fail(E2ECOND_EINVAL, "pcm is not aligned to its element size");
  std::vector<int64_t> nv((size_t)B, (int64_t)n);
  if (lens) RET(fetch_host(h, lens, (size_t)B, nv));
  for (int b = 0; b < B; ++b)
    if (nv[b] < 0 || nv[b] > n)
      return h->fail(E2ECOND_EINVAL, "lens[" + std::to_string(b) + "] = " + std::to_string((long long)nv[b]) + ": need 0 <= lens <= n = " + std::to_string(n));
  if (!h->configured) return h->fail(E2ECOND_ESTATE, "e2econd_analyze before e2econd_configure");
  const int rate = h->rate, W = h->W;
  std::vector<RowIn>& hr = h->host_rows;
  hr.resize((size_t)B);
  long long max_nb = 0, max_starts = 0;
  for (int b = 0; b < B; ++b) {
    const long long len = pl::len_ms(nv[b], rate);
    if (len > MAX_LEN_MS) return h->fail(E2ECOND_EINVAL, "lens[" + std::to_string(b) + "]: a row holds at most 2^30 ms");
    hr[b].N = nv[b];
    hr[b].len_ms = (int)len;
    hr[b].nb = (int)pl::n_bins(nv[b], rate, len);
    max_nb = std::max<long long>(max_nb, hr[b].nb);
    max_starts = std::max<long long>(max_starts, pl::n_starts(len, W));
  }
  const long long fwords = std::max<long long>(1, pl::ceil_div(max_starts, 64));
  // ---- enqueue
  RET(begin_call(h));
  h->analyzed = false;
  h->rB = 0;
  const bool host_in = !is_device_pointer(pcm);
  RET(reserve(h, h->rows, (size_t)B * sizeof(RowIn)));
  RET(reserve(h, h->bins, (size_t)B * std::max<long long>(1, max_nb) * 8));
  RET(reserve(h, h->flags, (size_t)B * fwords * 8));
  RET(reserve(h, h->ranges, (size_t)B * cap * 8));
  RET(reserve(h, h->recs, (size_t)B * sizeof(e2econd_row)));
  RET(reserve(h, h->spans, (size_t)B * sizeof(int2)));
  if (host_in) RET(reserve(h, h->in, (size_t)B * n * 2));
  hipStream_t s = h->stream;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[0], s));
  HIPCHK(h, hipMemcpyAsync(h->rows.p, hr.data(), (size_t)B * sizeof(RowIn), hipMemcpyHostToDevice, s));
  const int16_t* x = pcm;
  long long xs = stride;
  if (host_in) {   // host samples: only the n samples of each row travel
    RET(copy_rows(h, h->in.p, (size_t)n * 2, pcm, (size_t)stride * 2, (size_t)n * 2, B));
    x = (const int16_t*)h->in.p;
    xs = n;
  }
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[1], s));
  HIPCHK(h, hipMemsetAsync(h->ranges.p, 0, (size_t)B * cap * 8, s));
  const RowIn* rows = (const RowIn*)h->rows.p;
  u64* bins = (u64*)h->bins.p;
  u64* flags = (u64*)h->flags.p;
  e2econd_row* recs = (e2econd_row*)h->recs.p;
  int2* spans = (int2*)h->spans.p;
  if (max_nb > 0) hipLaunchKernelGGL(bins_kernel, dim3(grid_x(max_nb, pl::BIN_TILE), (unsigned)B), dim3(pl::THREADS), 0, s, x, xs, rows, bins, max_nb, rate);
  if (max_starts > 0)
    hipLaunchKernelGGL(window_kernel, dim3(grid_x(max_starts, h->tile.T), (unsigned)B), dim3(pl::THREADS), (size_t)h->tile.lds_words * 8, s, bins, max_nb, rows, flags,
                       fwords, W, h->k, rate, h->tile.T);
  hipLaunchKernelGGL(ranges_kernel, dim3((unsigned)B), dim3(64), 0, s, flags, fwords, rows, (int32_t*)h->ranges.p, cap, recs, spans, W, rate, trim);
  if (max_nb > 0) hipLaunchKernelGGL(span_kernel, dim3(grid_x(max_nb, pl::SPAN_TILE), (unsigned)B), dim3(pl::THREADS), 0, s, bins, max_nb, spans, recs);
  HIPCHK(h, hipGetLastError());
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[2], s));
  h->host_recs.resize((size_t)B);
  HIPCHK(h, hipMemcpyAsync(h->host_recs.data(), recs, (size_t)B * sizeof(e2econd_row), hipMemcpyDeviceToHost, s));   // the one small fetch
  const bool rows_dev = rows_out && is_device_pointer(rows_out);
  if (rows_dev) HIPCHK(h, hipMemcpyAsync(rows_out, recs, (size_t)B * sizeof(e2econd_row), hipMemcpyDeviceToDevice, s));
  RET(copy_out(h, ranges_out, h->ranges.p, (size_t)B * cap * 8));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[3], s));
  const Phase phases[3] = {{0, 1}, {1, 2}, {2, 3}};   // upload, compute, fetch
  RET(finish(h, phases));
  if (rows_out && !rows_dev) memcpy(rows_out, h->host_recs.data(), (size_t)B * sizeof(e2econd_row));
  long long width = 0;
  for (int b = 0; b < B; ++b) {
    if (h->host_recs[b].n_ranges > cap)
      return h->fail(E2ECOND_EINVAL, "row " + std::to_string(b) + " has " + std::to_string(h->host_recs[b].n_ranges) + " silence ranges, cap is " + std::to_string(cap));
    width = std::max<long long>(width, h->host_recs[b].n_out);
  }
  h->analyzed = true;
  h->aB = B;
  h->src = x;
  h->src_stride = xs;
  h->width = width;
  return E2ECOND_OK;
}

int e2econd_apply(e2econd_handle* h, const double* gain, int want, int16_t* pcm_out, float* wav_out, long long out_stride, long long* width_out) {
  if (!h) return E2ECOND_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!gain) return h->fail(E2ECOND_EINVAL, "gain must not be NULL");
  if (want < 1 || want > (E2ECOND_WANT_PCM | E2ECOND_WANT_WAV)) return h->fail(E2ECOND_EINVAL, "want must be E2ECOND_WANT_PCM, E2ECOND_WANT_WAV or both");
  if ((pcm_out && !(want & E2ECOND_WANT_PCM)) || (wav_out && !(want & E2ECOND_WANT_WAV))) return h->fail(E2ECOND_EINVAL, "an output pointer without its E2ECOND_WANT_* bit");
  if (!h->analyzed) return h->fail(E2ECOND_ESTATE, "e2econd_apply without a completed e2econd_analyze");
  const int B = h->aB;
  const long long width = h->width;
  RET(fetch_host(h, gain, (size_t)B, h->host_gain));
  for (int b = 0; b < B; ++b)
    if (!std::isfinite(h->host_gain[b]) || h->host_gain[b] < 0) return h->fail(E2ECOND_EINVAL, "gain[" + std::to_string(b) + "] must be finite and not negative");
  if ((pcm_out || wav_out) && out_stride < width)
    return h->fail(E2ECOND_EINVAL, "out_stride must be at least the width " + std::to_string(width) + " (got " + std::to_string(out_stride) + ")");
  if (width_out) *width_out = width;
  h->rB = 0;
  if (width == 0) return E2ECOND_OK;
  // ---- enqueue
  RET(begin_call(h));
  const long long os = pl::out_stride(width);
  RET(reserve(h, h->gain, (size_t)B * 8));
  if (want & E2ECOND_WANT_PCM) RET(reserve(h, h->pcm, (size_t)B * os * 2));
  if (want & E2ECOND_WANT_WAV) RET(reserve(h, h->wav, (size_t)B * os * 4));
  hipStream_t s = h->stream;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[0], s));
  HIPCHK(h, hipMemcpyAsync(h->gain.p, h->host_gain.data(), (size_t)B * 8, hipMemcpyHostToDevice, s));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[1], s));
  int16_t* pcm = (want & E2ECOND_WANT_PCM) ? (int16_t*)h->pcm.p : nullptr;
  float* wav = (want & E2ECOND_WANT_WAV) ? (float*)h->wav.p : nullptr;
  hipLaunchKernelGGL(apply_kernel, dim3(grid_x(os, 8 * pl::THREADS), (unsigned)B), dim3(pl::THREADS), 0, s, h->src, h->src_stride, (const RowIn*)h->rows.p,
                     (const e2econd_row*)h->recs.p, (const double*)h->gain.p, pcm, wav, os, h->rate);
  HIPCHK(h, hipGetLastError());
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[2], s));
  if (pcm_out) RET(copy_rows(h, pcm_out, (size_t)out_stride * 2, pcm, (size_t)os * 2, (size_t)width * 2, B));
  if (wav_out) RET(copy_rows(h, wav_out, (size_t)out_stride * 4, wav, (size_t)os * 4, (size_t)width * 4, B));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[3], s));
  const Phase phases[3] = {{0, 1}, {1, 2}, {2, 3}};   // upload, compute, fetch
  RET(finish(h, phases));
  h->rB = B;
  h->rS = os;
  h->rwant = want;
  return E2ECOND_OK;
}

const int16_t* e2econd_pcm_dev(e2econd_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB && (h->rwant & E2ECOND_WANT_PCM) ? (const int16_t*)h->pcm.p : nullptr;
}

const float* e2econd_wav_dev(e2econd_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB && (h->rwant & E2ECOND_WANT_WAV) ? (const float*)h->wav.p : nullptr;
}

long long e2econd_out_stride(const e2econd_handle* h) { return h && h->rB ? h->rS : 0; }

long long e2econd_tile_starts(const e2econd_handle* h) { return h && h->configured ? (long long)h->tile.T : 0; }

int e2econd_profile_enable(e2econd_handle* h, int on) { return companion::profile_enable(h, on); }
int e2econd_profile_read(e2econd_handle* h, double ms_out[3]) { return companion::profile_read(h, ms_out); }

#ifdef E2ECOND_TEST_HOOKS
int e2econd_debug_poison_workspace(e2econd_handle* h) {
  if (!h) return E2ECOND_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(poison_workspaces(h));
  h->unfinished = false;
  h->analyzed = false;
  h->rB = 0;
  h->mB = 0;
  return E2ECOND_OK;
}
#endif

}  // extern "C"
