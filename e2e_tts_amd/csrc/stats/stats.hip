// libe2etts_stats.so: what the reference's build_stats writes into stats.json -- mean and std of the voiced f0 frames, and for energy
// and pitch the mean and std of every utterance's values inside its own IQR fences with the min and max of the normalised values --
// from rows that lie on the device, and the data loader's energy target, behind the C ABI of include/e2etts_stats.h (the definition is
// there).  A companion of libe2etts_hip.so; it is linked with its kernel objects as every companion is, and uses none of them.
//
// Three kernels:
//   row_stats  one workgroup per row, sized for the batch's longest row; a row works with the threads and keys-per-thread of its OWN
//              length (plan.h: threads, elems), the other threads only meet the barriers, so a row's record does not depend on its batch.
//              The row is loaded into LDS as 32-bit keys in float order (16-byte loads when the row is aligned), padded with +inf to a
//              power of two, and sorted by a bitonic network: key r of thread t is element r * NT + t, so a stage's partner is another
//              register of the thread (distance >= NT), lane t ^ j of the wavefront (distance < 64: a shuffle) or, for the distances
//              between, an LDS read behind a barrier.  Every thread then reads the four order statistics and finds the kept range's ends
//              by binary search; the image is dead after that and its first bytes serve the reductions: thread-strided partials in
//              double from the registers, a shuffle tree per wavefront, the wavefronts' partials summed in order.  No atomics.
//   merge      one wavefront folds the rows' records into the kind's resident accumulator by Chan's update, strictly in row order.
//   normalize  elementwise.
//
// Contraction is off for the whole file: the percentile and fence arithmetic is numpy's, operation by operation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../../include/e2etts_stats.h"
#ifdef E2EST_TEST_HOOKS
#define E2E_COMPANION_TEST_HOOKS
#endif
#include "../companion/handle.h"
#include "plan.h"

#pragma clang fp contract(off)

#ifndef E2EST_SRC_HASH
#define E2EST_SRC_HASH "unknown"
#endif

using namespace e2etts;
using namespace e2etts::companion;
namespace pl = e2est_plan;

static_assert(E2EST_OK == E_OK && E2EST_EINVAL == E_INVAL && E2EST_EHIP == E_HIP && E2EST_ESTATE == E_STATE && E2EST_ENOMEM == E_NOMEM,
              "include/e2etts_stats.h and csrc/companion/handle.h disagree on the error codes");
static_assert(E2EST_MAX_B == pl::MAX_B && E2EST_MAX_ROW == pl::MAX_ROW, "include/e2etts_stats.h and csrc/stats/plan.h disagree on the limits");
static_assert(E2EST_F0 == pl::KIND_F0 && E2EST_ENERGY == pl::KIND_ENERGY && E2EST_PITCH == pl::KIND_PITCH, "include/e2etts_stats.h and csrc/stats/plan.h disagree on the kinds");
static_assert(sizeof(e2est_row) == pl::ROW_BYTES && sizeof(e2est_block) == 88 && sizeof(e2est_stats) == 264, "the records of include/e2etts_stats.h");
static_assert(pl::WAVE == 64 && pl::MAX_E == 16 && pl::MAX_THREADS == 1024, "the kernels are written for these");

namespace {

// the resident accumulator of one kind
struct Acc {
  int64_t rows, n_frames, n;
  double mean, m2;
  float rmin, rmax;
  int32_t err_row, err_add;   // the first refused row and the add it came with (err_row < 0: none)
};
static_assert(sizeof(Acc) == pl::ACC_BYTES, "plan.h: ACC_BYTES");

__device__ __forceinline__ float value_of(uint32_t key) { return __uint_as_float(pl::bits_of(key)); }

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);   // the same tree in every lane
  return v;
}

// the sum of v over the workgroup, in every thread: the row's nw wavefronts leave their sums in scratch, summed in order.  The threads
// beyond them hold 0 and only meet the barriers.  A barrier stands between the caller's last use of scratch and this call.
__device__ __forceinline__ double block_sum(double v, double* scratch, int tid, int nw) {
  v = wave_sum(v);
  const int w = tid >> 6;
  if ((tid & 63) == 0 && w < nw) scratch[w] = v;
  __syncthreads();
  double t = scratch[0];
  for (int i = 1; i < nw; ++i) t = t + scratch[i];
  __syncthreads();
  return t;
}

// numpy's _lerp on float32: each operation rounded
__device__ __forceinline__ float lerp_np(float a, float b, float g) {
  const float d = b - a;
  if (g < 0.5f) return a + d * g;
  return b - d * (1.0f - g);
}

template <int E>
__device__ __forceinline__ void sort_image(uint32_t (&key)[E], uint32_t* s, int P, int NT, int tid, bool active) {
  for (int k = 2; k <= P; k <<= 1) {       // uniform
    for (int j = k >> 1; j >= 1; j >>= 1) {   // uniform
      const int cls = pl::stage_class(j, NT);
      if (cls == pl::STAGE_REG) {
        if (active) {
#pragma unroll
          for (int d = E >> 1; d >= 1; d >>= 1) {
            if (d * NT != j) continue;
#pragma unroll
            for (int r = 0; r < E; ++r) {
              if (r & d) continue;
              const bool asc = pl::keeps_min(r * NT + tid, j, k);
              const uint32_t a = key[r], b = key[r | d];
              const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
              key[r] = asc ? lo : hi;
              key[r | d] = asc ? hi : lo;
            }
          }
        }
      } else if (cls == pl::STAGE_SHFL) {
        if (active) {   // whole wavefronts: NT is a multiple of 64
#pragma unroll
          for (int r = 0; r < E; ++r) {
            const uint32_t other = __shfl_xor(key[r], j);
            const bool mn = pl::keeps_min(r * NT + tid, j, k);
            key[r] = mn ? (key[r] < other ? key[r] : other) : (key[r] < other ? other : key[r]);
          }
        }
      } else {
        if (active) {
#pragma unroll
          for (int r = 0; r < E; ++r) s[r * NT + tid] = key[r];
        }
        __syncthreads();
        if (active) {
#pragma unroll
          for (int r = 0; r < E; ++r) {
            const int i = r * NT + tid;
            const uint32_t other = s[pl::partner(i, j)];
            const bool mn = pl::keeps_min(i, j, k);
            key[r] = mn ? (key[r] < other ? key[r] : other) : (key[r] < other ? other : key[r]);
          }
        }
        __syncthreads();
      }
    }
  }
}

__device__ __forceinline__ void refuse_row(e2est_row* rec, int n);

// a scaled row whose image lies in s: sort, percentiles, fences, the kept range, its sums
template <int E>
__device__ __forceinline__ void scaled_row(uint32_t* s, int n, int P, int NT, int tid, e2est_row* rec, float* sorted_row) {
  const bool active = tid < NT;
  uint32_t key[E];
#pragma unroll
  for (int r = 0; r < E; ++r) key[r] = active ? s[r * NT + tid] : pl::KEY_PAD;   // a thread rewrites only the cells it read
  sort_image<E>(key, s, P, NT, tid, active);
  if (active) {
#pragma unroll
    for (int r = 0; r < E; ++r) s[r * NT + tid] = key[r];
  }
  __syncthreads();
  // a non-finite value has sorted to an end of the row: -inf and the negative NaNs to the front, +inf and the positive NaNs behind
  if (s[0] <= pl::KEY_NEG_INF || s[n - 1] >= pl::KEY_PAD) {   // uniform
    if (tid == 0) refuse_row(rec, n);
    return;
  }
  const pl::VIndex q25 = pl::vindex(n, 25), q75 = pl::vindex(n, 75);
  const float p25 = lerp_np(value_of(s[q25.lo]), value_of(s[q25.hi]), q25.gamma);
  const float p75 = lerp_np(value_of(s[q75.lo]), value_of(s[q75.hi]), q75.gamma);
  const float spread = 1.5f * (p75 - p25);
  const float lower = p25 - spread, upper = p75 + spread;
  const float vmin = value_of(s[0]), vmax = value_of(s[n - 1]);
  int lo = 0, hi = n;   // the first index whose value is above the lower fence
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (value_of(s[mid]) > lower) hi = mid;
    else lo = mid + 1;
  }
  const int k0 = lo;
  lo = 0, hi = n;       // the first index whose value is not below the upper fence
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (value_of(s[mid]) < upper) lo = mid + 1;
    else hi = mid;
  }
  const int k1 = lo;
  const int nk = k1 > k0 ? k1 - k0 : 0;
  if (sorted_row)
    for (int i = tid; i < n; i += blockDim.x) sorted_row[i] = value_of(s[i]);
  __syncthreads();   // the image is dead: its first bytes are the reductions' scratch
  double* scratch = reinterpret_cast<double*>(s);
  const int nw = NT >> 6;
  double acc = 0.0;
  if (active) {
#pragma unroll
    for (int r = 0; r < E; ++r) {
      const int i = r * NT + tid;
      if (i >= k0 && i < k1) acc = acc + (double)value_of(key[r]);
    }
  }
  const double sum = block_sum(acc, scratch, tid, nw);
  const double mean = nk > 0 ? sum / (double)nk : 0.0;
  acc = 0.0;
  if (active) {
#pragma unroll
    for (int r = 0; r < E; ++r) {
      const int i = r * NT + tid;
      if (i >= k0 && i < k1) {
        const double d = (double)value_of(key[r]) - mean;
        acc = acc + d * d;
      }
    }
  }
  const double m2 = block_sum(acc, scratch, tid, nw);
  if (tid == 0) {
    e2est_row o;
    o.n = n, o.n_kept = nk, o.sum = sum, o.mean = mean, o.m2 = nk > 0 ? m2 : 0.0;
    o.p25 = p25, o.p75 = p75, o.lower = lower, o.upper = upper, o.min = vmin, o.max = vmax;
    o.status = 0, o.reserved = 0;
    *rec = o;
  }
}

__device__ __forceinline__ void refuse_row(e2est_row* rec, int n) {
  e2est_row o;
  o.n = n, o.n_kept = 0, o.sum = 0.0, o.mean = 0.0, o.m2 = 0.0;
  o.p25 = o.p75 = o.lower = o.upper = o.min = o.max = 0.f;
  o.status = 1, o.reserved = 0;
  *rec = o;
}

// grid = B rows, block = plan.h's threads for the longest row's image; dynamic LDS = that image
__global__ void __launch_bounds__(pl::MAX_THREADS) row_stats_kernel(const float* values, long long row_stride, const int* lens, e2est_row* rows, int kind,
                                                                    float* sorted_out, long long sorted_stride) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_keys[];
  const int tid = threadIdx.x, b = blockIdx.x, BT = blockDim.x;
  const int n = lens[b];                 // 1 <= n <= MAX_ROW (validated on the host)
  const int P = pl::image(n), NT = pl::threads(P);   // the row's own plan: NT <= BT
  const float* row = values + (size_t)b * (size_t)row_stride;
  if (kind == pl::KIND_F0) {
    int bad = 0;
    double cnt = 0.0, acc = 0.0;
    if (tid < NT) {
      for (int i = tid; i < n; i += NT) {
        const float v = row[i];
        bad |= pl::non_finite(__float_as_uint(v)) ? 1 : 0;
        if (v != 0.f) cnt = cnt + 1.0, acc = acc + (double)v;
      }
    }
    double* scratch = reinterpret_cast<double*>(lds_keys);
    const int nw = NT >> 6;
    if (block_sum((double)bad, scratch, tid, nw) > 0.0) {   // uniform
      if (tid == 0) refuse_row(rows + b, n);
      return;
    }
    const double nv = block_sum(cnt, scratch, tid, nw);
    const double sum = block_sum(acc, scratch, tid, nw);
    const double mean = nv > 0.0 ? sum / nv : 0.0;
    acc = 0.0;
    if (tid < NT) {
      for (int i = tid; i < n; i += NT) {
        const float v = row[i];
        if (v != 0.f) {
          const double d = (double)v - mean;
          acc = acc + d * d;
        }
      }
    }
    const double m2 = block_sum(acc, scratch, tid, nw);
    if (tid == 0) {
      e2est_row o;
      o.n = n, o.n_kept = (long long)nv, o.sum = sum, o.mean = mean, o.m2 = nv > 0.0 ? m2 : 0.0;
      o.p25 = o.p75 = o.lower = o.upper = o.min = o.max = 0.f;
      o.status = 0, o.reserved = 0;
      rows[b] = o;
    }
    return;
  }
  // the image: n keys, then +inf to P.  Nothing beyond n is read from the row.
  int done = 0;
  if (((uintptr_t)row & 15) == 0) {
    const int n4 = n >> 2;
    for (int q = tid; q < n4; q += BT) {
      const float4 v = reinterpret_cast<const float4*>(row)[q];
      const uint32_t b0 = __float_as_uint(v.x), b1 = __float_as_uint(v.y), b2 = __float_as_uint(v.z), b3 = __float_as_uint(v.w);
      *reinterpret_cast<uint4*>(lds_keys + 4 * q) = make_uint4(pl::key_of(b0), pl::key_of(b1), pl::key_of(b2), pl::key_of(b3));
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < n; i += BT) {
    lds_keys[i] = pl::key_of(__float_as_uint(row[i]));
  }
  for (int i = n + tid; i < P; i += BT) lds_keys[i] = pl::KEY_PAD;
  __syncthreads();
  float* sorted_row = sorted_out ? sorted_out + (size_t)b * (size_t)sorted_stride : nullptr;
  switch (pl::elems(P)) {   // uniform
    case 1: scaled_row<1>(lds_keys, n, P, NT, tid, rows + b, sorted_row); break;
    case 2: scaled_row<2>(lds_keys, n, P, NT, tid, rows + b, sorted_row); break;
    case 4: scaled_row<4>(lds_keys, n, P, NT, tid, rows + b, sorted_row); break;
    case 8: scaled_row<8>(lds_keys, n, P, NT, tid, rows + b, sorted_row); break;
    default: scaled_row<16>(lds_keys, n, P, NT, tid, rows + b, sorted_row); break;
  }
}

// one wavefront: the rows' records into the kind's accumulator, in row order
__global__ void __launch_bounds__(64) merge_kernel(const e2est_row* rows, int B, Acc* acc, int add_no) {
  const int lane = threadIdx.x;
  Acc a = *acc;
  if (a.err_row >= 0) return;   // a row was refused before: nothing more is taken until the reset
  for (int base = 0; base < B; base += 64) {   // uniform
    const int r = base + lane;
    const unsigned long long m = __ballot(r < B && rows[r].status != 0);
    if (m) {
      if (lane == 0) acc->err_row = base + __ffsll((long long)m) - 1, acc->err_add = add_no;
      return;
    }
  }
  for (int base = 0; base < B; base += 64) {   // uniform
    const int r = base + lane;
    const bool have = r < B;
    long long nb = 0, frames = 0;
    double mb = 0.0, m2b = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    if (have) {
      const e2est_row o = rows[r];
      nb = o.n_kept, frames = o.n, mb = o.mean, m2b = o.m2, mn = o.min, mx = o.max;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      frames += __shfl_xor(frames, d);
      mn = fminf(mn, __shfl_xor(mn, d));
      mx = fmaxf(mx, __shfl_xor(mx, d));
    }
    a.n_frames += frames;
    a.rmin = fminf(a.rmin, mn), a.rmax = fmaxf(a.rmax, mx);
    const int cnt = min(64, B - base);
    a.rows += cnt;
    for (int k = 0; k < cnt; ++k) {   // every lane folds the same values
      const long long nk = __shfl(nb, k);
      const double mk = __shfl(mb, k), m2k = __shfl(m2b, k);
      if (nk == 0) continue;
      if (a.n == 0) {
        a.n = nk, a.mean = mk, a.m2 = m2k;
      } else {
        const double na = (double)a.n, nbd = (double)nk, nt = (double)(a.n + nk);
        const double d = mk - a.mean;
        a.mean = a.mean + d * nbd / nt;
        a.m2 = a.m2 + m2k + d * d * na * nbd / nt;
        a.n += nk;
      }
    }
  }
  if (lane == 0) *acc = a;
}

__global__ void __launch_bounds__(256) normalize_kernel(const float* values, long long row_stride, const int* lens, float* out, int T, float mean, float std) {
  const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (t >= T) return;
  float r = 0.f;
  if (t < lens[b]) r = __fdiv_rn(values[(size_t)b * (size_t)row_stride + t] - mean, std);
  out[(size_t)b * T + t] = r;
}

thread_local std::string g_create_error;
const char* const KIND_NAME[pl::KINDS] = {"f0", "energy", "pitch"};

Acc empty_acc() {
  Acc a;
  memset(&a, 0, sizeof a);
  a.rmin = INFINITY, a.rmax = -INFINITY, a.err_row = -1;
  return a;
}
const Acc EMPTY[pl::KINDS] = {empty_acc(), empty_acc(), empty_acc()};   // static: an asynchronous copy reads it

}  // namespace

struct e2est_handle : Handle {
  Buf acc{this}, rows{this}, lens{this}, sorted{this};
  std::vector<std::vector<int32_t>> pending;   // host lengths whose asynchronous copies may not have run yet; emptied when the stream drains
  bool acc_ready = false, have_rows = false, timed_add = false, timed_norm = false;
  int last_B = 0, adds = 0;
  std::vector<e2est_row> host_rows;
};

namespace {

// drains the stream; with profiling, reads the phases recorded since
int drain(e2est_handle* h) {
  if (!h->open) return E2EST_OK;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->pending.clear();
  float ms = 0.f;
  if (h->timed_add) {
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->last_ms[0] = ms;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->last_ms[1] = ms;
    h->timed_add = false;
  }
  if (h->timed_norm) {
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[3], h->ev[4]));
    h->last_ms[2] = ms;
    h->timed_norm = false;
  }
  return E2EST_OK;
}

int reset(e2est_handle* h) {
  RET(open_device(h));
  RET(reserve(h, h->acc, sizeof EMPTY));
  HIPCHK(h, hipMemcpyAsync(h->acc.p, EMPTY, sizeof EMPTY, hipMemcpyHostToDevice, h->stream));
  h->acc_ready = true;
  h->have_rows = false;
  h->adds = 0;
  return E2EST_OK;
}

std::string shape_text(int B, int T, int64_t row_stride) { return " (B " + std::to_string(B) + ", T " + std::to_string(T) + ", row_stride " + std::to_string((long long)row_stride) + ")"; }

// the checks every entry point that reads rows shares, and the lengths as int32 (max_len: the longest)
int take_rows(e2est_handle* h, const float* values, int64_t row_stride, const int64_t* lens, int B, int T, bool sorting, std::vector<int32_t>& l32, int* max_len) {
  if (const char* m = pl::shape_check(B, T, row_stride)) return h->fail(E2EST_EINVAL, std::string(m) + shape_text(B, T, row_stride));
  if (!values || !lens) return h->fail(E2EST_EINVAL, "values and lens must not be NULL");
  if ((uintptr_t)values % 4) return h->fail(E2EST_EINVAL, "values must be aligned to 4 bytes");
  std::vector<int64_t> l64;
  RET(fetch_host(h, lens, (size_t)B, l64));
  l32.resize((size_t)B);
  *max_len = 0;
  for (int b = 0; b < B; ++b) {
    if (const char* m = sorting ? pl::len_check(l64[b], T) : pl::norm_len_check(l64[b], T))
      return h->fail(E2EST_EINVAL, std::string(m) + " (row " + std::to_string(b) + ": lens[" + std::to_string(b) + "] = " + std::to_string((long long)l64[b]) + ", T " + std::to_string(T) + ")");
    l32[b] = (int32_t)l64[b];
    if (l32[b] > *max_len) *max_len = l32[b];
  }
  if (!is_device_pointer(values)) return h->fail(E2EST_EINVAL, "values must be device memory");
  return E2EST_OK;
}

int upload_lens(e2est_handle* h, std::vector<int32_t>& l32) {
  const size_t B = l32.size();
  RET(reserve(h, h->lens, B * 4));
  h->pending.emplace_back();
  h->pending.back().swap(l32);
  HIPCHK(h, hipMemcpyAsync(h->lens.p, h->pending.back().data(), B * 4, hipMemcpyHostToDevice, h->stream));
  return E2EST_OK;
}

int launch_rows(e2est_handle* h, int kind, const float* values, int64_t row_stride, int B, int max_len, float* sorted_out, int64_t sorted_stride) {
  const int P = pl::image(max_len);
  hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)B), dim3((unsigned)pl::threads(P)), (size_t)pl::lds_bytes(P), h->stream, values, (long long)row_stride,
                     (const int*)h->lens.p, (e2est_row*)h->rows.p, kind, sorted_out, (long long)sorted_stride);
  HIPCHK(h, hipGetLastError());
  return E2EST_OK;
}

}  // namespace

extern "C" {

const char* e2est_version(void) { return "e2etts-stats 1 E2EST_SRC_HASH=" E2EST_SRC_HASH; }
int e2est_abi_version(void) { return E2EST_ABI_VERSION; }

const char* e2est_last_error(const e2est_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int e2est_create(int device_id, e2est_handle** out) {
  if (!out) {
    g_create_error = "e2est_create: out is NULL";
    return E2EST_EINVAL;
  }
  *out = nullptr;
  if (device_id < 0) {
    g_create_error = "e2est_create: device_id must not be negative";
    return E2EST_EINVAL;
  }
  e2est_handle* h = new (std::nothrow) e2est_handle();
  if (!h) {
    g_create_error = "out of host memory";
    return E2EST_ENOMEM;
  }
  h->device = device_id;
  *out = h;
  return E2EST_OK;
}

void e2est_destroy(e2est_handle* h) { companion::destroy(h); }

void* e2est_stream(e2est_handle* h) { return companion::stream(h); }
int e2est_order_after(e2est_handle* h, void* caller_stream) { return companion::order_after(h, caller_stream); }
size_t e2est_device_bytes(const e2est_handle* h) { return companion::device_bytes(h); }

int e2est_sync(e2est_handle* h) {
  if (!h) return E2EST_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  return drain(h);
}

int e2est_reset(e2est_handle* h) {
  if (!h) return E2EST_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->open) {   // nothing was added: the accumulators are made empty when the first add opens the device
    h->acc_ready = false, h->have_rows = false, h->adds = 0;
    return E2EST_OK;
  }
  return reset(h);
}

int e2est_add(e2est_handle* h, int kind, const float* values, int64_t row_stride, const int64_t* lens, int B, int T) {
  if (!h) return E2EST_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (const char* m = pl::kind_check(kind)) return h->fail(E2EST_EINVAL, std::string(m) + " (got " + std::to_string(kind) + ")");
  std::vector<int32_t> l32;
  int max_len = 0;
  RET(take_rows(h, values, row_stride, lens, B, T, true, l32, &max_len));
  RET(open_device(h));
  if (!h->acc_ready) RET(reset(h));
  h->have_rows = false;
  RET(reserve(h, h->rows, (size_t)B * sizeof(e2est_row)));
  RET(upload_lens(h, l32));
  hipStream_t s = h->stream;
  const bool timed = h->profile;
  if (timed) HIPCHK(h, hipEventRecord(h->ev[0], s));
  RET(launch_rows(h, kind, values, row_stride, B, max_len, nullptr, 0));
  if (timed) HIPCHK(h, hipEventRecord(h->ev[1], s));
  hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(64), 0, s, (const e2est_row*)h->rows.p, B, (Acc*)h->acc.p + kind, h->adds);
  HIPCHK(h, hipGetLastError());
  if (timed) HIPCHK(h, hipEventRecord(h->ev[2], s));
  h->timed_add = timed;
  h->adds += 1;
  h->last_B = B;
  h->have_rows = true;
  return E2EST_OK;
}

int e2est_fetch_rows(e2est_handle* h, e2est_row* out) {
  if (!h) return E2EST_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!out) return h->fail(E2EST_EINVAL, "out must not be NULL");
  if (!h->have_rows) return h->fail(E2EST_ESTATE, "e2est_fetch_rows without an add since the last reset");
  RET(drain(h));
  const size_t bytes = (size_t)h->last_B * sizeof(e2est_row);
  h->host_rows.resize((size_t)h->last_B);
  HIPCHK(h, hipMemcpy(h->host_rows.data(), h->rows.p, bytes, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(out, h->rows.p, bytes, hipMemcpyDefault));
  for (int b = 0; b < h->last_B; ++b)
    if (h->host_rows[b].status != 0) return h->fail(E2EST_EINVAL, "row " + std::to_string(b) + " of the last add holds a non-finite value: the add was refused");
  return E2EST_OK;
}

int e2est_result(e2est_handle* h, e2est_stats* out) {
  if (!h) return E2EST_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!out) return h->fail(E2EST_EINVAL, "out must not be NULL");
  memset(out, 0, sizeof *out);
  if (!h->open || !h->acc_ready) return E2EST_OK;   // nothing was added: every kind is absent
  RET(drain(h));
  Acc acc[pl::KINDS];
  HIPCHK(h, hipMemcpy(acc, h->acc.p, sizeof acc, hipMemcpyDeviceToHost));
  for (int k = 0; k < pl::KINDS; ++k) {
    const Acc& a = acc[k];
    if (a.err_row >= 0)
      return h->fail(E2EST_EINVAL, std::string(KIND_NAME[k]) + ": row " + std::to_string(a.err_row) + " of add " + std::to_string(a.err_add) + " (counted from the last reset) holds a non-finite value; that add was refused, and every add of this kind after it");
  }
  for (int k = 0; k < pl::KINDS; ++k) {
    const Acc& a = acc[k];
    if (a.rows == 0) continue;
    if (a.n == 0) {
      memset(out, 0, sizeof *out);
      return h->fail(E2EST_ESTATE, std::string(KIND_NAME[k]) + (k == pl::KIND_F0 ? ": no voiced frame was added" : ": no value lies inside its row's fences") + " (" + std::to_string((long long)a.rows) + " rows, " + std::to_string((long long)a.n_frames) + " frames): there is no mean and no std");
    }
    e2est_block& o = out->kind[k];
    o.present = 1, o.rows = a.rows, o.n_frames = a.n_frames, o.n_kept = a.n;
    o.mean = a.mean, o.m2 = a.m2;
    o.std = std::sqrt(a.m2 / (double)a.n);
    if (k != pl::KIND_F0) {
      if (a.m2 == 0.0) o.std = 1.0;
      o.raw_min = (double)a.rmin, o.raw_max = (double)a.rmax;
      o.min = ((double)a.rmin - o.mean) / o.std;
      o.max = ((double)a.rmax - o.mean) / o.std;
    }
  }
  return E2EST_OK;
}

int e2est_normalize(e2est_handle* h, const float* values, int64_t row_stride, const int64_t* lens, int B, int T, double mean, double std, float* out) {
  if (!h) return E2EST_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!out) return h->fail(E2EST_EINVAL, "out must not be NULL");
  if (!std::isfinite(mean) || !std::isfinite(std) || !(std > 0.0) || !((float)std > 0.f) || !std::isfinite((float)mean) || !std::isfinite((float)std))
    return h->fail(E2EST_EINVAL, "mean must be finite and std positive and finite, in float32 too (got mean " + std::to_string(mean) + ", std " + std::to_string(std) + ")");
  std::vector<int32_t> l32;
  int max_len = 0;
  RET(take_rows(h, values, row_stride, lens, B, T, false, l32, &max_len));
  if ((uintptr_t)out % 4 || !is_device_pointer(out)) return h->fail(E2EST_EINVAL, "out must be device memory aligned to 4 bytes");
  RET(open_device(h));
  RET(upload_lens(h, l32));
  hipStream_t s = h->stream;
  const bool timed = h->profile;
  if (timed) HIPCHK(h, hipEventRecord(h->ev[3], s));
  hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, s, values, (long long)row_stride, (const int*)h->lens.p, out, T,
                     (float)mean, (float)std);
  HIPCHK(h, hipGetLastError());
  if (timed) HIPCHK(h, hipEventRecord(h->ev[4], s));
  h->timed_norm = timed;
  return E2EST_OK;
}

int e2est_profile_enable(e2est_handle* h, int on) { return companion::profile_enable(h, on); }
int e2est_profile_read(e2est_handle* h, double ms_out[3]) { return companion::profile_read(h, ms_out); }

#ifdef E2EST_TEST_HOOKS
int e2est_debug_poison_workspace(e2est_handle* h) {
  if (!h) return E2EST_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->open) return E2EST_OK;
  RET(drain(h));
  RET(poison_workspaces(h));
  return reset(h);
}

int e2est_debug_sorted(e2est_handle* h, const float* values, int64_t row_stride, const int64_t* lens, int B, int T, float* out) {
  if (!h) return E2EST_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!out) return h->fail(E2EST_EINVAL, "out must not be NULL");
  std::vector<int32_t> l32;
  int max_len = 0;
  RET(take_rows(h, values, row_stride, lens, B, T, true, l32, &max_len));
  RET(open_device(h));
  h->have_rows = false;
  const size_t bytes = (size_t)B * T * 4;
  RET(reserve(h, h->rows, (size_t)B * sizeof(e2est_row)));
  RET(reserve(h, h->sorted, bytes));
  RET(upload_lens(h, l32));
  HIPCHK(h, hipMemcpyAsync(h->sorted.p, out, bytes, hipMemcpyDefault, h->stream));   // what lies beyond a row's length stays
  RET(launch_rows(h, pl::KIND_ENERGY, values, row_stride, B, max_len, (float*)h->sorted.p, T));
  HIPCHK(h, hipMemcpyAsync(out, h->sorted.p, bytes, hipMemcpyDefault, h->stream));
  return drain(h);
}
#endif

}  // extern "C"
