// libe2etts_f0.so: the f0 track of a recording on the mel grid, and the data loader's pitch targets, behind the C ABI of
// include/e2etts_f0.h (the definition is there).  A companion of libe2etts_hip.so; it is linked with its kernel objects as every
// companion is, and uses none of them.
//
// Four kernels:
//   analyse   a workgroup takes F consecutive frames of one row and stages their samples once in LDS (the windows overlap by W - hop).
//             A wavefront owns a frame at a time: mean (a float64 sum, rounded once), a = (x - m) w into its own LDS row with a zero
//             tail, then the lags -- a lane owns four consecutive lags, reads a[i0 + tau .. + 7] as two aligned 16-byte words (lanes on
//             consecutive words: no bank conflict; the second word is the next step's first) and a[i0 .. i0 + 3] as one broadcast word: 16
//             fused multiply-adds per three LDS reads, every lag summed over ascending i in chunks of 32 terms.  Then r, the local maxima
//             (ballot + popcount into a list), the parabola and K - 1 rounds of a wavefront argmax.
//   rowpeak   one workgroup per row: g = max_t p_t through an LDS tree (no atomics), then the unvoiced strengths.
//   path      one wavefront per row: lane = (to-candidate j, a slice of four from-candidates), a two-step shuffle reduction, sequential over
//             the frames in double; sixteen 4-bit back-pointers are one 64-bit word per frame; the backtrack reads 64 words at a time and
//             walks them with shuffles.  log2 f is taken once per candidate, four frames at a time: the slice lanes of a candidate
//             load four consecutive frames, so the next block's loads are in flight under this block's steps.
//   targets   one workgroup per row: previous and next voiced frame by LDS scans over per-thread chunks, np.interp's arithmetic in
//             double without contraction.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../../include/e2etts_f0.h"
#ifdef E2EF0_TEST_HOOKS
#define E2E_COMPANION_TEST_HOOKS
#endif
#include "../companion/handle.h"
#include "plan.h"

#ifndef E2EF0_SRC_HASH
#define E2EF0_SRC_HASH "unknown"
#endif

using namespace e2etts;
using namespace e2etts::companion;
namespace pl = e2ef0_plan;

static_assert(E2EF0_OK == E_OK && E2EF0_EINVAL == E_INVAL && E2EF0_EHIP == E_HIP && E2EF0_ESTATE == E_STATE && E2EF0_ENOMEM == E_NOMEM,
              "include/e2etts_f0.h and csrc/companion/handle.h disagree on the error codes");
static_assert(E2EF0_MAX_B == pl::MAX_B && E2EF0_MAX_K == pl::MAX_K && E2EF0_MIN_RATE == pl::MIN_RATE && E2EF0_MAX_RATE == pl::MAX_RATE,
              "include/e2etts_f0.h and csrc/f0/plan.h disagree on the limits");
static_assert(pl::THREADS == 64 * pl::WAVES && pl::LANE_LAGS == 4 && pl::MAX_K == 16, "the kernels are written for these");

namespace {

typedef unsigned long long u64;

struct RowIn {
  long long n;   // valid samples
  int T;         // frames
  int pad;
};

// what the analysis kernel needs of the configuration
struct Analysis {
  int hop, W, h, tau_min, tau_max, NL, NL4, Wp, AL, NC, F, stage4;
  int K;
  float sr, floor_hz, octave_cost;
};

__device__ __forceinline__ float sample_of(const float* x, long long i) { return x[i]; }
__device__ __forceinline__ float sample_of(const int16_t* x, long long i) { return (float)x[i] * (1.0f / 32768.0f); }   // exact

template <typename T_in>
__global__ void __launch_bounds__(pl::THREADS) analyse_kernel(const T_in* x, long long stride, const RowIn* rows, Analysis g, const float* w, const float* rw,
                                                              float* cand_f, float* cand_s, float* peaks, float* r_out, int T) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long b = blockIdx.y;
  const RowIn row = rows[b];
  const long long t0 = (long long)blockIdx.x * g.F;
  if (t0 >= row.T) return;   // uniform over the workgroup
  const int nf = (int)min((long long)g.F, row.T - t0);
  float* stage = lds;
  float* a = lds + g.stage4 + wv * g.AL;
  float* r = lds + g.stage4 + pl::WAVES * g.AL + wv * g.NL4;
  {
    const long long s0 = pl::first_sample(t0, g.hop, g.h);
    const int need = (nf - 1) * g.hop + g.W;   // <= stage
    const T_in* xr = x + b * stride;
    for (int j = tid; j < need; j += pl::THREADS) {
      const long long s = s0 + j;
      stage[j] = (s >= 0 && s < row.n) ? sample_of(xr, s) : 0.f;
    }
  }
  __syncthreads();
  // every wavefront makes the same number of rounds (the barriers below are uniform); one past the tile's frames is idle
  for (int f0 = 0; f0 < nf; f0 += pl::WAVES) {
    const int fi = f0 + wv;
    const bool active = fi < nf;
    const long long t = t0 + fi;
    const float* xs = stage + pl::frame_offset(t, t0, g.hop);
    float pk = 0.f;
    if (active) {
      double sum = 0.0;
      for (int i = lane; i < g.W; i += 64) sum += (double)xs[i];
      for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);   // the same tree in every lane
      const float m = (float)(sum / (double)g.W);
      for (int i = lane; i < g.AL; i += 64) {
        float v = 0.f;
        if (i < g.W) {
          const float d = xs[i] - m;
          pk = fmaxf(pk, fabsf(d));
          v = d * w[i];
        }
        a[i] = v;
      }
      for (int d = 32; d >= 1; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d));
    }
    __syncthreads();
    if (active) {
      for (int tau0 = lane * 4; tau0 < g.NL4; tau0 += pl::PASS_LAGS) {
        float tot0 = 0.f, tot1 = 0.f, tot2 = 0.f, tot3 = 0.f;
        float4 cur = *reinterpret_cast<const float4*>(a + tau0);
        for (int c0 = 0; c0 < g.Wp; c0 += pl::CHUNK) {   // a chunk of CHUNK terms in one accumulator; the chunk sums in ascending order
          float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
          const int c1 = min(c0 + pl::CHUNK, g.Wp);
          for (int i0 = c0; i0 < c1; i0 += 4) {   // reads a[.. i0 + tau0 + 7], at most Wp + NL4 - 1 < AL
            const float4 nxt = *reinterpret_cast<const float4*>(a + i0 + tau0 + 4);
            const float4 av = *reinterpret_cast<const float4*>(a + i0);
            acc0 = fmaf(av.x, cur.x, acc0); acc0 = fmaf(av.y, cur.y, acc0); acc0 = fmaf(av.z, cur.z, acc0); acc0 = fmaf(av.w, cur.w, acc0);
            acc1 = fmaf(av.x, cur.y, acc1); acc1 = fmaf(av.y, cur.z, acc1); acc1 = fmaf(av.z, cur.w, acc1); acc1 = fmaf(av.w, nxt.x, acc1);
            acc2 = fmaf(av.x, cur.z, acc2); acc2 = fmaf(av.y, cur.w, acc2); acc2 = fmaf(av.z, nxt.x, acc2); acc2 = fmaf(av.w, nxt.y, acc2);
            acc3 = fmaf(av.x, cur.w, acc3); acc3 = fmaf(av.y, nxt.x, acc3); acc3 = fmaf(av.z, nxt.y, acc3); acc3 = fmaf(av.w, nxt.z, acc3);
            cur = nxt;
          }
          tot0 += acc0, tot1 += acc1, tot2 += acc2, tot3 += acc3;
        }
        *reinterpret_cast<float4*>(r + tau0) = make_float4(tot0, tot1, tot2, tot3);
      }
    }
    __syncthreads();
    const float ra0 = active ? r[0] : 0.f;
    __syncthreads();
    if (active) {
      for (int tau = lane; tau < g.NL; tau += 64) {
        const float v = ra0 > 0.f ? r[tau] / (ra0 * rw[tau]) : 0.f;
        r[tau] = v;
        if (r_out) r_out[((size_t)b * T + t) * g.NL + tau] = v;
      }
    }
    __syncthreads();
    // the local maxima, in ascending tau, into a list that reuses the wavefront's `a`
    float* cs = a;
    float* cf = a + g.NC;
    int* ct = reinterpret_cast<int*>(a + 2 * g.NC);
    int count = 0;
    if (active && ra0 > 0.f) {
      for (int base = g.tau_min; base <= g.tau_max; base += 64) {
        const int tau = base + lane;
        bool is_max = false;
        float rm = 0.f, r0 = 0.f, rp = 0.f;
        if (tau <= g.tau_max) {   // tau - 1 >= 1 and tau + 1 <= tau_max + 1 = NL - 1
          rm = r[tau - 1], r0 = r[tau], rp = r[tau + 1];
          is_max = r0 > rm && r0 >= rp && r0 > 0.f;
        }
        const u64 mask = __ballot(is_max);
        if (is_max) {
          const int pos = count + __popcll(mask & (((u64)1 << lane) - 1));   // < NC: two neighbours are never both maxima
          const float d = 0.5f * (rm - rp) / (rm - 2.f * r0 + rp);
          const float v = fminf(1.f, r0 - 0.25f * (rm - rp) * d);
          const float lag = (float)tau + d;
          cs[pos] = v - g.octave_cost * log2f(g.floor_hz * lag / g.sr);
          cf[pos] = g.sr / lag;
          ct[pos] = tau;
        }
        count += __popcll(mask);
      }
    }
    __syncthreads();
    float* of = cand_f + ((size_t)b * T + t) * g.K;
    float* os = cand_s + ((size_t)b * T + t) * g.K;
    for (int k = 1; k < g.K; ++k) {   // K is uniform: so are these barriers
      float bs = -INFINITY;
      int bt = 0x7fffffff, bi = -1;
      for (int c = lane; c < count; c += 64) {
        const float s = cs[c];
        const int tau = ct[c];
        if (s > bs || (s == bs && tau < bt)) bs = s, bt = tau, bi = c;
      }
      for (int d = 32; d >= 1; d >>= 1) {
        const float s2 = __shfl_xor(bs, d);
        const int t2 = __shfl_xor(bt, d), i2 = __shfl_xor(bi, d);
        if (s2 > bs || (s2 == bs && t2 < bt)) bs = s2, bt = t2, bi = i2;
      }
      const bool found = bi >= 0 && bs > -INFINITY;
      if (active && lane == 0) {
        of[k] = found ? cf[bi] : 0.f;
        os[k] = found ? bs : -INFINITY;
        if (found) cs[bi] = -INFINITY;
      }
      __syncthreads();
    }
    if (active && lane == 0) {
      of[0] = 0.f;
      os[0] = 0.f;   // the row-peak kernel writes the unvoiced strength
      peaks[(size_t)b * T + t] = pk;
    }
  }
}

__global__ void __launch_bounds__(256) rowpeak_kernel(const RowIn* rows, const float* peaks, float* cand_s, int T, int K, double vt, double st) {
  __shared__ float part[256];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int Tb = rows[b].T;
  float g = 0.f;
  for (int t = tid; t < Tb; t += 256) g = fmaxf(g, peaks[(size_t)b * T + t]);
  part[tid] = g;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) part[tid] = fmaxf(part[tid], part[tid + d]);
    __syncthreads();
  }
  g = part[0];
  const double scale = st / (1.0 + vt);
  for (int t = tid; t < Tb; t += 256) {
    double su = vt + 2.0;
    if (g > 0.f) su = vt + fmax(0.0, 2.0 - ((double)peaks[(size_t)b * T + t] / (double)g) / scale);
    cand_s[((size_t)b * T + t) * K] = (float)su;
  }
}

__global__ void __launch_bounds__(64) path_kernel(const RowIn* rows, const int32_t* frames, const float* cand_f, const float* cand_s, u64* bp, float* f0, int T, int K,
                                                  double vuc, double ojc) {
  __shared__ double dprev[2][16], plf[2][16];   // the previous frame's cells; frame t writes [t & 1] and reads the other
  __shared__ int pv[2][16];
  const int lane = threadIdx.x, j = lane >> 2, sl = lane & 3;
  const long long b = blockIdx.x;
  const int Tb = frames ? frames[b] : rows[b].T;
  const float* rf = cand_f + (size_t)b * T * K;
  const float* rs = cand_s + (size_t)b * T * K;
  u64* rbp = bp + (size_t)b * T;
  float* out = f0 + (size_t)b * T;
  for (int t = Tb + lane; t < T; t += 64) out[t] = 0.f;
  if (Tb <= 0) return;   // uniform
  const bool have = j < K;
  // frames go in blocks of four: lane (j, sl) loads candidate j of frame tb + sl and takes its log2, the next block's loads are in
  // flight under this block's four steps, and a step fetches its frame's values from the lane that holds them
  float nf = 0.f, ns = -INFINITY;
  if (have && sl < Tb) nf = rf[(size_t)sl * K + j], ns = rs[(size_t)sl * K + j];
  double delta = 0.0;
  for (int tb = 0; tb < Tb; tb += 4) {   // uniform
    const float bf = nf, bs = ns;
    nf = 0.f, ns = -INFINITY;
    if (have && tb + 4 + sl < Tb) nf = rf[(size_t)(tb + 4 + sl) * K + j], ns = rs[(size_t)(tb + 4 + sl) * K + j];
    const int bvoiced = bs > -INFINITY && bf > 0.f;
    const double blf = bvoiced ? log2((double)bf) : 0.0;
    const int nq = min(4, Tb - tb);
    for (int q = 0; q < nq; ++q) {
      const int t = tb + q, src = (lane & ~3) | q;
      const float cs = __shfl(bs, src);
      const int voiced = __shfl(bvoiced, src);
      const double lf = __shfl(blf, src);
      const bool empty = !(cs > -INFINITY);
      const int cur = t & 1, prv = cur ^ 1;
      int bi = sl * 4;
      if (t == 0) {
        delta = empty ? -INFINITY : (double)cs;
      } else {
        double best = -INFINITY;
        for (int k = 0; k < 4; ++k) {
          const int i = sl * 4 + k;
          if (i < K) {
            const int pvi = pv[prv][i];
            const double cost = (pvi && voiced) ? ojc * fabs(plf[prv][i] - lf) : (pvi != voiced ? vuc : 0.0);
            const double val = dprev[prv][i] - cost;
            if (val > best) best = val, bi = i;
          }
        }
        for (int d = 1; d <= 2; d <<= 1) {
          const double b2 = __shfl_xor(best, d);
          const int i2 = __shfl_xor(bi, d);
          if (b2 > best || (b2 == best && i2 < bi)) best = b2, bi = i2;
        }
        delta = empty ? -INFINITY : best + (double)cs;
        u64 word = 0;
        for (int bit = 0; bit < 4; ++bit) word |= __ballot(sl == 0 && ((bi >> bit) & 1)) << bit;   // lane 4 j: bits 4 j .. 4 j + 3
        if (lane == 0) rbp[t] = word;
      }
      if (sl == 0) dprev[cur][j] = delta, plf[cur][j] = lf, pv[cur][j] = voiced;
      __syncthreads();   // frame t + 1 reads [cur] after it and writes [prv], which every lane has read before it
    }
  }
  // the end of the path: the first maximum
  double best = (sl == 0 && have) ? delta : -INFINITY;
  int jcur = (sl == 0 && have) ? j : 99;
  for (int d = 32; d >= 1; d >>= 1) {
    const double b2 = __shfl_xor(best, d);
    const int j2 = __shfl_xor(jcur, d);
    if (b2 > best || (b2 == best && j2 < jcur)) best = b2, jcur = j2;
  }
  if (jcur > 15) jcur = 0;
  __threadfence();
  __syncthreads();
  for (int tend = Tb; tend > 0; tend -= 64) {
    const int tlo = max(0, tend - 64), cnt = tend - tlo;
    const int t = tlo + lane;
    const u64 word = (lane < cnt && t > 0) ? rbp[t] : 0;
    int myj = 0;
    for (int l = cnt - 1; l >= 0; --l) {
      if (lane == l) myj = jcur;
      const u64 wl = __shfl(word, l);
      if (tlo + l > 0) jcur = (int)((wl >> (4 * jcur)) & 15);
    }
    if (lane < cnt) out[t] = rf[(size_t)t * K + myj];
  }
}

__global__ void __launch_bounds__(256) targets_kernel(const RowIn* rows, const float* f0, float* tf0, float* tuv, int T, double mean, double sd, int mode, double eps) {
#pragma clang fp contract(off)
  __shared__ int sprev[2][256], snext[2][256];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int Tb = rows[b].T;
  const float* f = f0 + (size_t)b * T;
  float* of = tf0 + (size_t)b * T;
  float* ou = tuv + (size_t)b * T;
  for (int t = Tb + tid; t < T; t += 256) of[t] = 0.f, ou[t] = 0.f;
  const int NONE = 0x7fffffff;
  const int chunk = (Tb + 255) / 256;
  const int lo = min(tid * chunk, Tb), hi = min(lo + chunk, Tb);
  int lastv = -1, firstv = NONE;
  for (int t = lo; t < hi; ++t)
    if (f[t] != 0.f) {
      lastv = t;
      if (firstv == NONE) firstv = t;
    }
  sprev[0][tid] = lastv;
  snext[0][tid] = firstv;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < 256; d <<= 1) {   // inclusive scans: max of the last voiced frame from the left, min of the first from the right
    int p = sprev[cur][tid], q = snext[cur][tid];
    if (tid >= d) p = max(p, sprev[cur][tid - d]);
    if (tid + d < 256) q = min(q, snext[cur][tid + d]);
    sprev[cur ^ 1][tid] = p;
    snext[cur ^ 1][tid] = q;
    __syncthreads();
    cur ^= 1;
  }
  int prev = tid > 0 ? sprev[cur][tid - 1] : -1;            // the last voiced frame before this chunk
  const int after = tid < 255 ? snext[cur][tid + 1] : NONE;   // the first voiced frame after it
  const bool any = sprev[cur][255] >= 0;
  const auto value = [&](int t) { return mode == E2EF0_LOG ? log2((double)f[t] + eps) : ((double)f[t] - mean) / sd; };
  int nxt = -1;   // the next voiced frame at or after t (stale while < t)
  for (int t = lo; t < hi; ++t) {
    if (f[t] != 0.f) {
      of[t] = (float)value(t);
      ou[t] = 0.f;
      prev = t;
      continue;
    }
    if (nxt < t) {
      nxt = after;
      for (int u = t + 1; u < hi; ++u)
        if (f[u] != 0.f) {
          nxt = u;
          break;
        }
    }
    double y = 0.0;
    if (any) {
      if (prev < 0) y = value(nxt);
      else if (nxt == NONE) y = value(prev);
      else {
        const double y0 = value(prev), y1 = value(nxt);
        const double slope = (y1 - y0) / ((double)nxt - (double)prev);
        y = slope * ((double)t - (double)prev) + y0;
      }
    }
    of[t] = (float)y;
    ou[t] = 1.f;
  }
}

thread_local std::string g_create_error;

enum Stop { STOP_ACF, STOP_CANDIDATES, STOP_TRACK };

}  // namespace

struct e2ef0_handle : Handle {
  int sr = 0, hop = 0;
  bool configured = false;
  e2ef0_params par{};
  pl::Geometry geo;
  Buf w{this, Buf::WEIGHTS}, rw{this, Buf::WEIGHTS};
  Buf in{this}, rows{this}, cand_f{this}, cand_s{this}, peaks{this}, bp{this}, f0{this}, tf0{this}, tuv{this}, acf{this}, frames{this};
  std::vector<RowIn> host_rows;   // outlive the asynchronous copies of a call
  std::vector<int64_t> host_lens;
  int rB = 0, rT = 0;             // the resident track (0: none)
  bool have_targets = false;
};

namespace {

int copy_rows(e2ef0_handle* h, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
  if (!width || !rows) return E2EF0_OK;
  if (rows == 1 || (dpitch == width && spitch == width)) HIPCHK(h, hipMemcpyAsync(dst, src, width * rows, hipMemcpyDefault, h->stream));
  else HIPCHK(h, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDefault, h->stream));
  return E2EF0_OK;
}

Analysis analysis_of(const e2ef0_handle* h) {
  const pl::Geometry& q = h->geo;
  Analysis g;
  g.hop = q.hop; g.W = q.W; g.h = q.h; g.tau_min = q.tau_min; g.tau_max = q.tau_max; g.NL = q.NL; g.NL4 = q.NL4; g.Wp = q.Wp; g.AL = q.AL; g.NC = q.NC;
  g.F = q.F; g.stage4 = pl::round_up(q.stage, 4);
  g.K = h->par.max_candidates;
  g.sr = (float)q.sr; g.floor_hz = (float)h->par.floor; g.octave_cost = (float)h->par.octave_cost;
  return g;
}

// the path search over the candidates in h->cand_f / h->cand_s (frames: device [B] int32, or NULL for the rows' own counts)
int launch_path(e2ef0_handle* h, const int32_t* frames, int B, int T) {
  const double c = 0.01 * (double)h->sr / (double)h->hop;
  hipLaunchKernelGGL(path_kernel, dim3((unsigned)B), dim3(64), 0, h->stream, (const RowIn*)h->rows.p, frames, (const float*)h->cand_f.p, (const float*)h->cand_s.p,
                     (u64*)h->bp.p, (float*)h->f0.p, T, h->par.max_candidates, h->par.voiced_unvoiced_cost * c, h->par.octave_jump_cost * c);
  HIPCHK(h, hipGetLastError());
  return E2EF0_OK;
}

// e2ef0_forward and the two hooks that stop earlier (the mutex held)
int run(e2ef0_handle* h, Stop stop, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n, float* out_a, float* out_b,
        int64_t* lens_out, int* T_out) {
  // ---- validation: nothing is enqueued before the last check
  if (!audio) return h->fail(E2EF0_EINVAL, "audio must not be NULL");
  if (dtype != E2EF0_F32 && dtype != E2EF0_I16) return h->fail(E2EF0_EINVAL, "dtype must be E2EF0_F32 or E2EF0_I16 (got " + std::to_string(dtype) + ")");
  if (!h->configured) return h->fail(E2EF0_ESTATE, "e2ef0_forward before e2ef0_configure");
  const int K = h->par.max_candidates, NL = h->geo.NL, hop = h->hop;
  if (const char* m = pl::batch_check(B, n, audio_stride, hop, std::max(K, NL)))
    return h->fail(E2EF0_EINVAL, std::string(m) + " (B " + std::to_string(B) + ", n " + std::to_string(n) + ", audio_stride " + std::to_string(audio_stride) + ")");
  const size_t esz = dtype == E2EF0_I16 ? 2 : 4;
  if ((uintptr_t)audio % esz) return h->fail(E2EF0_EINVAL, "audio is not aligned to its element size");
  std::vector<int64_t> nv((size_t)B, (int64_t)n);
  if (n_valid) RET(fetch_host(h, n_valid, (size_t)B, nv));
  int T = 0;
  for (int b = 0; b < B; ++b) {
    if (nv[b] < 0 || nv[b] > n)
      return h->fail(E2EF0_EINVAL, "n_valid[" + std::to_string(b) + "] = " + std::to_string((long long)nv[b]) + ": need 0 <= n_valid <= n = " + std::to_string(n));
    T = std::max(T, (int)pl::frames_of(nv[b], hop));
  }
  if (T < 1) return h->fail(E2EF0_EINVAL, "no row holds a frame: need n_valid >= hop = " + std::to_string(hop) + " in at least one row");
  // ---- enqueue
  RET(begin_call(h));
  h->rB = 0;
  h->have_targets = false;
  h->host_rows.resize((size_t)B);
  h->host_lens.resize((size_t)B);
  for (int b = 0; b < B; ++b) {
    h->host_rows[b].n = nv[b];
    h->host_rows[b].T = (int)pl::frames_of(nv[b], hop);
    h->host_rows[b].pad = 0;
    h->host_lens[b] = h->host_rows[b].T;
  }
  const size_t cells = (size_t)B * T;
  RET(reserve(h, h->rows, (size_t)B * sizeof(RowIn)));
  RET(reserve(h, h->cand_f, cells * K * 4));
  RET(reserve(h, h->cand_s, cells * K * 4));
  RET(reserve(h, h->peaks, cells * 4));
  RET(reserve(h, h->bp, cells * 8));
  RET(reserve(h, h->f0, cells * 4));
  if (stop == STOP_ACF) RET(reserve(h, h->acf, cells * NL * 4));
  const bool host_in = !is_device_pointer(audio);
  if (host_in) RET(reserve(h, h->in, (size_t)B * n * esz));
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->rows.p, h->host_rows.data(), (size_t)B * sizeof(RowIn), hipMemcpyHostToDevice, s));
  const void* x = audio;
  long long xs = audio_stride;
  if (host_in) {   // host samples: only the n samples of each row travel
    RET(copy_rows(h, h->in.p, (size_t)n * esz, audio, (size_t)audio_stride * esz, (size_t)n * esz, B));
    x = h->in.p;
    xs = n;
  }
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[0], s));
  HIPCHK(h, hipMemsetAsync(h->cand_f.p, 0, cells * K * 4, s));
  HIPCHK(h, hipMemsetAsync(h->cand_s.p, 0, cells * K * 4, s));
  if (stop == STOP_ACF) HIPCHK(h, hipMemsetAsync(h->acf.p, 0, cells * NL * 4, s));
  const Analysis g = analysis_of(h);
  const RowIn* rows = (const RowIn*)h->rows.p;
  float* r_out = stop == STOP_ACF ? (float*)h->acf.p : nullptr;
  const dim3 grid((unsigned)pl::tiles_of(T, g.F), (unsigned)B);
  const size_t lds = (size_t)h->geo.lds_floats * 4;
  if (dtype == E2EF0_I16)
    hipLaunchKernelGGL(analyse_kernel<int16_t>, grid, dim3(pl::THREADS), lds, s, (const int16_t*)x, xs, rows, g, (const float*)h->w.p, (const float*)h->rw.p,
                       (float*)h->cand_f.p, (float*)h->cand_s.p, (float*)h->peaks.p, r_out, T);
  else
    hipLaunchKernelGGL(analyse_kernel<float>, grid, dim3(pl::THREADS), lds, s, (const float*)x, xs, rows, g, (const float*)h->w.p, (const float*)h->rw.p,
                       (float*)h->cand_f.p, (float*)h->cand_s.p, (float*)h->peaks.p, r_out, T);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(rowpeak_kernel, dim3((unsigned)B), dim3(256), 0, s, rows, (const float*)h->peaks.p, (float*)h->cand_s.p, T, K, h->par.voicing_threshold,
                     h->par.silence_threshold);
  HIPCHK(h, hipGetLastError());
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[1], s));
  if (stop == STOP_TRACK) RET(launch_path(h, nullptr, B, T));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[2], s));
  if (stop == STOP_ACF) RET(copy_out(h, out_a, h->acf.p, cells * NL * 4));
  if (stop == STOP_CANDIDATES) {
    RET(copy_out(h, out_a, h->cand_f.p, cells * K * 4));
    RET(copy_out(h, out_b, h->cand_s.p, cells * K * 4));
  }
  if (stop == STOP_TRACK) RET(copy_out(h, out_a, h->f0.p, cells * 4));
  if (lens_out) HIPCHK(h, hipMemcpyAsync(lens_out, h->host_lens.data(), (size_t)B * 8, hipMemcpyDefault, s));
  HIPCHK(h, hipStreamSynchronize(s));
  h->unfinished = false;
  if (h->profile) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->last_ms[0] = ms;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->last_ms[1] = ms;
  }
  if (T_out) *T_out = T;
  if (stop == STOP_TRACK) {
    h->rB = B;
    h->rT = T;
  }
  return E2EF0_OK;
}

const char* geometry_of(int sr, int hop, double floor_hz, double ceiling_hz, pl::Geometry* g) { return pl::geometry(sr, hop, floor_hz, ceiling_hz, g); }

}  // namespace

extern "C" {

const char* e2ef0_version(void) { return "e2etts-f0 1 E2EF0_SRC_HASH=" E2EF0_SRC_HASH; }
int e2ef0_abi_version(void) { return E2EF0_ABI_VERSION; }

const char* e2ef0_last_error(const e2ef0_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int e2ef0_create(int device_id, int sample_rate, int hop, e2ef0_handle** out) {
  if (!out) {
    g_create_error = "e2ef0_create: out is NULL";
    return E2EF0_EINVAL;
  }
  *out = nullptr;
  if (device_id < 0) {
    g_create_error = "e2ef0_create: device_id must not be negative";
    return E2EF0_EINVAL;
  }
  if (sample_rate < pl::MIN_RATE || sample_rate > pl::MAX_RATE || hop < 1 || hop > sample_rate) {
    g_create_error = "e2ef0_create: need sample_rate in [1000, 384000] and hop in [1, sample_rate] (got " + std::to_string(sample_rate) + ", " + std::to_string(hop) + ")";
    return E2EF0_EINVAL;
  }
  e2ef0_handle* h = new (std::nothrow) e2ef0_handle();
  if (!h) {
    g_create_error = "out of host memory";
    return E2EF0_ENOMEM;
  }
  h->device = device_id;
  h->sr = sample_rate;
  h->hop = hop;
  *out = h;
  return E2EF0_OK;
}

void e2ef0_destroy(e2ef0_handle* h) { companion::destroy(h); }

int e2ef0_window(int sample_rate, int hop, double floor_hz, double ceiling_hz) {
  pl::Geometry g;
  return geometry_of(sample_rate, hop, floor_hz, ceiling_hz, &g) ? E2EF0_EINVAL : g.W;
}
int e2ef0_lags(int sample_rate, int hop, double floor_hz, double ceiling_hz) {
  pl::Geometry g;
  return geometry_of(sample_rate, hop, floor_hz, ceiling_hz, &g) ? E2EF0_EINVAL : g.NL;
}
int e2ef0_tau_min(int sample_rate, int hop, double floor_hz, double ceiling_hz) {
  pl::Geometry g;
  return geometry_of(sample_rate, hop, floor_hz, ceiling_hz, &g) ? E2EF0_EINVAL : g.tau_min;
}
int e2ef0_tile_frames(const e2ef0_handle* h) { return h && h->configured ? h->geo.F : 0; }

int e2ef0_configure(e2ef0_handle* h, const e2ef0_params* p, const float* w, const float* r_w) {
  if (!h) return E2EF0_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!p || !w || !r_w) return h->fail(E2EF0_EINVAL, "params, w and r_w must not be NULL");
  if (const char* m = pl::params_check(p->struct_size, sizeof(e2ef0_params), p->voicing_threshold, p->silence_threshold, p->octave_cost, p->octave_jump_cost,
                                       p->voiced_unvoiced_cost, p->max_candidates))
    return h->fail(E2EF0_EINVAL, m);
  pl::Geometry g;
  if (const char* m = pl::geometry(h->sr, h->hop, p->floor, p->ceiling, &g))
    return h->fail(E2EF0_EINVAL, std::string(m) + " (sample_rate " + std::to_string(h->sr) + ", hop " + std::to_string(h->hop) + ", floor " + std::to_string(p->floor) +
                                     ", ceiling " + std::to_string(p->ceiling) + ")");
  for (int i = 0; i < g.W; ++i)
    if (!std::isfinite(w[i]) || w[i] < 0.f || w[i] > 1.f) return h->fail(E2EF0_EINVAL, "w[" + std::to_string(i) + "] must lie in [0, 1]");
  if (r_w[0] != 1.f) return h->fail(E2EF0_EINVAL, "r_w[0] must be 1");
  for (int i = 0; i < g.NL; ++i)
    if (!std::isfinite(r_w[i]) || !(r_w[i] > 0.f) || r_w[i] > 1.f) return h->fail(E2EF0_EINVAL, "r_w[" + std::to_string(i) + "] must lie in (0, 1]");
  RET(open_device(h));
  // staged in buffers of their own and swapped in only when both have arrived: a failure leaves the configuration held before in place
  Buf nb[2];
  int rc = reserve(h, nb[0], (size_t)g.W * 4);
  if (rc == E2EF0_OK) rc = reserve(h, nb[1], (size_t)g.NL * 4);
  if (rc == E2EF0_OK && hipMemcpy(nb[0].p, w, (size_t)g.W * 4, hipMemcpyHostToDevice) != hipSuccess) rc = h->fail(E2EF0_EHIP, "upload of w failed");
  if (rc == E2EF0_OK && hipMemcpy(nb[1].p, r_w, (size_t)g.NL * 4, hipMemcpyHostToDevice) != hipSuccess) rc = h->fail(E2EF0_EHIP, "upload of r_w failed");
  if (rc != E2EF0_OK) {
    (void)hipGetLastError();
    for (Buf& b : nb) release(h, b);
    return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));   // nothing reads the old tables
  release(h, h->w);
  release(h, h->rw);
  h->w.p = nb[0].p, h->w.bytes = nb[0].bytes;
  h->rw.p = nb[1].p, h->rw.bytes = nb[1].bytes;
  h->par = *p;
  h->geo = g;
  h->configured = true;
  h->rB = 0;
  h->have_targets = false;
  return E2EF0_OK;
}

void* e2ef0_stream(e2ef0_handle* h) { return companion::stream(h); }
int e2ef0_order_after(e2ef0_handle* h, void* caller_stream) { return companion::order_after(h, caller_stream); }
int e2ef0_sync(e2ef0_handle* h) { return companion::sync(h); }
size_t e2ef0_device_bytes(const e2ef0_handle* h) { return companion::device_bytes(h); }

int e2ef0_forward(e2ef0_handle* h, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n, float* f0_out, int64_t* lens_out,
                  int* T_out) {
  if (!h) return E2EF0_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  return run(h, STOP_TRACK, audio, dtype, audio_stride, n_valid, B, n, f0_out, nullptr, lens_out, T_out);
}

int e2ef0_targets(e2ef0_handle* h, double mean, double sd, int mode, double eps, float* f0_t_out, float* uv_out) {
  if (!h) return E2EF0_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (mode != E2EF0_LINEAR && mode != E2EF0_LOG) return h->fail(E2EF0_EINVAL, "mode must be E2EF0_LINEAR or E2EF0_LOG (got " + std::to_string(mode) + ")");
  if (mode == E2EF0_LINEAR && (!std::isfinite(mean) || !std::isfinite(sd) || sd == 0.0)) return h->fail(E2EF0_EINVAL, "mean and std must be finite, std not 0");
  if (mode == E2EF0_LOG && (!std::isfinite(eps) || eps < 0.0)) return h->fail(E2EF0_EINVAL, "eps must be finite and not negative");
  if (!h->rB) return h->fail(E2EF0_ESTATE, "e2ef0_targets without a resident track (no forward has completed)");
  const int B = h->rB, T = h->rT;
  const size_t cells = (size_t)B * T;
  RET(begin_call(h));
  h->have_targets = false;
  RET(reserve(h, h->tf0, cells * 4));
  RET(reserve(h, h->tuv, cells * 4));
  hipStream_t s = h->stream;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[3], s));
  hipLaunchKernelGGL(targets_kernel, dim3((unsigned)B), dim3(256), 0, s, (const RowIn*)h->rows.p, (const float*)h->f0.p, (float*)h->tf0.p, (float*)h->tuv.p, T, mean, sd,
                     mode, eps);
  HIPCHK(h, hipGetLastError());
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[4], s));
  RET(copy_out(h, f0_t_out, h->tf0.p, cells * 4));
  RET(copy_out(h, uv_out, h->tuv.p, cells * 4));
  HIPCHK(h, hipStreamSynchronize(s));
  h->unfinished = false;
  if (h->profile) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[3], h->ev[4]));
    h->last_ms[2] = ms;
  }
  h->have_targets = true;
  return E2EF0_OK;
}

const float* e2ef0_f0_dev(e2ef0_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB ? (const float*)h->f0.p : nullptr;
}
const float* e2ef0_target_f0_dev(e2ef0_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB && h->have_targets ? (const float*)h->tf0.p : nullptr;
}
const float* e2ef0_target_uv_dev(e2ef0_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB && h->have_targets ? (const float*)h->tuv.p : nullptr;
}

int e2ef0_profile_enable(e2ef0_handle* h, int on) { return companion::profile_enable(h, on); }
int e2ef0_profile_read(e2ef0_handle* h, double ms_out[3]) { return companion::profile_read(h, ms_out); }

#ifdef E2EF0_TEST_HOOKS
int e2ef0_debug_poison_workspace(e2ef0_handle* h) {
  if (!h) return E2EF0_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(poison_workspaces(h));
  h->unfinished = false;
  h->rB = 0;
  h->have_targets = false;
  return E2EF0_OK;
}

int e2ef0_debug_acf(e2ef0_handle* h, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n, float* r_out, int* T_out) {
  if (!h) return E2EF0_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  return run(h, STOP_ACF, audio, dtype, audio_stride, n_valid, B, n, r_out, nullptr, nullptr, T_out);
}

int e2ef0_debug_candidates(e2ef0_handle* h, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n, float* freq_out,
                           float* strength_out, int* T_out) {
  if (!h) return E2EF0_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  return run(h, STOP_CANDIDATES, audio, dtype, audio_stride, n_valid, B, n, freq_out, strength_out, nullptr, T_out);
}

int e2ef0_debug_path(e2ef0_handle* h, const float* freq, const float* strength, const int32_t* frames, int B, int T, float* f0_out) {
  if (!h) return E2EF0_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!freq || !strength || !frames) return h->fail(E2EF0_EINVAL, "freq, strength and frames must not be NULL");
  if (!h->configured) return h->fail(E2EF0_ESTATE, "e2ef0_debug_path before e2ef0_configure");
  const int K = h->par.max_candidates;
  if (B < 1 || B > pl::MAX_B || T < 1 || T > pl::MAX_T || (long long)B * T * K > pl::MAX_CELLS) return h->fail(E2EF0_EINVAL, "need 1 <= B <= 4096, 1 <= T <= 2^24, B * T * K <= 2^31");
  std::vector<int32_t> fr;
  RET(fetch_host(h, frames, (size_t)B, fr));
  for (int b = 0; b < B; ++b)
    if (fr[b] < 0 || fr[b] > T) return h->fail(E2EF0_EINVAL, "frames[" + std::to_string(b) + "] must lie in [0, T]");
  const size_t cells = (size_t)B * T;
  std::vector<float> s0;   // index 0 of every frame in use must hold a candidate
  RET(fetch_host(h, strength, cells * K, s0));
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < fr[b]; ++t)
      if (!(s0[((size_t)b * T + t) * K] > -INFINITY)) return h->fail(E2EF0_EINVAL, "candidate 0 of row " + std::to_string(b) + ", frame " + std::to_string(t) + " is empty or NaN");
  RET(begin_call(h));
  h->rB = 0;
  h->have_targets = false;
  RET(reserve(h, h->rows, (size_t)B * sizeof(RowIn)));
  h->host_rows.resize((size_t)B);
  for (int b = 0; b < B; ++b) h->host_rows[b] = RowIn{0, fr[b], 0};
  RET(reserve(h, h->cand_f, cells * K * 4));
  RET(reserve(h, h->cand_s, cells * K * 4));
  RET(reserve(h, h->bp, cells * 8));
  RET(reserve(h, h->f0, cells * 4));
  RET(reserve(h, h->frames, (size_t)B * 4));
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->cand_f.p, freq, cells * K * 4, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(h->cand_s.p, s0.data(), cells * K * 4, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->frames.p, fr.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->rows.p, h->host_rows.data(), (size_t)B * sizeof(RowIn), hipMemcpyHostToDevice, s));
  RET(launch_path(h, (const int32_t*)h->frames.p, B, T));
  RET(copy_out(h, f0_out, h->f0.p, cells * 4));
  HIPCHK(h, hipStreamSynchronize(s));
  h->unfinished = false;
  h->rB = B;   // the track is resident as a forward's is: e2ef0_targets can be run on constructed tracks
  h->rT = T;
  return E2EF0_OK;
}
#endif

}  // extern "C"
