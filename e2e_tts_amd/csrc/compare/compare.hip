// libe2etts_compare.so: how close two recordings are -- DTW over cepstra of their log-mel, and along the path the mel-cepstral
// distortion, the mel L1, the f0 error and the voiced/unvoiced error -- behind the C ABI of include/e2etts_compare.h (the definition is
// there).  A companion of libe2etts_hip.so; it is linked with its kernel objects as every companion is, and uses none of them.
//
// Four kernels:
//   cepstra   a workgroup takes a tile of frames of one utterance; the basis and the tile lie in LDS in rows padded against bank
//             conflicts (plan.h: cep_stride), the tile loaded 16 bytes wide along the mel axis; a thread owns (frame, k) values and runs
//             one fused-multiply-add chain over m ascending per value, reading both rows as 16-byte words.
//   pad       features given ready: rows padded with zeros to 16-byte words, rows past an utterance's length zeroed.
//   search    one workgroup per pair, of up to 1024 threads (plan.h: search_threads).  The shorter sequence lies on the threads in chunks of that many rows (when that is B, the tie order and
//             the back-pointer codes are swapped back), the grid sweeps the anti-diagonals of a chunk: a thread keeps its own previous
//             value and its upper neighbour's value before last in registers, reads the neighbour's last value from LDS (two rows,
//             written and read alternately: one barrier per diagonal) and its own feature row from registers; the other side's rows come
//             from L2 as 16-byte words, loaded a diagonal ahead and left in flight across the barrier.  The last row of a chunk stays in LDS for the next chunk's first thread.  The cost of a cell is
//             computed in double where it is used and never stored.  The 2-bit back-pointers of 16 neighbouring threads are merged with
//             shuffles into one 32-bit word: a diagonal's cells lie side by side (plan.h: bp_word).
//   walk      one wavefront per pair: back-tracks into LDS (a cell packs into 24 bits), then every lane takes every 64th cell in path
//             order, writes it to the path, recomputes its cost and takes its mel and f0 terms in double; the lanes' sums are reduced
//             by a fixed tree.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../../include/e2etts_compare.h"
#ifdef E2ECMP_TEST_HOOKS
#define E2E_COMPANION_TEST_HOOKS
#endif
#include "../companion/handle.h"
#include "plan.h"

#ifndef E2ECMP_SRC_HASH
#define E2ECMP_SRC_HASH "unknown"
#endif

using namespace e2etts;
using namespace e2etts::companion;
namespace pl = e2ecmp_plan;

static_assert(E2ECMP_OK == E_OK && E2ECMP_EINVAL == E_INVAL && E2ECMP_EHIP == E_HIP && E2ECMP_ESTATE == E_STATE && E2ECMP_ENOMEM == E_NOMEM,
              "include/e2etts_compare.h and csrc/companion/handle.h disagree on the error codes");
static_assert(E2ECMP_MAX_B == pl::MAX_B && E2ECMP_MAX_T == pl::MAX_T && E2ECMP_MAX_D == pl::MAX_D && E2ECMP_MAX_MEL == pl::MAX_MEL,
              "include/e2etts_compare.h and csrc/compare/plan.h disagree on the limits");
static_assert(E2ECMP_DTW == pl::MODE_DTW && E2ECMP_SYNC == pl::MODE_SYNC, "include/e2etts_compare.h and csrc/compare/plan.h disagree on the modes");
static_assert(pl::THREADS == 256 && pl::BP_CELLS == 16 && pl::search_threads_cap(16) == 1024 && pl::search_threads_cap(32) == 512 && pl::search_threads_cap(64) == 256, "the kernels are written for these");
static_assert(sizeof(e2ecmp_result) == 72, "e2ecmp_result is four int64 and five doubles");

namespace {

typedef unsigned long long u64;

struct PairIn {
  int Ta, Tb;
  long long bp_off;     // in 32-bit words
  long long path_off;   // in cells
};

__global__ void __launch_bounds__(pl::THREADS) cepstra_kernel(const float* mel, const int* lens, const float* basis, float* feat, int T, int n_mel, int n_cep, int D4,
                                                              int stride, int tile, int vec) {
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  float* sb = lds_f;                    // [n_cep, stride]
  float* sm = lds_f + n_cep * stride;   // [tile, stride]
  const int tid = threadIdx.x;
  const int b = blockIdx.y, t0 = blockIdx.x * tile;
  const int len = min(lens[b], T);
  const int nf = max(0, min(tile, len - t0));   // frames of this tile that exist
  const int M4 = pl::round_up(n_mel, 4);
  for (int idx = tid; idx < n_cep * stride; idx += pl::THREADS) {
    const int k = idx / stride, m = idx - k * stride;
    sb[idx] = m < n_mel ? basis[k * n_mel + m] : 0.f;
  }
  const float* src = mel + ((size_t)b * T + t0) * n_mel;
  if (vec) {   // n_mel is a multiple of 4 and the tensor is 16-byte aligned: so is every row
    const int q4 = n_mel / 4;
    for (int idx = tid; idx < nf * q4; idx += pl::THREADS) {
      const int f = idx / q4, q = idx - f * q4;
      *reinterpret_cast<float4*>(sm + f * stride + 4 * q) = reinterpret_cast<const float4*>(src + (size_t)f * n_mel)[q];
    }
  } else {
    for (int idx = tid; idx < nf * M4; idx += pl::THREADS) {
      const int f = idx / M4, m = idx - f * M4;
      sm[f * stride + m] = m < n_mel ? src[(size_t)f * n_mel + m] : 0.f;
    }
  }
  __syncthreads();
  for (int it = tid; it < tile * D4; it += pl::THREADS) {
    const int f = it / D4, k = it - f * D4;
    const int t = t0 + f;
    if (t >= T) break;
    float acc = 0.f;
    if (f < nf && k < n_cep) {
      const float* br = sb + k * stride;
      const float* mr = sm + f * stride;
      for (int m = 0; m < M4; m += 4) {   // whole 16-byte words are read; the chain ends at m = n_mel - 1
        const float4 bv = *reinterpret_cast<const float4*>(br + m);
        const float4 mv = *reinterpret_cast<const float4*>(mr + m);
        acc = fmaf(bv.x, mv.x, acc);
        if (m + 1 < n_mel) acc = fmaf(bv.y, mv.y, acc);
        if (m + 2 < n_mel) acc = fmaf(bv.z, mv.z, acc);
        if (m + 3 < n_mel) acc = fmaf(bv.w, mv.w, acc);
      }
    }
    feat[((size_t)b * T + t) * D4 + k] = acc;
  }
}

__global__ void __launch_bounds__(256) pad_kernel(const float* src, const int* lens, float* feat, int T, int D, int D4, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t bt = idx / D4;
  const int k = (int)(idx - bt * D4);
  const size_t b = bt / T;
  const int t = (int)(bt - b * T);
  feat[idx] = (k < D && t < lens[b]) ? src[bt * D + k] : 0.f;
}

// d(i, j) of two padded rows in double: k ascending, product and sum rounded separately -- plain operators under contract(off): the
// __dmul_rn / __dadd_rn of the HIP headers are inline functions outside this pragma and would be fused -- and the square root correctly
// rounded (the pad adds +0 terms)
template <int DMAX>
__device__ __forceinline__ double cost_of(const float (&own)[DMAX], const float4 (&y)[DMAX / 4], int D4) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < DMAX; k += 4) {
    if (k < D4) {
      const float4 v = y[k / 4];
      const double d0 = (double)own[k] - (double)v.x, d1 = (double)own[k + 1] - (double)v.y;
      const double d2 = (double)own[k + 2] - (double)v.z, d3 = (double)own[k + 3] - (double)v.w;
      acc = acc + d0 * d0;
      acc = acc + d1 * d1;
      acc = acc + d2 * d2;
      acc = acc + d3 * d3;
    }
  }
  return __dsqrt_rn(acc);
}

// row l of the swept side into registers (nothing is read for a cell that does not exist)
template <int DMAX>
__device__ __forceinline__ void load_row(float4 (&y)[DMAX / 4], const float* Y, int l, int L, int D4, bool row) {
#pragma unroll
  for (int k = 0; k < DMAX; k += 4)
    if (k < D4 && row && l >= 0 && l < L) y[k / 4] = *reinterpret_cast<const float4*>(Y + (size_t)l * D4 + k);
}

// the barrier of a diagonal: the LDS writes of this diagonal are waited for, the loads of the next diagonal's row stay in flight across it
// (a __syncthreads() would drain them first).  Nothing in global memory is handed between threads inside the kernel.
__device__ __forceinline__ void diagonal_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int DMAX, int MAX_NT>
__global__ void __launch_bounds__(MAX_NT) search_kernel(const float* fa, const float* fb, int TA, int TB, int D4, const PairIn* pairs, uint32_t* bp, double* dtot,
                                                             long long band) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  const int tid = threadIdx.x, lane = tid & 63, NT = blockDim.x;   // NT: plan.h's search_threads, a multiple of 64
  double* ex = lds_d;              // [2, NT]: row dd & 1 holds the values of diagonal dd
  double* bound = lds_d + 2 * NT;  // [L]: the last row of the chunk before
  const int p = blockIdx.x;
  const PairIn pr = pairs[p];
  const int Ta = pr.Ta, Tb = pr.Tb;
  const bool sw = pl::swapped(Ta, Tb);
  const int S = sw ? Tb : Ta, L = sw ? Ta : Tb;
  const float* X = sw ? fb + (size_t)p * TB * D4 : fa + (size_t)p * TA * D4;   // the side on the threads
  const float* Y = sw ? fa + (size_t)p * TA * D4 : fb + (size_t)p * TB * D4;   // the side that is swept
  uint32_t* w = bp + pr.bp_off;
  const double INF = INFINITY;
  for (int c0 = 0; c0 < S; c0 += NT) {   // uniform
    const int s = c0 + tid;
    const bool row = s < S;
    float own[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; k += 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row && k < D4) v = *reinterpret_cast<const float4*>(X + (size_t)s * D4 + k);
      own[k] = v.x, own[k + 1] = v.y, own[k + 2] = v.z, own[k + 3] = v.w;
    }
    ex[NT + tid] = INF;   // what diagonal 0 reads as diagonal -1
    __syncthreads();
    const bool hand_on = c0 + NT < S;   // a chunk follows: this one is full
    const int nd = min(NT, S - c0) + L - 1;
    double own_prev = INF, diag = INF;   // (s, l - 1) and (s - 1, l - 1)
    float4 ycur[DMAX / 4], ynext[DMAX / 4];   // the swept side's row of this diagonal, and of the next: loaded a diagonal ahead
#pragma unroll
    for (int k = 0; k < DMAX / 4; ++k) ycur[k] = ynext[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    load_row<DMAX>(ycur, Y, -tid, L, D4, row);
    for (int dd = 0; dd < nd; ++dd) {   // uniform
      const int l = dd - tid;
      load_row<DMAX>(ynext, Y, l + 1, L, D4, row);
      const bool act = row && l >= 0 && l < L;
      double nb;   // (s - 1, l)
      if (tid > 0) nb = ex[((dd & 1) ^ 1) * NT + tid - 1];
      else nb = (c0 > 0 && l < L) ? bound[l] : INF;
      double val = INF;
      int code = 0;
      if (act) {
        const int i = sw ? l : s, j = sw ? s : l;
        if (pl::band_allows(i, j, Ta, Tb, band)) {
          const double d = cost_of<DMAX>(own, ycur, D4);
          const double up = sw ? own_prev : nb, left = sw ? nb : own_prev;   // (i - 1, j) and (i, j - 1)
          double best = diag;
          if (up < best) best = up, code = 1;
          if (left < best) best = left, code = 2;
          val = (s == 0 && l == 0) ? d : d + best;
        }
      }
      diag = nb;
      own_prev = val;
      ex[(dd & 1) * NT + tid] = val;
      if (hand_on && tid == NT - 1 && act) bound[l] = val;   // read by thread 0 of the next chunk; this chunk's thread 0 is THREADS - 1 cells ahead
      const u64 mask = __ballot(act);
      uint32_t bits = act ? (uint32_t)code << (2 * (lane & 15)) : 0u;
      bits |= __shfl_xor(bits, 1);
      bits |= __shfl_xor(bits, 2);
      bits |= __shfl_xor(bits, 4);
      bits |= __shfl_xor(bits, 8);
      if ((lane & 15) == 0 && ((mask >> lane) & 0xffffull)) w[pl::bp_word(c0 + dd, s, S)] = bits;
      if (act && s == S - 1 && l == L - 1) dtot[p] = val;
#pragma unroll
      for (int k = 0; k < DMAX / 4; ++k) ycur[k] = ynext[k];
      diagonal_barrier();
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);   // the same tree in every lane
  return v;
}

__global__ void __launch_bounds__(64) walk_kernel(const float* fa, const float* fb, int TA, int TB, int D4, const float* mela, const float* melb, int n_mel,
                                                  const float* f0a, const float* f0b, const PairIn* pairs, const uint32_t* bp, const double* dtot, int32_t* path,
                                                  e2ecmp_result* res, int mode, double mcd_scale) {
#pragma clang fp contract(off)
  __shared__ uint32_t cells[2 * pl::MAX_T - 1];   // the path from its end to its start
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  const PairIn pr = pairs[p];
  const int Ta = pr.Ta, Tb = pr.Tb;
  const double NaN = __longlong_as_double(0x7ff8000000000000ll);
  int N = 0;
  double total = 0.0;
  if (mode == pl::MODE_SYNC) {
    N = min(Ta, Tb);
  } else {
    total = dtot[p];
    if (!isfinite(total)) {   // uniform: no path inside the band
      if (lane == 0) {
        e2ecmp_result r;
        r.n_path = 0, r.n_voiced_both = 0, r.n_vuv_mismatch = 0, r.status = 1;
        r.dist_total = NaN, r.mcd_db = NaN, r.mel_l1 = NaN, r.f0_rmse_hz = NaN, r.f0_rmse_cents = NaN;
        res[p] = r;
      }
      return;
    }
    const bool sw = pl::swapped(Ta, Tb);
    const int S = sw ? Tb : Ta;
    const uint32_t* w = bp + pr.bp_off;
    int i = Ta - 1, j = Tb - 1;
    for (;;) {   // every lane walks the same cells; i + j falls by one or two a step, so N <= Ta + Tb - 1 whatever the words hold
      if (lane == 0) cells[N] = pl::pack_cell(i, j);
      ++N;
      if (i == 0 && j == 0) break;
      int code;
      if (i == 0) code = 2;
      else if (j == 0) code = 1;
      else {
        const int s = sw ? j : i;
        code = (int)((w[pl::bp_word(i + j, s, S)] >> pl::bp_shift(s)) & 3u);
      }
      if (code == 1) --i;
      else if (code == 2) --j;
      else --i, --j;
    }
    __syncthreads();
  }
  const float* A = fa + (size_t)p * TA * D4;
  const float* Bf = fb + (size_t)p * TB * D4;
  const bool have_mel = mela && melb, have_f0 = f0a && f0b;
  int32_t* out = path + pr.path_off * 2;
  double sd = 0.0, sl1 = 0.0, shz = 0.0, sct = 0.0, nboth = 0.0, nmis = 0.0;
  for (int n = lane; n < N; n += 64) {
    int i = n, j = n;
    if (mode != pl::MODE_SYNC) {
      const uint32_t c = cells[N - 1 - n];
      i = pl::cell_i(c), j = pl::cell_j(c);
    }
    out[2 * (size_t)n] = i;
    out[2 * (size_t)n + 1] = j;
    double acc = 0.0;
    const float* a = A + (size_t)i * D4;
    const float* b = Bf + (size_t)j * D4;
    for (int k = 0; k < D4; ++k) {
      const double d = (double)a[k] - (double)b[k];
      acc = acc + d * d;
    }
    sd += __dsqrt_rn(acc);
    if (have_mel) {
      const float* ma = mela + ((size_t)p * TA + i) * n_mel;
      const float* mb = melb + ((size_t)p * TB + j) * n_mel;
      double s = 0.0;
      for (int m = 0; m < n_mel; ++m) s += fabs((double)ma[m] - (double)mb[m]);
      sl1 += s;
    }
    if (have_f0) {
      const float x = f0a[(size_t)p * TA + i], y = f0b[(size_t)p * TB + j];
      const bool va = x > 0.f, vb = y > 0.f;
      if (va && vb) {
        const double e = (double)y - (double)x;
        const double c = 1200.0 * log2((double)y / (double)x);
        shz += e * e;
        sct += c * c;
        nboth += 1.0;
      } else if (va != vb) {
        nmis += 1.0;
      }
    }
  }
  sd = wave_sum(sd), sl1 = wave_sum(sl1), shz = wave_sum(shz), sct = wave_sum(sct), nboth = wave_sum(nboth), nmis = wave_sum(nmis);
  if (lane == 0) {
    e2ecmp_result r;
    r.n_path = N;
    r.n_voiced_both = (long long)nboth;
    r.n_vuv_mismatch = (long long)nmis;
    r.status = 0;
    r.dist_total = mode == pl::MODE_SYNC ? sd : total;
    r.mcd_db = mcd_scale * (sd / (double)N);
    r.mel_l1 = have_mel ? sl1 / ((double)N * (double)n_mel) : NaN;
    r.f0_rmse_hz = (have_f0 && nboth > 0.0) ? __dsqrt_rn(shz / nboth) : NaN;
    r.f0_rmse_cents = (have_f0 && nboth > 0.0) ? __dsqrt_rn(sct / nboth) : NaN;
    res[p] = r;
  }
}

thread_local std::string g_create_error;

struct Side {
  bool set = false, has_mel = false, has_f0 = false;
  int B = 0, T = 0, D = 0;
  std::vector<int32_t> lens;   // outlives the asynchronous copy of a call
};

}  // namespace

struct e2ecmp_handle : Handle {
  int n_mel = 0, n_cep = 0;
  pl::CepPlan cep;
  bool loaded = false, have_run = false;
  Side side[2];
  Buf basis{this, Buf::WEIGHTS};
  Buf feat_a{this}, feat_b{this}, mel_a{this}, mel_b{this}, f0_a{this}, f0_b{this}, lens_a{this}, lens_b{this};
  Buf stage{this}, pairs{this}, bp{this}, dtot{this}, path{this}, res{this};
  std::vector<PairIn> host_pairs;
  std::vector<e2ecmp_result> host_res;
  Buf& feat(int s) { return s ? feat_b : feat_a; }
  Buf& mel(int s) { return s ? mel_b : mel_a; }
  Buf& f0(int s) { return s ? f0_b : f0_a; }
  Buf& lens(int s) { return s ? lens_b : lens_a; }
};

namespace {

// the lengths of a side: fetched, checked, kept as int32
int take_lens(e2ecmp_handle* h, const int64_t* lens, int B, int T, std::vector<int32_t>& out) {
  std::vector<int64_t> l64;
  RET(fetch_host(h, lens, (size_t)B, l64));
  out.resize((size_t)B);
  for (int b = 0; b < B; ++b) {
    if (const char* m = pl::len_check(l64[b], T)) return h->fail(E2ECMP_EINVAL, std::string(m) + " (lens[" + std::to_string(b) + "] = " + std::to_string((long long)l64[b]) + ", T " + std::to_string(T) + ")");
    out[b] = (int32_t)l64[b];
  }
  return E2ECMP_OK;
}

int run(e2ecmp_handle* h, int mode, long long band, e2ecmp_result* results_out, bool zero_band_ok) {
  if (const char* m = pl::run_check(mode, band, zero_band_ok)) return h->fail(E2ECMP_EINVAL, std::string(m) + " (mode " + std::to_string(mode) + ", band " + std::to_string(band) + ")");
  const Side &sa = h->side[0], &sb = h->side[1];
  if (!sa.set || !sb.set) return h->fail(E2ECMP_ESTATE, "e2ecmp_run before both sides are set");
  if (sa.B != sb.B || sa.D != sb.D)
    return h->fail(E2ECMP_EINVAL, "the sides differ: A has B " + std::to_string(sa.B) + ", D " + std::to_string(sa.D) + "; B has B " + std::to_string(sb.B) + ", D " + std::to_string(sb.D));
  const int B = sa.B, D4 = pl::padded_d(sa.D);
  RET(begin_call(h));
  h->have_run = false;
  h->host_pairs.resize((size_t)B);
  h->host_res.resize((size_t)B);
  long long words = 0, cells = 0;
  int Lmax = 1, Smax = 1;
  for (int b = 0; b < B; ++b) {
    PairIn& q = h->host_pairs[b];
    q.Ta = sa.lens[b], q.Tb = sb.lens[b];
    q.bp_off = words, q.path_off = cells;
    words += pl::bp_words(q.Ta, q.Tb);
    cells += pl::path_cells(q.Ta, q.Tb);
    Lmax = std::max(Lmax, std::max(q.Ta, q.Tb));
    Smax = std::max(Smax, std::min(q.Ta, q.Tb));
  }
  RET(reserve(h, h->pairs, (size_t)B * sizeof(PairIn)));
  if (mode == E2ECMP_DTW) RET(reserve(h, h->bp, (size_t)words * 4));
  RET(reserve(h, h->dtot, (size_t)B * 8));
  RET(reserve(h, h->path, (size_t)cells * 8));
  RET(reserve(h, h->res, (size_t)B * sizeof(e2ecmp_result)));
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->pairs.p, h->host_pairs.data(), (size_t)B * sizeof(PairIn), hipMemcpyHostToDevice, s));
  const float* fa = (const float*)h->feat_a.p;
  const float* fb = (const float*)h->feat_b.p;
  const PairIn* pairs = (const PairIn*)h->pairs.p;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[2], s));
  if (mode == E2ECMP_DTW) {
    HIPCHK(h, hipMemsetAsync(h->dtot.p, 0xff, (size_t)B * 8, s));   // NaN until the end cell is written
    const int NT = pl::search_threads(D4, Smax);
    const size_t lds = (size_t)pl::search_lds_doubles(Lmax, NT) * 8;
    const dim3 grid((unsigned)B), block((unsigned)NT);
#define E2ECMP_SEARCH(DMAX) hipLaunchKernelGGL((search_kernel<DMAX, pl::search_threads_cap(DMAX)>), grid, block, lds, s, fa, fb, sa.T, sb.T, D4, pairs, (uint32_t*)h->bp.p, (double*)h->dtot.p, band)
    if (D4 <= 4) E2ECMP_SEARCH(4);
    else if (D4 <= 16) E2ECMP_SEARCH(16);
    else if (D4 <= 32) E2ECMP_SEARCH(32);
    else E2ECMP_SEARCH(64);
#undef E2ECMP_SEARCH
    HIPCHK(h, hipGetLastError());
  }
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[3], s));
  const bool mels = sa.has_mel && sb.has_mel, f0s = sa.has_f0 && sb.has_f0;
  const double mcd_scale = 10.0 * std::sqrt(2.0) / std::log(10.0);
  hipLaunchKernelGGL(walk_kernel, dim3((unsigned)B), dim3(64), 0, s, fa, fb, sa.T, sb.T, D4, mels ? (const float*)h->mel_a.p : nullptr,
                     mels ? (const float*)h->mel_b.p : nullptr, h->n_mel, f0s ? (const float*)h->f0_a.p : nullptr, f0s ? (const float*)h->f0_b.p : nullptr, pairs,
                     (const uint32_t*)h->bp.p, (const double*)h->dtot.p, (int32_t*)h->path.p, (e2ecmp_result*)h->res.p, mode, mcd_scale);
  HIPCHK(h, hipGetLastError());
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[4], s));
  HIPCHK(h, hipMemcpyAsync(h->host_res.data(), h->res.p, (size_t)B * sizeof(e2ecmp_result), hipMemcpyDeviceToHost, s));
  RET(copy_out(h, results_out, h->res.p, (size_t)B * sizeof(e2ecmp_result)));
  HIPCHK(h, hipStreamSynchronize(s));
  h->unfinished = false;
  if (h->profile) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    h->last_ms[1] = ms;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[3], h->ev[4]));
    h->last_ms[2] = ms;
  }
  h->have_run = true;
  return E2ECMP_OK;
}

}  // namespace

extern "C" {

const char* e2ecmp_version(void) { return "e2etts-compare 1 E2ECMP_SRC_HASH=" E2ECMP_SRC_HASH; }
int e2ecmp_abi_version(void) { return E2ECMP_ABI_VERSION; }

const char* e2ecmp_last_error(const e2ecmp_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int e2ecmp_create(int device_id, int n_mel, int n_cep, e2ecmp_handle** out) {
  if (!out) {
    g_create_error = "e2ecmp_create: out is NULL";
    return E2ECMP_EINVAL;
  }
  *out = nullptr;
  if (device_id < 0) {
    g_create_error = "e2ecmp_create: device_id must not be negative";
    return E2ECMP_EINVAL;
  }
  pl::CepPlan cp;
  if (const char* m = pl::cep_plan(n_mel, n_cep, &cp)) {
    g_create_error = std::string("e2ecmp_create: ") + m + " (got n_mel " + std::to_string(n_mel) + ", n_cep " + std::to_string(n_cep) + ")";
    return E2ECMP_EINVAL;
  }
  e2ecmp_handle* h = new (std::nothrow) e2ecmp_handle();
  if (!h) {
    g_create_error = "out of host memory";
    return E2ECMP_ENOMEM;
  }
  h->device = device_id;
  h->n_mel = n_mel;
  h->n_cep = n_cep;
  h->cep = cp;
  *out = h;
  return E2ECMP_OK;
}

void e2ecmp_destroy(e2ecmp_handle* h) { companion::destroy(h); }

int e2ecmp_load(e2ecmp_handle* h, const float* basis) {
  if (!h) return E2ECMP_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!basis) return h->fail(E2ECMP_EINVAL, "basis must not be NULL");
  const size_t n = (size_t)h->n_cep * h->n_mel;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(basis[i])) return h->fail(E2ECMP_EINVAL, "basis[" + std::to_string(i) + "] is not finite");
  RET(open_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // nothing reads the old basis
  RET(reserve(h, h->basis, n * 4));
  HIPCHK(h, hipMemcpy(h->basis.p, basis, n * 4, hipMemcpyHostToDevice));
  h->loaded = true;
  return E2ECMP_OK;
}

void* e2ecmp_stream(e2ecmp_handle* h) { return companion::stream(h); }
int e2ecmp_order_after(e2ecmp_handle* h, void* caller_stream) { return companion::order_after(h, caller_stream); }
int e2ecmp_sync(e2ecmp_handle* h) { return companion::sync(h); }
size_t e2ecmp_device_bytes(const e2ecmp_handle* h) { return companion::device_bytes(h); }

int e2ecmp_set_mels(e2ecmp_handle* h, int side, const float* mel, const float* f0, const int64_t* lens, int B, int T) {
  if (!h) return E2ECMP_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (const char* m = pl::side_check(side, B, T, h->n_cep)) return h->fail(E2ECMP_EINVAL, std::string(m) + " (side " + std::to_string(side) + ", B " + std::to_string(B) + ", T " + std::to_string(T) + ")");
  if (!mel || !lens) return h->fail(E2ECMP_EINVAL, "mel and lens must not be NULL");
  if ((uintptr_t)mel % 4 || (uintptr_t)f0 % 4) return h->fail(E2ECMP_EINVAL, "mel and f0 must be aligned to 4 bytes");
  if (!h->loaded) return h->fail(E2ECMP_ESTATE, "e2ecmp_set_mels before e2ecmp_load");
  std::vector<int32_t> l32;
  RET(take_lens(h, lens, B, T, l32));
  RET(begin_call(h));
  Side& sd = h->side[side];
  sd.set = false;
  h->have_run = false;
  sd.lens.swap(l32);
  const int D4 = pl::padded_d(h->n_cep);
  const size_t frames = (size_t)B * T;
  RET(reserve(h, h->feat(side), frames * D4 * 4));
  RET(reserve(h, h->mel(side), frames * h->n_mel * 4));
  if (f0) RET(reserve(h, h->f0(side), frames * 4));
  RET(reserve(h, h->lens(side), (size_t)B * 4));
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->lens(side).p, sd.lens.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->mel(side).p, mel, frames * h->n_mel * 4, hipMemcpyDefault, s));
  if (f0) HIPCHK(h, hipMemcpyAsync(h->f0(side).p, f0, frames * 4, hipMemcpyDefault, s));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[0], s));
  const dim3 grid((unsigned)pl::ceil_div(T, h->cep.tile), (unsigned)B);
  hipLaunchKernelGGL(cepstra_kernel, grid, dim3(pl::THREADS), (size_t)h->cep.lds_floats * 4, s, (const float*)h->mel(side).p, (const int*)h->lens(side).p,
                     (const float*)h->basis.p, (float*)h->feat(side).p, T, h->n_mel, h->n_cep, D4, h->cep.stride, h->cep.tile, h->n_mel % 4 == 0 ? 1 : 0);
  HIPCHK(h, hipGetLastError());
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[1], s));
  HIPCHK(h, hipStreamSynchronize(s));
  h->unfinished = false;
  if (h->profile) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->last_ms[0] = ms;
  }
  sd.B = B, sd.T = T, sd.D = h->n_cep;
  sd.has_mel = true, sd.has_f0 = f0 != nullptr;
  sd.set = true;
  return E2ECMP_OK;
}

int e2ecmp_set_features(e2ecmp_handle* h, int side, const float* features, const int64_t* lens, int B, int T, int D) {
  if (!h) return E2ECMP_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (const char* m = pl::side_check(side, B, T, D))
    return h->fail(E2ECMP_EINVAL, std::string(m) + " (side " + std::to_string(side) + ", B " + std::to_string(B) + ", T " + std::to_string(T) + ", D " + std::to_string(D) + ")");
  if (!features || !lens) return h->fail(E2ECMP_EINVAL, "features and lens must not be NULL");
  if ((uintptr_t)features % 4) return h->fail(E2ECMP_EINVAL, "features must be aligned to 4 bytes");
  std::vector<int32_t> l32;
  RET(take_lens(h, lens, B, T, l32));
  RET(begin_call(h));
  Side& sd = h->side[side];
  sd.set = false;
  h->have_run = false;
  sd.lens.swap(l32);
  const int D4 = pl::padded_d(D);
  const size_t frames = (size_t)B * T;
  RET(reserve(h, h->feat(side), frames * D4 * 4));
  RET(reserve(h, h->lens(side), (size_t)B * 4));
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->lens(side).p, sd.lens.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
  const float* src = features;
  if (!is_device_pointer(features)) {
    RET(reserve(h, h->stage, frames * D * 4));
    HIPCHK(h, hipMemcpyAsync(h->stage.p, features, frames * D * 4, hipMemcpyHostToDevice, s));
    src = (const float*)h->stage.p;
  }
  const size_t total = frames * D4;
  hipLaunchKernelGGL(pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, (const int*)h->lens(side).p, (float*)h->feat(side).p, T, D, D4, total);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(s));
  h->unfinished = false;
  sd.B = B, sd.T = T, sd.D = D;
  sd.has_mel = false, sd.has_f0 = false;
  sd.set = true;
  return E2ECMP_OK;
}

int e2ecmp_fetch_features(e2ecmp_handle* h, int side, float* out) {
  if (!h) return E2ECMP_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (side != E2ECMP_A && side != E2ECMP_B) return h->fail(E2ECMP_EINVAL, "side must be E2ECMP_A or E2ECMP_B");
  if (!out) return h->fail(E2ECMP_EINVAL, "out must not be NULL");
  const Side& sd = h->side[side];
  if (!sd.set) return h->fail(E2ECMP_ESTATE, "e2ecmp_fetch_features of a side that is not set");
  const int D4 = pl::padded_d(sd.D);
  const size_t frames = (size_t)sd.B * sd.T;
  HIPCHK(h, hipSetDevice(h->device));
  if (D4 == sd.D) HIPCHK(h, hipMemcpyAsync(out, h->feat(side).p, frames * D4 * 4, hipMemcpyDefault, h->stream));
  else HIPCHK(h, hipMemcpy2DAsync(out, (size_t)sd.D * 4, h->feat(side).p, (size_t)D4 * 4, (size_t)sd.D * 4, frames, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return E2ECMP_OK;
}

int e2ecmp_run(e2ecmp_handle* h, int mode, long long band, e2ecmp_result* results_out) {
  if (!h) return E2ECMP_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  return run(h, mode, band, results_out, false);
}

int e2ecmp_fetch_path(e2ecmp_handle* h, int b, int32_t* out, long long capacity, long long* n_out) {
  if (!h) return E2ECMP_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->have_run) return h->fail(E2ECMP_ESTATE, "e2ecmp_fetch_path without a completed run");
  if (b < 0 || b >= (int)h->host_res.size()) return h->fail(E2ECMP_EINVAL, "b must lie in [0, B)");
  const long long n = (long long)h->host_res[b].n_path;
  if (n_out) *n_out = n;
  if (!out || !n) return E2ECMP_OK;
  if (capacity < n) return h->fail(E2ECMP_EINVAL, "capacity " + std::to_string(capacity) + " < n_path " + std::to_string(n));
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(out, (const int32_t*)h->path.p + h->host_pairs[b].path_off * 2, (size_t)n * 8, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return E2ECMP_OK;
}

int e2ecmp_profile_enable(e2ecmp_handle* h, int on) { return companion::profile_enable(h, on); }
int e2ecmp_profile_read(e2ecmp_handle* h, double ms_out[3]) { return companion::profile_read(h, ms_out); }

#ifdef E2ECMP_TEST_HOOKS
int e2ecmp_debug_poison_workspace(e2ecmp_handle* h) {
  if (!h) return E2ECMP_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(poison_workspaces(h));
  h->unfinished = false;
  h->side[0].set = h->side[1].set = false;
  h->have_run = false;
  return E2ECMP_OK;
}

int e2ecmp_debug_run(e2ecmp_handle* h, int mode, long long band, e2ecmp_result* results_out) {
  if (!h) return E2ECMP_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  return run(h, mode, band, results_out, true);
}
#endif

}  // extern "C"
