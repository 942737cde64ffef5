// libe2etts_critic.so: the eval() forward of HiFi-GAN's multi-period and multi-scale discriminators and the figures of the reference's
// V/loss.py on their outputs, behind the C ABI of include/e2etts_critic.h (the definition is there).  A companion of libe2etts_hip.so:
// its dense layers run on that library's exact-fp32 launch_conv_gemm, everything else is here.  All exact fp32, figures in double.
//
// Layout.  A discriminator's sequences are its rows' columns: period p makes p sequences of a row (the folded signal's columns), a scale
// discriminator one.  Activations are channels-last [sequence, rows, C], `rows` (plan.h: launch_rows) the same for every sequence of a
// call; a layer writes zeros from a sequence's own length to `rows`, which is what lets the next dense layer view that buffer as
// [rows / s, s * C] (the stride fold) and conv_gemm's zero padding stand for the row's own end.
//
// Kernels:
//   first     Cin = 1: one thread per (sequence, position, channel), one chain over the taps, summed in double and rounded once.  For a period discriminator the
//             reflect extension and the fold are the index it reads the signal at; nothing is materialised.
//   grouped   v_mfma_f32_32x32x2_f32.  A workgroup takes TM positions of one group of one sequence and stages the input window once into
//             LDS, channel-major and de-interleaved by the stride's phase ([c][r % s][r / s]): for a tap the 32 positions of an MFMA's A
//             fragment are consecutive floats whatever the stride.  A wavefront owns units of 64 positions x 32 output channels (two
//             accumulator tiles sharing every B fragment) and walks tap-major, channel pairs ascending, tap j into accumulator j % 4 of
//             four that a fixed tree merges: the order of terms per element is fixed and independent of TM.  B fragments come straight from global memory in the packer's fragment order (one 256-byte
//             load per MFMA pair).  Bias, leaky ReLU and the zero rows go in the epilogue.
//   post      Cout = 1: one wavefront per position, lanes stride the channels, a fixed xor tree merges them; in double, rounded once.
//   pool      AvgPool1d(4, 2, padding 2) over a row's own length.
//   reduce    |r - g| and the score moments: per chunk of 4096 values the lanes' partial sums in double and a fixed tree in LDS; a
//             second launch merges the chunks by the same tree.  No atomics.
//   layout    a resident map to the reference's [B, C, T, p] for e2ecr_fetch_fmap / e2ecr_fetch_scores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../../include/e2etts_critic.h"
#ifdef E2ECR_TEST_HOOKS
#define E2E_COMPANION_TEST_HOOKS
#endif
#include "../companion/handle.h"
#include "../host_logic.h"
#include "../kernels.h"
#include "plan.h"

#ifndef E2ECR_SRC_HASH
#define E2ECR_SRC_HASH "unknown"
#endif

using namespace e2etts;
using namespace e2etts::companion;
namespace pl = e2ecr_plan;

static_assert(E2ECR_OK == E_OK && E2ECR_EINVAL == E_INVAL && E2ECR_EHIP == E_HIP && E2ECR_ESTATE == E_STATE && E2ECR_ENOMEM == E_NOMEM,
              "include/e2etts_critic.h and csrc/companion/handle.h disagree on the error codes");
static_assert(E2ECR_MAX_B == pl::MAX_B && E2ECR_MAX_LEN == pl::MAX_LEN && E2ECR_MAX_PERIODS == pl::MAX_PERIODS && E2ECR_MAX_SCALES == pl::MAX_SCALES &&
                  E2ECR_MAX_LAYERS == pl::MAX_LAYERS && E2ECR_MAX_DISC == pl::MAX_DISC && E2ECR_MAX_MAPS == pl::MAX_MAPS,
              "include/e2etts_critic.h and csrc/critic/plan.h disagree on the limits");
static_assert(pl::RED_THREADS == 256 && pl::RED_PER_LANE == 16, "the reduction kernels are written for these");
static_assert(sizeof(e2ecr_layer) == 20 && sizeof(e2ecr_config) == 4 + 32 + 4 + 160 + 20 + 4 + 4 + 160 + 20 + 4 + 4 + 8, "e2ecr_config is int32 / float words and one int64");
static_assert(sizeof(e2ecr_result) == 16 + 8 * (E2ECR_MAX_DISC * E2ECR_MAX_MAPS + 3 * E2ECR_MAX_DISC + 6), "e2ecr_result is two int64 and doubles");

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(256) pcm_to_f32_kernel(const int16_t* src, float* dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (float)src[i] * (1.0f / 32768.0f);
}

// out[row, t] = (((x[2t - 2] + x[2t - 1]) + x[2t]) + x[2t + 1]) * 0.25, summed in double and rounded once, over the row's own n_in[row]
// samples; zeros from pool_len(n) on
__global__ void __launch_bounds__(256) pool_kernel(const float* in, long long in_ld, const int32_t* n_in, float* out, long long out_ld, int R) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)R * out_ld) return;
  const int row = (int)(idx / out_ld);
  const long long t = idx - (long long)row * out_ld;
  const long long n = n_in[row];
  float v = 0.f;
  if (t < pl::pool_len(n)) {
    const float* x = in + (long long)row * in_ld;
    auto at = [&](long long i) { return (i >= 0 && i < n) ? x[i] : 0.f; };
    v = (float)(((((double)at(2 * t - 2) + (double)at(2 * t - 1)) + (double)at(2 * t)) + (double)at(2 * t + 1)) * 0.25);   // one rounding
  }
  out[idx] = v;
}

struct FirstArgs {
  const float* sig;        // [rows, ld]
  long long ld;
  const int32_t* n_sig;    // [rows] samples of the row's signal
  const float* w;          // [Cout, k]
  const float* bias;
  float* out;              // [rows * cols, rows_l, Cout]
  const int32_t* lens_out; // [rows * cols]
  int cols, rows_l, Cout, k, stride, pad;
  float slope;
  long long total;
};

__global__ void __launch_bounds__(256) first_conv_kernel(FirstArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.total) return;
  const int c = (int)(idx % a.Cout);
  const long long st = idx / a.Cout;
  const int t = (int)(st % a.rows_l);
  const int seq = (int)(st / a.rows_l);
  float v = 0.f;
  if (t < a.lens_out[seq]) {
    const int row = seq / a.cols, col = seq - row * a.cols;
    const long long n = a.n_sig[row];
    const long long H = pl::period_rows(n, a.cols);
    const float* x = a.sig + (long long)row * a.ld;
    const float* w = a.w + (long long)c * a.k;
    double acc = 0.0;   // a product of two floats is exact in double: the chain rounds only its sums, and the result once
    for (int j = 0; j < a.k; ++j) {
      const long long h = (long long)t * a.stride - a.pad + j;
      if (h >= 0 && h < H) acc += (double)w[j] * (double)x[pl::reflect_index(h * a.cols + col, n)];
    }
    v = (float)(acc + (double)a.bias[c]);
    v = fmaxf(v, v * a.slope);
  }
  a.out[idx] = v;
}

struct GroupArgs {
  const float* in;          // [NS, t_in_cap, cin]
  const int32_t* lens_in;   // [NS]
  const float* wfrag;
  const float* bias;
  float* out;               // [NS, t_out_cap, cout]
  int NS, t_in_cap, t_out_cap, cin, cout, k, stride, groups, pad, tiles;
  float slope;
  pl::GroupPlan gp;
};

__global__ void __launch_bounds__(256) grouped_conv_kernel(GroupArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_g[];
  const pl::GroupPlan gp = a.gp;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  int bid = blockIdx.x;
  const int tile = bid % a.tiles;
  bid /= a.tiles;
  const int g = bid % a.groups, seq = bid / a.groups;
  if (seq >= a.NS) return;
  const int t0 = tile * gp.tm;
  const int len_in = min(max(a.lens_in[seq], 0), a.t_in_cap);
  const int len_out = (int)min(pl::out_len(len_in, a.k, a.stride, a.pad), (int64_t)a.t_out_cap);
  float* outp = a.out + ((long long)seq * a.t_out_cap) * a.cout + (long long)g * gp.cout_g;
  const int t_end = min(t0 + gp.tm, a.t_out_cap);
  if (t0 >= len_out) {   // uniform: a tile past the sequence's end only writes its zero rows
    for (int idx = tid; idx < (t_end - t0) * gp.cout_g; idx += nthr) {
      const int r = idx / gp.cout_g, c = idx - r * gp.cout_g;
      outp[(long long)(t0 + r) * a.cout + c] = 0.f;
    }
    return;
  }
  // the window: rows t0 s - pad .. + (tm - 1) s + k - 1 of this group's channels, zeros outside the sequence
  const int wr = (gp.tm - 1) * a.stride + a.k;
  const long long r0 = (long long)t0 * a.stride - a.pad;
  const float* inp = a.in + ((long long)seq * a.t_in_cap) * a.cin + (long long)g * gp.cin_g;
  for (int idx = tid; idx < wr * gp.cin_g; idx += nthr) {
    const int r = idx / gp.cin_g, c = idx - r * gp.cin_g;
    const long long row = r0 + r;
    const float v = (row >= 0 && row < len_in) ? inp[row * a.cin + c] : 0.f;
    lds_g[pl::group_lds_index(gp, a.stride, r, c)] = v;
  }
  __syncthreads();
  const int mp_n = gp.tm / 64, units = mp_n * gp.ntp, half = gp.cin_g / 2;
  const int li = lane & 31, lh = lane >> 5;
  for (int u = wave; u < units; u += nw) {   // uniform per wavefront
    const int mp = u % mp_n, nt = u / mp_n;
    // four accumulators per tile, tap j into accumulator j % 4: chains a quarter as long, merged below by the tree (a0 + a1) + (a2 + a3)
    f32x16 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;
    const float* wf = a.wfrag + ((long long)(g * gp.ntp + nt) * a.k * half) * 64 + lane;
    for (int j0 = 0; j0 < a.k; j0 += 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = j0 + q;
        if (j < a.k) {   // uniform
          const int base = (j % a.stride) * gp.prow + j / a.stride + mp * 64 + li + lh * gp.cstride;
          const float* wj = wf + (long long)j * half * 64;
#pragma unroll 4
          for (int c2 = 0; c2 < half; ++c2) {
            const float b = wj[c2 * 64];
            const float* ap = lds_g + 2 * c2 * gp.cstride + base;
            acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[0], b, acc[0][q], 0, 0, 0);
            acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[32], b, acc[1][q], 0, 0, 0);
          }
        }
      }
    }
    const f32x16 acc0 = (acc[0][0] + acc[0][1]) + (acc[0][2] + acc[0][3]);
    const f32x16 acc1 = (acc[1][0] + acc[1][1]) + (acc[1][2] + acc[1][3]);
    // C layout of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int n = nt * 32 + li;
    if (n < gp.cout_g) {
      const float bv = a.bias[g * gp.cout_g + n];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int t = t0 + mp * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (t < t_end) {
            float v = (m ? acc1[r] : acc0[r]) + bv;
            v = fmaxf(v, v * a.slope);
            outp[(long long)t * a.cout + n] = t < len_out ? v : 0.f;
          }
        }
    }
  }
}

// out = leaky(tree(partials) + bias) on rows that exist, 0 past a sequence's length; the tree is plan.h's: pairs, then pairs of pairs
struct MergeSplitArgs {
  const float* part;        // [splits][NS, rows, C]
  long long split_stride;   // NS * rows * C
  const float* bias;
  const int32_t* lens;      // [NS]
  float* out;               // [NS, rows, C]
  int splits, rows, C;
  float slope;
  long long total;
};

__global__ void __launch_bounds__(256) merge_splits_kernel(MergeSplitArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.total) return;
  const int c = (int)(idx % a.C);
  const long long st = idx / a.C;
  const int t = (int)(st % a.rows), seq = (int)(st / a.rows);
  float v = 0.f;
  if (t < a.lens[seq]) {
    float p[pl::MAX_SPLITS];
#pragma unroll
    for (int i = 0; i < pl::MAX_SPLITS; ++i) p[i] = i < a.splits ? a.part[(long long)i * a.split_stride + idx] : 0.f;
    if (a.splits == 2) v = p[0] + p[1];
    else if (a.splits == 4) v = (p[0] + p[1]) + (p[2] + p[3]);
    else v = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
    v += a.bias[c];
    v = fmaxf(v, v * a.slope);
  }
  a.out[idx] = v;
}

struct PostArgs {
  const float* in;          // [NS, rows_in, C]
  const int32_t* lens_in;
  const int32_t* lens_out;
  const float* w;           // [k, C]
  const float* bias;        // [1]
  float* out;               // [NS, rows_l]
  int NS, rows_in, rows_l, C, k, pad;
};

__global__ void __launch_bounds__(256) post_conv_kernel(PostArgs a) {
  const long long gw = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (gw >= (long long)a.NS * a.rows_l) return;   // uniform per wavefront
  const int t = (int)(gw % a.rows_l), seq = (int)(gw / a.rows_l);
  const int len_in = min(a.lens_in[seq], a.rows_in);
  double acc = 0.0;   // in double: the score is a sum of 3 C terms that largely cancel
  const bool live = t < a.lens_out[seq];
  if (live) {
    const float* x = a.in + (long long)seq * a.rows_in * a.C;
    for (int j = 0; j < a.k; ++j) {
      const int r = t - a.pad + j;
      if (r < 0 || r >= len_in) continue;
      for (int c = lane; c < a.C; c += 64) acc += (double)a.w[j * a.C + c] * (double)x[(long long)r * a.C + c];
    }
  }
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) a.out[gw] = live ? (float)(acc + (double)a.bias[0]) : 0.f;
}

__device__ __forceinline__ double block_tree(double* v, int tid) {
  for (int s = 128; s >= 1; s >>= 1) {
    __syncthreads();
    if (tid < s) v[tid] += v[tid + s];
  }
  __syncthreads();
  return v[0];
}

struct RedArgs {
  const float* a;           // [NS, rows_l, C]
  long long seq_stride;     // rows_l * C
  const int32_t* lens;      // [NS] lengths of this map
  int cols, C, chunks_max;
  int mode;                 // 0: |r - g| of pair u = sequences of rows 2u and 2u + 1; 1: (1 - v)^2 and v^2 of row u
  double* partial;          // [units, chunks_max, 2]
};

__global__ void __launch_bounds__(256) reduce_chunks_kernel(RedArgs q) {
#pragma clang fp contract(off)
  __shared__ double v0[256], v1[256];
  const int tid = threadIdx.x, u = blockIdx.y, chunk = blockIdx.x;
  const int sa = (q.mode == 0 ? 2 * u : u) * q.cols, sb = sa + q.cols;
  int len = q.lens[sa];
  if (q.mode == 0) len = min(len, q.lens[sb]);
  const long long per = (long long)len * q.C, N = per * q.cols;
  if ((long long)chunk * pl::RED_CHUNK >= N) return;   // uniform
  double s0 = 0.0, s1 = 0.0;
  for (int i = 0; i < pl::RED_PER_LANE; ++i) {
    const long long e = (long long)chunk * pl::RED_CHUNK + (long long)i * 256 + tid;
    if (e >= N) break;
    const long long col = e / per, off = e - col * per;
    const double x = (double)q.a[(sa + col) * q.seq_stride + off];
    if (q.mode == 0) {
      const double y = (double)q.a[(sb + col) * q.seq_stride + off];
      s0 = s0 + fabs(x - y);
    } else {
      const double d = 1.0 - x;
      s0 = s0 + d * d;
      s1 = s1 + x * x;
    }
  }
  v0[tid] = s0;
  v1[tid] = s1;
  const double r0 = block_tree(v0, tid), r1 = block_tree(v1, tid);
  if (tid == 0) {
    double* p = q.partial + ((long long)u * q.chunks_max + chunk) * 2;
    p[0] = r0;
    p[1] = r1;
  }
}

struct MergeArgs {
  const double* partial;
  const int32_t* lens;
  int cols, C, chunks_max, mode;
  double* out;              // unit u writes out[u * out_stride] (and [+ 1] in mode 1)
  long long out_stride;
};

__global__ void __launch_bounds__(256) reduce_merge_kernel(MergeArgs q) {
#pragma clang fp contract(off)
  __shared__ double v0[256], v1[256];
  const int tid = threadIdx.x, u = blockIdx.x;
  const int sa = (q.mode == 0 ? 2 * u : u) * q.cols, sb = sa + q.cols;
  int len = q.lens[sa];
  if (q.mode == 0) len = min(len, q.lens[sb]);
  const long long N = (long long)len * q.C * q.cols;
  const long long nch = pl::red_chunks(N);
  double s0 = 0.0, s1 = 0.0;
  if (N > 0)
    for (long long c = tid; c < nch; c += 256) {
      const double* p = q.partial + ((long long)u * q.chunks_max + c) * 2;
      s0 = s0 + p[0];
      s1 = s1 + p[1];
    }
  v0[tid] = s0;
  v1[tid] = s1;
  const double r0 = block_tree(v0, tid), r1 = block_tree(v1, tid);
  if (tid == 0) {
    const double NaN = __longlong_as_double(0x7ff8000000000000ll);
    double* o = q.out + (long long)u * q.out_stride;
    o[0] = N > 0 ? r0 / (double)N : NaN;
    if (q.mode == 1) o[1] = N > 0 ? r1 / (double)N : NaN;
  }
}

// in [B * cols, rows_l, C] -> out [B, C, Tmax, cols], zeros at t >= lens[sequence]
__global__ void __launch_bounds__(256) layout_kernel(const float* in, const int32_t* lens, float* out, int cols, int rows_l, int C, int Tmax, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int col = (int)(idx % cols);
  long long r = idx / cols;
  const int t = (int)(r % Tmax);
  r /= Tmax;
  const int c = (int)(r % C);
  const long long b = r / C;
  const long long seq = b * cols + col;
  out[idx] = t < lens[seq] ? in[(seq * rows_l + t) * C + c] : 0.f;
}

thread_local std::string g_create_error;

struct Want {
  std::string name;
  size_t numel;
  const float** dst;
};

constexpr int FM_SLOTS = pl::MAX_DISC * pl::MAX_MAPS;   // doubles per pair
constexpr int MOM_SLOTS = pl::MAX_DISC * 2;             // doubles per row

}  // namespace

struct e2ecr_handle : Handle {
  e2ecr_config cfg;
  std::vector<pl::Disc> disc;
  int min_len = 2;
  bool loaded = false;
  const float* w[pl::MAX_DISC][pl::MAX_MAPS] = {};
  const float* b[pl::MAX_DISC][pl::MAX_MAPS] = {};
  Buf blob{this, Buf::WEIGHTS};
  Buf raw{this}, sig{this}, pooled{this}, lens_dev{this}, buf_a{this}, buf_b{this}, part{this}, maps{this}, scores{this}, partial{this}, figs{this}, stage{this};
  // the geometry of the last computing call (what the fetch entry points read)
  int have = 0;   // 0 nothing, 1 a run, 2 a forward
  int R = 0, B = 0;
  bool paired = false;
  long long ld = 0;
  std::vector<int64_t> n_row;                 // [R] samples per row (row 2 b = y_b, 2 b + 1 = g_b for a paired run)
  std::vector<int32_t> host_lens;             // every lengths table of the call, as uploaded
  std::vector<double> host_figs;
  long long rows_l[pl::MAX_DISC][pl::MAX_MAPS] = {};
  long long lens_off[pl::MAX_DISC][pl::MAX_MAPS + 1] = {};   // level 0: the discriminator's input, 1 + l: after layer l
  long long nsig_off[pl::MAX_SCALES] = {};
  long long sig_ld[pl::MAX_SCALES] = {};
  long long sig_off[pl::MAX_SCALES] = {};     // floats into `pooled` (scale >= 1)
  long long maps_off[pl::MAX_DISC][pl::MAX_MAPS] = {};
  long long score_off[pl::MAX_DISC] = {};
  std::vector<hipEvent_t> pev;
  std::vector<int> pcls;
  size_t pev_used = 0;
  ~e2ecr_handle() {
    for (auto e : pev) (void)hipEventDestroy(e);
  }
};

namespace {

int build_discs(const e2ecr_config& c, std::vector<pl::Disc>& out, int* min_len, std::string& why) {
  auto bad = [&](const std::string& m) {
    why = m;
    return E2ECR_EINVAL;
  };
  if (c.n_periods < 0 || c.n_periods > pl::MAX_PERIODS || c.n_scales < 0 || c.n_scales > pl::MAX_SCALES || c.n_periods + c.n_scales < 1)
    return bad("n_periods in [0, 8], n_scales in [0, 4], at least one discriminator");
  if (!(c.slope >= 0.f && c.slope <= 1.f)) return bad("slope must lie in [0, 1]");
  if (c.workspace_cap_bytes < 0) return bad("workspace_cap_bytes must not be negative");
  int pmax = 1;
  auto table = [&](const e2ecr_layer* t, int n, const e2ecr_layer& post, pl::Disc& d, const char* what) -> int {
    if (n < 1 || n > pl::MAX_LAYERS) return bad(std::string(what) + ": 1 to 8 layers before the post layer");
    d.n_layers = n;
    int cin = 1;
    for (int l = 0; l <= n; ++l) {
      const e2ecr_layer& s = l < n ? t[l] : post;
      const pl::LayerSpec sp{s.cout, s.k, s.stride, s.groups, s.pad};
      if (const char* m = pl::layer_plan(sp, cin, l == 0, l == n, &d.layer[l]))
        return bad(std::string(what) + (l < n ? " layer " + std::to_string(l) : std::string(" post layer")) + ": " + m);
      cin = s.cout;
    }
    return E2ECR_OK;
  };
  out.clear();
  for (int i = 0; i < c.n_periods; ++i) {
    if (c.periods[i] < 1 || c.periods[i] > pl::MAX_PERIOD) return bad("periods must lie in [1, 64]");
    pl::Disc d;
    d.period = c.periods[i];
    pmax = std::max(pmax, d.period);
    RET(table(c.mpd, c.n_mpd_layers, c.mpd_post, d, "period discriminator"));
    out.push_back(d);
  }
  for (int i = 0; i < c.n_scales; ++i) {
    pl::Disc d;
    d.scale = i;
    RET(table(c.msd, c.n_msd_layers, c.msd_post, d, "scale discriminator"));
    out.push_back(d);
  }
  *min_len = pmax + 1;
  return E2ECR_OK;
}

std::string wname(int d, int l, const char* what) { return "d" + std::to_string(d) + ".l" + std::to_string(l) + "." + what; }

size_t weight_numel(const pl::Layer& L) {
  switch (L.kind) {
    case pl::FIRST: return (size_t)L.cout * L.k;
    case pl::DENSE: return (size_t)L.cout * L.fold.kf * L.stride * L.cin;
    case pl::GROUPED: return (size_t)pl::group_frag_floats(L.cin, L.cout, L.k, L.groups);
    default: return (size_t)L.k * L.cin;
  }
}

// profiling: one pair of events around every launch, tagged with its class (0 dense, 1 grouped, 2 the rest)
int prof_mark(e2ecr_handle* h, int cls) {
  if (!h->profile) return E2ECR_OK;
  if (h->pev_used == h->pev.size()) {
    hipEvent_t e;
    HIPCHK(h, hipEventCreate(&e));
    h->pev.push_back(e);
    h->pcls.push_back(0);
  }
  h->pcls[h->pev_used] = cls;
  HIPCHK(h, hipEventRecord(h->pev[h->pev_used++], h->stream));
  return E2ECR_OK;
}

int launch_grouped(e2ecr_handle* h, GroupArgs a) {
  const long long blocks = (long long)a.tiles * a.groups * a.NS;
  if (blocks < 1 || blocks >= (1LL << 31)) return h->fail(E2ECR_EINVAL, "grouped layer: the launch would have " + std::to_string(blocks) + " workgroups");
  hipLaunchKernelGGL(grouped_conv_kernel, dim3((unsigned)blocks), dim3((unsigned)(64 * a.gp.waves)), (size_t)a.gp.lds_floats * 4, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return E2ECR_OK;
}

// One discriminator over the sequences of rows [row0, row0 + nrows): layer l writes to out_of(l); figures when `fused`.
int run_disc(e2ecr_handle* h, int di, int row0, int nrows, bool keep) {
  const pl::Disc& d = h->disc[di];
  const int cols = pl::disc_cols(d), NS = nrows * cols;
  const int32_t* L = (const int32_t*)h->lens_dev.p;
  auto lens_at = [&](int level) { return L + h->lens_off[di][level] + (long long)row0 * cols; };
  hipStream_t s = h->stream;
  const float* in = nullptr;
  long long rows_in = 0;
  for (int l = 0; l <= d.n_layers; ++l) {
    const pl::Layer& Ly = d.layer[l];
    const long long rows = h->rows_l[di][l];
    float* out;
    if (l == d.n_layers) out = (float*)h->scores.p + h->score_off[di] + (long long)row0 * cols * rows;
    else if (keep) out = (float*)h->maps.p + h->maps_off[di][l];
    else out = (float*)((l & 1) ? h->buf_b.p : h->buf_a.p);
    if (Ly.kind == pl::FIRST) {
      FirstArgs a;
      const int sc = d.scale;
      a.sig = (sc == 0 ? (const float*)h->sig.p : (const float*)h->pooled.p + h->sig_off[sc]) + (long long)row0 * h->sig_ld[sc];
      a.ld = h->sig_ld[sc];
      a.n_sig = L + h->nsig_off[sc] + row0;
      a.w = h->w[di][l], a.bias = h->b[di][l], a.out = out, a.lens_out = lens_at(1);
      a.cols = cols, a.rows_l = (int)rows, a.Cout = Ly.cout, a.k = Ly.k, a.stride = Ly.stride, a.pad = Ly.pad, a.slope = h->cfg.slope;
      a.total = (long long)NS * rows * Ly.cout;
      RET(prof_mark(h, 2));
      hipLaunchKernelGGL(first_conv_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, a);
      HIPCHK(h, hipGetLastError());
      RET(prof_mark(h, 2));
    } else if (Ly.kind == pl::DENSE) {
      ConvParams p;
      p.in = in, p.w = h->w[di][l], p.bias = h->b[di][l], p.out = out, p.lens = lens_at(1 + l);
      p.B = NS, p.T = (int)rows, p.Cin = Ly.stride * Ly.cin, p.Cout = Ly.cout, p.KW = Ly.fold.kf, p.dil = 1, p.pad = Ly.fold.q;
      p.in_bs = rows_in * Ly.cin, p.out_bs = rows * Ly.cout, p.in_ld = Ly.stride * Ly.cin, p.out_ld = Ly.cout;
      p.act = ACT_LRELU, p.act_slope = h->cfg.slope;
      RET(prof_mark(h, 0));
      if (Ly.splits < 2) {
        KCHK(h, launch_conv_gemm(p, s));
      } else {
        // the K split (plan.h: dense_splits): one launch per range of the folded channel axis into a partial buffer of its own -- the
        // packer laid the weights out range by range --, then the fixed tree, the bias and the activation
        const int cw = p.Cin / Ly.splits;
        MergeSplitArgs m;
        m.part = (const float*)h->part.p, m.split_stride = (long long)NS * rows * Ly.cout, m.bias = h->b[di][l], m.lens = p.lens, m.out = out;
        m.splits = Ly.splits, m.rows = (int)rows, m.C = Ly.cout, m.slope = h->cfg.slope, m.total = m.split_stride;
        p.bias = nullptr, p.act = ACT_NONE, p.Cin = cw;
        for (int i = 0; i < Ly.splits; ++i) {
          p.in = in + (long long)i * cw;
          p.w = h->w[di][l] + (long long)i * Ly.cout * Ly.fold.kf * cw;
          p.out = (float*)h->part.p + (long long)i * m.split_stride;
          KCHK(h, launch_conv_gemm(p, s));
        }
        hipLaunchKernelGGL(merge_splits_kernel, dim3((unsigned)((m.total + 255) / 256)), dim3(256), 0, s, m);
        HIPCHK(h, hipGetLastError());
      }
      RET(prof_mark(h, 0));
    } else if (Ly.kind == pl::GROUPED) {
      GroupArgs a;
      a.in = in, a.lens_in = lens_at(l), a.wfrag = h->w[di][l], a.bias = h->b[di][l], a.out = out;
      a.NS = NS, a.t_in_cap = (int)rows_in, a.t_out_cap = (int)rows, a.cin = Ly.cin, a.cout = Ly.cout, a.k = Ly.k, a.stride = Ly.stride, a.groups = Ly.groups,
      a.pad = Ly.pad, a.slope = h->cfg.slope, a.gp = Ly.gp;
      a.tiles = (int)pl::ceil_div(rows, Ly.gp.tm);
      RET(prof_mark(h, 1));
      RET(launch_grouped(h, a));
      RET(prof_mark(h, 1));
    } else {
      PostArgs a;
      a.in = in, a.lens_in = lens_at(l), a.lens_out = lens_at(1 + l), a.w = h->w[di][l], a.bias = h->b[di][l], a.out = out;
      a.NS = NS, a.rows_in = (int)rows_in, a.rows_l = (int)rows, a.C = Ly.cin, a.k = Ly.k, a.pad = Ly.pad;
      const long long waves = (long long)NS * rows;
      RET(prof_mark(h, 2));
      hipLaunchKernelGGL(post_conv_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
      HIPCHK(h, hipGetLastError());
      RET(prof_mark(h, 2));
    }
    if (!keep) {
      // the figures of this map: |r - g| per pair, and for the scores both moments per row
      for (int mode = (h->paired ? 0 : 1); mode <= (l == d.n_layers ? 1 : 0); ++mode) {
        const int units = mode == 0 ? nrows / 2 : nrows;
        long long nmax = 0;   // the longest map of this pass sizes the grid
        for (int r = 0; r < nrows; ++r) nmax = std::max<long long>(nmax, h->host_lens[h->lens_off[di][1 + l] + (long long)(row0 + r) * cols]);
        const int chunks = (int)pl::red_chunks(nmax * Ly.cout * cols);
        RedArgs q;
        q.a = out, q.seq_stride = rows * Ly.cout, q.lens = lens_at(1 + l), q.cols = cols, q.C = Ly.cout, q.chunks_max = chunks, q.mode = mode;
        q.partial = (double*)h->partial.p;
        MergeArgs m;
        m.partial = q.partial, m.lens = q.lens, m.cols = cols, m.C = Ly.cout, m.chunks_max = chunks, m.mode = mode;
        double* figs = (double*)h->figs.p;
        if (mode == 0) m.out = figs + (long long)(row0 / 2) * FM_SLOTS + di * pl::MAX_MAPS + l, m.out_stride = FM_SLOTS;
        else m.out = figs + (long long)(h->paired ? h->B : 0) * FM_SLOTS + (long long)row0 * MOM_SLOTS + di * 2, m.out_stride = MOM_SLOTS;
        RET(prof_mark(h, 2));
        hipLaunchKernelGGL(reduce_chunks_kernel, dim3((unsigned)chunks, (unsigned)units), dim3(256), 0, s, q);
        hipLaunchKernelGGL(reduce_merge_kernel, dim3((unsigned)units), dim3(256), 0, s, m);
        HIPCHK(h, hipGetLastError());
        RET(prof_mark(h, 2));
      }
    }
    in = out;
    rows_in = rows;
  }
  return E2ECR_OK;
}

// validation, the lengths tables and the signals of a call; then every discriminator, in passes of rows under the cap
int compute(e2ecr_handle* h, const void* y, const int64_t* y_lens, long long ld_y, const void* g, const int64_t* g_lens, long long ld_g, int B, int dtype,
            bool keep, e2ecr_result* results_out) {
  for (long long ldv : {ld_y, g ? ld_g : ld_y})
    if (const char* m = pl::batch_check(B, ldv, dtype)) return h->fail(E2ECR_EINVAL, std::string(m) + " (B " + std::to_string(B) + ", ld " + std::to_string(ldv) + ", dtype " + std::to_string(dtype) + ")");
  if (!y || !y_lens) return h->fail(E2ECR_EINVAL, "the samples and their lengths must not be NULL");
  if ((g == nullptr) != (g_lens == nullptr)) return h->fail(E2ECR_EINVAL, "g and g_lens must both be given or both be NULL");
  const size_t esz = dtype == E2ECR_PCM16 ? 2 : 4;
  if ((uintptr_t)y % esz || (uintptr_t)g % esz) return h->fail(E2ECR_EINVAL, "the samples must be aligned to their element size");
  const bool paired = g != nullptr;
  const int R = paired ? 2 * B : B;
  std::vector<int64_t> ly, lg;
  RET(fetch_host(h, y_lens, (size_t)B, ly));
  if (paired) RET(fetch_host(h, g_lens, (size_t)B, lg));
  std::vector<int64_t> n_row((size_t)R);
  int64_t nmax = 0;
  for (int b = 0; b < B; ++b)
    for (int side = 0; side < (paired ? 2 : 1); ++side) {
      const int64_t n = side ? lg[b] : ly[b];
      if (const char* m = pl::len_check(n, side ? ld_g : ld_y, h->min_len))
        return h->fail(E2ECR_EINVAL, std::string(m) + " (" + (side ? "g_lens[" : "lens[") + std::to_string(b) + "] = " + std::to_string((long long)n) + ", smallest " + std::to_string(h->min_len) + ", ld " + std::to_string(side ? ld_g : ld_y) + ")");
      n_row[paired ? 2 * b + side : b] = n;
      nmax = std::max(nmax, n);
    }
  if (!h->loaded) return h->fail(E2ECR_ESTATE, "a computing call before e2ecr_load_weights");
  const long long ld = nmax;   // the row stride inside the handle: the longest row of either side
  const int ND = (int)h->disc.size();
  // the lengths tables: per scale the rows' signal lengths, per discriminator and level the sequences' lengths
  std::vector<int32_t> tab;
  long long sig_ld[pl::MAX_SCALES] = {}, sig_off[pl::MAX_SCALES] = {}, nsig_off[pl::MAX_SCALES] = {};
  const int n_scales = std::max(1, (int)h->cfg.n_scales);
  long long pooled_floats = 0;
  for (int sc = 0; sc < n_scales; ++sc) {
    sig_ld[sc] = sc == 0 ? ld : pl::pool_len(sig_ld[sc - 1]);
    if (sc > 0) sig_off[sc] = pooled_floats, pooled_floats += (long long)R * sig_ld[sc];
    nsig_off[sc] = (long long)tab.size();
    for (int r = 0; r < R; ++r) {
      int64_t v = n_row[r];
      for (int i = 0; i < sc; ++i) v = pl::pool_len(v);
      tab.push_back((int32_t)v);
    }
  }
  long long rows_l[pl::MAX_DISC][pl::MAX_MAPS] = {}, lens_off[pl::MAX_DISC][pl::MAX_MAPS + 1] = {}, maps_off[pl::MAX_DISC][pl::MAX_MAPS] = {}, score_off[pl::MAX_DISC] = {};
  long long per_row_floats = 0, part_floats = 0, maps_floats = 0, score_floats = 0, partial_doubles = 2;
  for (int di = 0; di < ND; ++di) {
    const pl::Disc& d = h->disc[di];
    const int cols = pl::disc_cols(d);
    int64_t len[pl::MAX_MAPS + 1], rows[pl::MAX_MAPS];
    pl::disc_lens(d, nmax, len);
    pl::launch_rows(d, len, rows);
    for (int level = 0; level <= d.n_layers + 1; ++level) {
      lens_off[di][level] = (long long)tab.size();
      tab.resize(tab.size() + (size_t)R * cols);
    }
    for (int r = 0; r < R; ++r) {
      int64_t lr[pl::MAX_MAPS + 1];
      pl::disc_lens(d, n_row[r], lr);
      for (int level = 0; level <= d.n_layers + 1; ++level) {
        if (lr[level] < 1) return h->fail(E2ECR_EINVAL, "a row of " + std::to_string((long long)n_row[r]) + " samples is too short for the layer tables (discriminator " + std::to_string(di) + ")");
        for (int c = 0; c < cols; ++c) tab[lens_off[di][level] + (long long)r * cols + c] = (int32_t)lr[level];
      }
    }
    for (int l = 0; l <= d.n_layers; ++l) {
      const pl::Layer& Ly = d.layer[l];
      rows_l[di][l] = rows[l];
      if (Ly.kind == pl::DENSE && (rows[l] * Ly.stride * Ly.cin * 4 >= (1LL << 31) || rows[l] >= (1LL << 31) / 8))
        return h->fail(E2ECR_EINVAL, "rows of " + std::to_string((long long)nmax) + " samples are too long for the dense layers (2 GiB per sequence)");
      if (rows[l] * Ly.cout >= (1LL << 31)) return h->fail(E2ECR_EINVAL, "rows too long: a sequence's map must stay below 2^31 elements");
      if (l < d.n_layers) maps_off[di][l] = maps_floats, maps_floats += (long long)R * cols * rows[l] * Ly.cout;
      partial_doubles = std::max(partial_doubles, 2 * (long long)R * pl::red_chunks((long long)len[1 + l] * Ly.cout * cols));
    }
    score_off[di] = score_floats;
    score_floats += (long long)R * cols * rows[d.n_layers];
    per_row_floats = std::max<long long>(per_row_floats, pl::disc_buffer_floats(d, nmax));
    part_floats = std::max<long long>(part_floats, pl::disc_partial_floats(d, nmax));
  }
  const int unit = paired ? 2 : 1;
  const long long pass_rows = keep ? R : std::min<long long>(R, pl::rows_per_pass(per_row_floats, part_floats, h->cfg.workspace_cap_bytes, unit));
  // ---- nothing was enqueued so far
  RET(begin_call(h));
  h->have = 0;
  h->R = R, h->B = B, h->paired = paired, h->ld = ld;
  h->n_row.swap(n_row);
  h->host_lens.swap(tab);
  memcpy(h->rows_l, rows_l, sizeof rows_l), memcpy(h->lens_off, lens_off, sizeof lens_off), memcpy(h->maps_off, maps_off, sizeof maps_off);
  memcpy(h->score_off, score_off, sizeof score_off), memcpy(h->sig_ld, sig_ld, sizeof sig_ld), memcpy(h->sig_off, sig_off, sizeof sig_off);
  memcpy(h->nsig_off, nsig_off, sizeof nsig_off);
  const size_t n_figs = (size_t)(paired ? B : 0) * FM_SLOTS + (size_t)R * MOM_SLOTS;
  RET(reserve(h, h->lens_dev, h->host_lens.size() * 4));
  RET(reserve(h, h->sig, (size_t)R * ld * 4));
  if (pooled_floats) RET(reserve(h, h->pooled, (size_t)pooled_floats * 4));
  RET(reserve(h, h->scores, (size_t)score_floats * 4));
  if (part_floats) RET(reserve(h, h->part, (size_t)pass_rows * part_floats * 4));
  if (keep) {
    RET(reserve(h, h->maps, (size_t)maps_floats * 4));
  } else {
    RET(reserve(h, h->buf_a, (size_t)pass_rows * per_row_floats * 4));
    RET(reserve(h, h->buf_b, (size_t)pass_rows * per_row_floats * 4));
    RET(reserve(h, h->partial, (size_t)partial_doubles * 8));
    RET(reserve(h, h->figs, n_figs * 8));
  }
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->lens_dev.p, h->host_lens.data(), h->host_lens.size() * 4, hipMemcpyHostToDevice, s));
  // the signals: row 2 b = y_b and 2 b + 1 = g_b of a paired call, so that a pass holds whole pairs
  const size_t row_bytes = (size_t)ld * esz;
  if (dtype == E2ECR_PCM16) RET(reserve(h, h->raw, (size_t)R * row_bytes));
  char* dst = (char*)(dtype == E2ECR_PCM16 ? h->raw.p : h->sig.p);
  // (each side has a row stride of its own; what a row holds past its own length is copied along and never read)
  const size_t wy = (size_t)std::min(ld, ld_y) * esz, wg = (size_t)std::min(ld, ld_g) * esz;
  if (!paired) {
    HIPCHK(h, hipMemcpy2DAsync(dst, row_bytes, y, (size_t)ld_y * esz, wy, (size_t)B, hipMemcpyDefault, s));
  } else {
    HIPCHK(h, hipMemcpy2DAsync(dst, 2 * row_bytes, y, (size_t)ld_y * esz, wy, (size_t)B, hipMemcpyDefault, s));
    HIPCHK(h, hipMemcpy2DAsync(dst + row_bytes, 2 * row_bytes, g, (size_t)ld_g * esz, wg, (size_t)B, hipMemcpyDefault, s));
  }
  h->pev_used = 0;
  if (dtype == E2ECR_PCM16) {
    const size_t n = (size_t)R * ld;
    hipLaunchKernelGGL(pcm_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int16_t*)h->raw.p, (float*)h->sig.p, n);
    HIPCHK(h, hipGetLastError());
  }
  const int32_t* Ld = (const int32_t*)h->lens_dev.p;
  for (int sc = 1; sc < n_scales; ++sc) {
    const float* src = sc == 1 ? (const float*)h->sig.p : (const float*)h->pooled.p + sig_off[sc - 1];
    const long long total = (long long)R * sig_ld[sc];
    RET(prof_mark(h, 2));
    hipLaunchKernelGGL(pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, sig_ld[sc - 1], Ld + nsig_off[sc - 1], (float*)h->pooled.p + sig_off[sc], sig_ld[sc], R);
    HIPCHK(h, hipGetLastError());
    RET(prof_mark(h, 2));
  }
  for (long long r0 = 0; r0 < R; r0 += pass_rows) {
    const int nr = (int)std::min<long long>(pass_rows, R - r0);
    for (int di = 0; di < ND; ++di) RET(run_disc(h, di, (int)r0, nr, keep));
  }
  if (!keep) {
    h->host_figs.resize(n_figs);
    HIPCHK(h, hipMemcpyAsync(h->host_figs.data(), h->figs.p, n_figs * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(h, hipStreamSynchronize(s));
  h->unfinished = false;
  if (h->profile) {
    double ms[3] = {0, 0, 0};
    for (size_t i = 0; i + 1 < h->pev_used; i += 2) {
      float t = 0.f;
      HIPCHK(h, hipEventElapsedTime(&t, h->pev[i], h->pev[i + 1]));
      ms[h->pcls[i]] += t;
    }
    for (int i = 0; i < 3; ++i) h->last_ms[i] = ms[i];
  }
  h->have = keep ? 2 : 1;
  if (keep || !results_out) return E2ECR_OK;
  const double NaN = std::numeric_limits<double>::quiet_NaN();
  const double* fm = h->host_figs.data();
  const double* mom = fm + (size_t)(paired ? B : 0) * FM_SLOTS;
  for (int b = 0; b < B; ++b) {
    e2ecr_result& r = results_out[b];
    r.status = 0, r.n_disc = ND;
    for (auto& row : r.fm)
      for (double& v : row) v = NaN;
    for (int i = 0; i < pl::MAX_DISC; ++i) r.d_real[i] = r.d_fake[i] = r.g_fake[i] = NaN;
    const bool differ = paired && ly[b] != lg[b];
    if (differ) r.status |= E2ECR_ST_LENGTHS_DIFFER;
    if (!paired) r.status |= E2ECR_ST_ONE_SIDED;
    double fl[2] = {0, 0}, dl[2] = {0, 0}, gl[2] = {0, 0};
    for (int di = 0; di < ND; ++di) {
      const int k = h->disc[di].period ? 0 : 1;
      const double* my = mom + (size_t)(paired ? 2 * b : b) * MOM_SLOTS + di * 2;
      const double* mg = paired ? my + MOM_SLOTS : my;
      r.d_real[di] = my[0], r.d_fake[di] = mg[1], r.g_fake[di] = mg[0];
      dl[k] += r.d_real[di] + r.d_fake[di];
      gl[k] += r.g_fake[di];
      if (paired && !differ)
        for (int l = 0; l <= h->disc[di].n_layers; ++l) {
          r.fm[di][l] = fm[(size_t)b * FM_SLOTS + di * pl::MAX_MAPS + l];
          fl[k] += r.fm[di][l];
        }
    }
    const bool have_fm = paired && !differ;
    r.feature_loss_mpd = have_fm ? 2.0 * fl[0] : NaN, r.feature_loss_msd = have_fm ? 2.0 * fl[1] : NaN;
    r.disc_loss_mpd = dl[0], r.disc_loss_msd = dl[1], r.gen_loss_mpd = gl[0], r.gen_loss_msd = gl[1];
  }
  return E2ECR_OK;
}

// a resident [B * cols, rows, C] tensor in the reference's layout through the staging buffer
// (all R rows of the call; t_out [R]; *tmax_out the longest).  out == nullptr: the staging buffer is filled and left for the caller
int to_layout(e2ecr_handle* h, const float* src, int di, int level, long long rows, int C, long long* t_out, long long* tmax_out) {
  const int cols = pl::disc_cols(h->disc[di]);
  long long Tmax = 0;
  for (int r = 0; r < h->R; ++r) {
    const long long t = h->host_lens[h->lens_off[di][level] + (long long)r * cols];
    if (t_out) t_out[r] = t;
    Tmax = std::max(Tmax, t);
  }
  *tmax_out = Tmax;
  if (!src) return E2ECR_OK;
  const long long total = (long long)h->R * C * Tmax * cols;
  HIPCHK(h, hipSetDevice(h->device));
  RET(reserve(h, h->stage, (size_t)total * 4));
  hipLaunchKernelGGL(layout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, src, (const int32_t*)h->lens_dev.p + h->lens_off[di][level], (float*)h->stage.p,
                     cols, (int)rows, C, (int)Tmax, total);
  HIPCHK(h, hipGetLastError());
  return E2ECR_OK;
}

}  // namespace

extern "C" {

const char* e2ecr_version(void) { return "e2etts-critic 1 E2ECR_SRC_HASH=" E2ECR_SRC_HASH; }
int e2ecr_abi_version(void) { return E2ECR_ABI_VERSION; }
const char* e2ecr_last_error(const e2ecr_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void e2ecr_default_config(e2ecr_config* c) {
  if (!c) return;
  memset(c, 0, sizeof *c);
  const int periods[5] = {2, 3, 5, 7, 11};
  c->n_periods = 5;
  for (int i = 0; i < 5; ++i) c->periods[i] = periods[i];
  const int ch[5] = {32, 128, 512, 1024, 1024};
  c->n_mpd_layers = 5;
  for (int i = 0; i < 5; ++i) c->mpd[i] = e2ecr_layer{ch[i], 5, i < 4 ? 3 : 1, 1, 2};
  c->mpd_post = e2ecr_layer{1, 3, 1, 1, 1};
  c->n_scales = 3;
  c->n_msd_layers = 7;
  const e2ecr_layer msd[7] = {{128, 15, 1, 1, 7}, {128, 41, 2, 4, 20}, {256, 41, 2, 16, 20}, {512, 41, 4, 16, 20}, {1024, 41, 4, 16, 20}, {1024, 41, 1, 16, 20}, {1024, 5, 1, 1, 2}};
  for (int i = 0; i < 7; ++i) c->msd[i] = msd[i];
  c->msd_post = e2ecr_layer{1, 3, 1, 1, 1};
  c->slope = 0.1f;
  c->workspace_cap_bytes = 0;
}

int e2ecr_create(int device_id, const e2ecr_config* config, e2ecr_handle** out) {
  if (!out) {
    g_create_error = "e2ecr_create: out is NULL";
    return E2ECR_EINVAL;
  }
  *out = nullptr;
  if (device_id < 0) {
    g_create_error = "e2ecr_create: device_id must not be negative";
    return E2ECR_EINVAL;
  }
  e2ecr_config c;
  if (config) c = *config;
  else e2ecr_default_config(&c);
  std::vector<pl::Disc> discs;
  int min_len = 2;
  std::string why;
  if (build_discs(c, discs, &min_len, why) != E2ECR_OK) {
    g_create_error = "e2ecr_create: " + why;
    return E2ECR_EINVAL;
  }
  e2ecr_handle* h = new (std::nothrow) e2ecr_handle();
  if (!h) {
    g_create_error = "out of host memory";
    return E2ECR_ENOMEM;
  }
  h->device = device_id;
  h->cfg = c;
  h->disc.swap(discs);
  h->min_len = min_len;
  *out = h;
  return E2ECR_OK;
}

void e2ecr_destroy(e2ecr_handle* h) { companion::destroy(h); }

int e2ecr_load_weights(e2ecr_handle* h, const void* blob, size_t nbytes) {
  if (!h) return E2ECR_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!blob) return h->fail(E2ECR_EINVAL, "blob is NULL");
  if (nbytes < sizeof(BlobHeader)) return h->fail(E2ECR_EINVAL, "weight blob too small");
  const bool dev = is_device_pointer(blob);
  BlobHeader hd;
  if (dev) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(&hd, blob, sizeof hd, hipMemcpyDefault));
  } else {
    memcpy(&hd, blob, sizeof hd);
  }
  if (const char* m = blob_check_header(hd, nbytes)) return h->fail(E2ECR_EINVAL, m);
  std::vector<BlobEntry> dir(hd.n_entries);
  if (hd.n_entries) {
    if (dev) HIPCHK(h, hipMemcpy(dir.data(), (const char*)blob + sizeof hd, dir.size() * sizeof(BlobEntry), hipMemcpyDefault));
    else memcpy(dir.data(), (const char*)blob + sizeof hd, dir.size() * sizeof(BlobEntry));
  }
  std::vector<BlobTensor> tensors;
  std::string bad;
  if (const char* m = blob_check_directory(hd, dir.data(), nbytes, tensors, bad)) return h->fail(E2ECR_EINVAL, std::string(m) + ": " + bad);
  const float* w[pl::MAX_DISC][pl::MAX_MAPS] = {};
  const float* b[pl::MAX_DISC][pl::MAX_MAPS] = {};
  std::vector<Want> wants;
  for (int di = 0; di < (int)h->disc.size(); ++di)
    for (int l = 0; l <= h->disc[di].n_layers; ++l) {
      wants.push_back(Want{wname(di, l, "w"), weight_numel(h->disc[di].layer[l]), &w[di][l]});
      wants.push_back(Want{wname(di, l, "b"), (size_t)h->disc[di].layer[l].cout, &b[di][l]});
    }
  std::vector<uint64_t> offs(wants.size());
  for (size_t i = 0; i < wants.size(); ++i) {
    const BlobTensor* t = nullptr;
    for (const auto& x : tensors)
      if (x.name == wants[i].name) t = &x;
    if (!t) return h->fail(E2ECR_EINVAL, "weight blob has no tensor '" + wants[i].name + "'");
    if (t->numel != wants[i].numel)
      return h->fail(E2ECR_EINVAL, "tensor '" + wants[i].name + "' has " + std::to_string(t->numel) + " elements, this critic's tables need " + std::to_string(wants[i].numel));
    offs[i] = t->offset;
  }
  RET(open_device(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // nothing reads the old weights
  RET(reserve(h, h->blob, nbytes));
  HIPCHK(h, hipMemcpyAsync(h->blob.p, blob, nbytes, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < wants.size(); ++i) *wants[i].dst = (const float*)((const char*)h->blob.p + offs[i]);
  memcpy(h->w, w, sizeof w);
  memcpy(h->b, b, sizeof b);
  h->loaded = true;
  return E2ECR_OK;
}

void* e2ecr_stream(e2ecr_handle* h) { return companion::stream(h); }
int e2ecr_order_after(e2ecr_handle* h, void* caller_stream) { return companion::order_after(h, caller_stream); }
int e2ecr_sync(e2ecr_handle* h) { return companion::sync(h); }
size_t e2ecr_device_bytes(const e2ecr_handle* h) { return companion::device_bytes(h); }

int e2ecr_run(e2ecr_handle* h, const void* y, const int64_t* y_lens, long long ld_y, const void* g, const int64_t* g_lens, long long ld_g, int B, int dtype,
              e2ecr_result* results_out) {
  if (!h) return E2ECR_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  return compute(h, y, y_lens, ld_y, g, g_lens, ld_g, B, dtype, false, results_out);
}

int e2ecr_forward(e2ecr_handle* h, const void* x, const int64_t* lens, int B, long long ld, int dtype) {
  if (!h) return E2ECR_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  return compute(h, x, lens, ld, nullptr, nullptr, ld, B, dtype, true, nullptr);
}

int e2ecr_fetch_scores(e2ecr_handle* h, int side, int disc, float* out, long long* n_out, long long* n_max_out) {
  if (!h) return E2ECR_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->have) return h->fail(E2ECR_ESTATE, "e2ecr_fetch_scores without a completed computing call");
  if (disc < 0 || disc >= (int)h->disc.size()) return h->fail(E2ECR_EINVAL, "disc must lie in [0, n_disc)");
  if (side != 0 && !(side == 1 && h->paired)) return h->fail(E2ECR_EINVAL, "side must be 0, or 1 after a two-sided run");
  const pl::Disc& d = h->disc[disc];
  const int nl = d.n_layers, cols = pl::disc_cols(d);
  const int step = h->paired ? 2 : 1;   // rows 2 b + side of a two-sided run
  std::vector<long long> t_all((size_t)h->R);
  long long tmax = 0;
  RET(to_layout(h, out ? (const float*)h->scores.p + h->score_off[disc] : nullptr, disc, 1 + nl, h->rows_l[disc][nl], 1, t_all.data(), &tmax));
  const long long nmax = tmax * cols;
  if (n_out)
    for (int b = 0; b < h->B; ++b) n_out[b] = t_all[(size_t)step * b + side] * cols;
  if (n_max_out) *n_max_out = nmax;
  if (!out) return E2ECR_OK;
  HIPCHK(h, hipMemcpy2DAsync(out, (size_t)nmax * 4, (const float*)h->stage.p + (size_t)side * nmax, (size_t)step * nmax * 4, (size_t)nmax * 4, (size_t)h->B, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return E2ECR_OK;
}

int e2ecr_fetch_fmap(e2ecr_handle* h, int disc, int layer, float* out, long long* shape_out, long long* t_out) {
  if (!h) return E2ECR_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->have != 2) return h->fail(E2ECR_ESTATE, "e2ecr_fetch_fmap without a completed e2ecr_forward");
  if (disc < 0 || disc >= (int)h->disc.size()) return h->fail(E2ECR_EINVAL, "disc must lie in [0, n_disc)");
  const pl::Disc& d = h->disc[disc];
  if (layer < 0 || layer > d.n_layers) return h->fail(E2ECR_EINVAL, "layer must lie in [0, n_layers]");
  const float* src = layer == d.n_layers ? (const float*)h->scores.p + h->score_off[disc] : (const float*)h->maps.p + h->maps_off[disc][layer];
  const int C = d.layer[layer].cout, cols = pl::disc_cols(d);
  long long tmax = 0;
  RET(to_layout(h, out ? src : nullptr, disc, 1 + layer, h->rows_l[disc][layer], C, t_out, &tmax));
  if (shape_out) shape_out[0] = h->R, shape_out[1] = C, shape_out[2] = tmax, shape_out[3] = cols;
  if (!out) return E2ECR_OK;
  HIPCHK(h, hipMemcpyAsync(out, h->stage.p, (size_t)h->R * C * tmax * cols * 4, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return E2ECR_OK;
}

int e2ecr_profile_enable(e2ecr_handle* h, int on) { return companion::profile_enable(h, on); }
int e2ecr_profile_read(e2ecr_handle* h, double ms_out[3]) { return companion::profile_read(h, ms_out); }

#ifdef E2ECR_TEST_HOOKS
int e2ecr_debug_poison_workspace(e2ecr_handle* h) {
  if (!h) return E2ECR_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(poison_workspaces(h));
  h->unfinished = false;
  h->have = 0;
  return E2ECR_OK;
}

int e2ecr_debug_grouped_conv(e2ecr_handle* h, const float* in, const int32_t* lens_in, const float* wfrag, const float* bias, float* out, int B, int t_in_cap,
                             int t_out_cap, int cin, int cout, int k, int stride, int groups, int pad, float slope, int tm) {
  if (!h) return E2ECR_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!in || !lens_in || !wfrag || !bias || !out) return h->fail(E2ECR_EINVAL, "NULL pointer");
  if (!is_device_pointer(in) || !is_device_pointer(lens_in) || !is_device_pointer(wfrag) || !is_device_pointer(bias) || !is_device_pointer(out))
    return h->fail(E2ECR_EINVAL, "e2ecr_debug_grouped_conv works on device buffers");
  if (B < 1 || B > pl::MAX_B || t_in_cap < 1 || t_out_cap < 1 || t_in_cap > pl::MAX_LEN || t_out_cap > pl::MAX_LEN) return h->fail(E2ECR_EINVAL, "B, t_in_cap, t_out_cap out of range");
  const pl::LayerSpec sp{cout, k, stride, groups, pad};
  pl::Layer L;
  if (cin < 1 || cin > pl::MAX_CH) return h->fail(E2ECR_EINVAL, "cin out of range");
  if (const char* m = pl::layer_plan(sp, cin, false, false, &L)) return h->fail(E2ECR_EINVAL, m);
  if (L.kind != pl::GROUPED) return h->fail(E2ECR_EINVAL, "not a grouped layer (groups must exceed 1)");
  if (tm)
    if (const char* m = pl::group_plan(cin, cout, k, stride, groups, tm, &L.gp)) return h->fail(E2ECR_EINVAL, m);
  if (!(slope >= 0.f && slope <= 1.f)) return h->fail(E2ECR_EINVAL, "slope must lie in [0, 1]");
  if ((long long)t_in_cap * cin >= (1LL << 31) || (long long)t_out_cap * cout >= (1LL << 31)) return h->fail(E2ECR_EINVAL, "a sequence must stay below 2^31 elements");
  RET(begin_call(h));
  GroupArgs a;
  a.in = in, a.lens_in = lens_in, a.wfrag = wfrag, a.bias = bias, a.out = out;
  a.NS = B, a.t_in_cap = t_in_cap, a.t_out_cap = t_out_cap, a.cin = cin, a.cout = cout, a.k = k, a.stride = stride, a.groups = groups, a.pad = pad, a.slope = slope;
  a.gp = L.gp;
  a.tiles = (int)pl::ceil_div(t_out_cap, L.gp.tm);
  RET(launch_grouped(h, a));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->unfinished = false;
  return E2ECR_OK;
}
#endif

}  // extern "C"
