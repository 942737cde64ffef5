// libe2etts_align.so: the reference's AlignmentEncoder (U/layers.py:275-369) and monotonic alignment search (U/function.py:96-137) behind
// the C ABI of include/e2etts_align.h.  A companion of libe2etts_hip.so that shares its kernel objects (the exact-fp32 convolution
// launch_conv_gemm serves the projections) and none of its entry points.
//
// Three kinds of device work per call:
//   projections   key_proj / query_proj as exact-fp32 conv_gemm launches on channels-last [B, N, C] tensors, the speaker terms added to every
//                 position first (aln_add_rows_kernel);
//   attention     aln_attn_kernel: squared distance in the direct form, both softmaxes and the prior in one pass per 16-frame tile, the
//                 scores of the tile living in LDS -- the reference's [B, n_att, T, L] tensor is never formed;
//   search        aln_mas_wave_kernel (L <= 256): one wavefront per utterance, 1, 2 or 4 phonemes per lane by the row width, the previous log_p row
//                 in registers, one shuffle per frame; aln_mas_kernel (wider rows): one workgroup per utterance, threads over phonemes, the row ping-ponged in
//                 LDS, one barrier per frame.  Back-pointers one bit per cell, one lane backtracks.
// The beta-binomial attention prior (e2ealign_prior; the *_bb entry points) is generated in float64: aln_prior_cols_kernel forms the column
// terms of the batch once, aln_prior_kernel writes the padded tensor, and the generated-prior form of aln_attn_kernel evaluates the same
// cells where the given-prior form loads them.  Argument checks, table size and index formulas: prior_plan.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../../include/e2etts_align.h"
#ifdef E2EALIGN_TEST_HOOKS
#define E2E_COMPANION_TEST_HOOKS
#endif
#include "../companion/handle.h"
#include "../host_logic.h"
#include "../kernels.h"
#include "prior_plan.h"

#ifndef E2EALIGN_SRC_HASH
#define E2EALIGN_SRC_HASH "unknown"
#endif

using namespace e2etts;
using namespace e2etts::companion;

static_assert(E2EALIGN_OK == E_OK && E2EALIGN_EINVAL == E_INVAL && E2EALIGN_EHIP == E_HIP && E2EALIGN_ESTATE == E_STATE && E2EALIGN_ENOMEM == E_NOMEM,
              "include/e2etts_align.h and csrc/companion/handle.h disagree on the error codes");

namespace pp = e2ealign_prior_plan;
static_assert(pp::MAX_B == E2EALIGN_MAX_B && pp::MAX_L == E2EALIGN_MAX_L && pp::MAX_SCALING == E2EALIGN_MAX_PRIOR_SCALING,
              "include/e2etts_align.h and csrc/align/prior_plan.h disagree on the limits");

namespace {

constexpr int MAS_THREADS = 256;
constexpr int MAS_COLS = E2EALIGN_MAX_L / MAS_THREADS;   // columns per thread at the widest row
constexpr size_t MAS_LDS_BUDGET = 40 * 1024;            // back-pointer bits live in LDS up to this (with the three [L] rows), else in the workspace
constexpr size_t ATTN_LDS_MAX = 64 * 1024;

// x[b, t, :] += s[b, :]
__global__ void aln_add_rows_kernel(float* x, const float* s, int B, int N, int C) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)B * N * C;
  if (i >= n) return;
  const int c = (int)(i % C);
  const int b = (int)(i / ((long long)N * C));
  x[i] = x[i] + s[(size_t)b * C + c];
}

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- the generated prior.  Every float64 product lives in the two functions below, which are never inlined: aln_prior_kernel and the
// generated-prior form of aln_attn_kernel call the SAME machine code, so a cell has the same bits wherever it is formed (no contraction
// or scheduling choice of the compiler can differ between the two kernels).  What the callers add around them are sums and differences.

// log-gamma of frame argument `which` of frame t: 0 alpha, 1 beta, 2 alpha + beta, 3 P + alpha + beta
__device__ __noinline__ double aln_prior_frame_lgamma(int P, int M, double s, int t, int which) {
#pragma clang fp contract(off)
  const double a = pp::alpha_of(s, t), b = pp::beta_of(s, M, t);
  const double ab = a + b;
  const double x = which == 0 ? a : which == 1 ? b : which == 2 ? ab : (double)P + ab;
  return lgamma(x);
}

// The frame term -log B(alpha, beta) - lgamma(P + alpha + beta), formed once per frame by the wavefront that owns it: lanes 0 .. 3 take one
// log-gamma each (every lane evaluates one; the four are broadcast).  All 64 lanes must be active.
__device__ __forceinline__ double aln_prior_frame_term(int P, int M, double s, int t, int lane) {
  const double v = aln_prior_frame_lgamma(P, M, s, t, lane & 3);
  const double la = __shfl(v, 0, 64), lb = __shfl(v, 1, 64), lab = __shfl(v, 2, 64), ln = __shfl(v, 3, 64);
  return (lab - (la + lb)) - ln;
}

// The column term log C(P, k), k < P.
__device__ __forceinline__ double aln_prior_col_term(int P, int k) { return (lgamma((double)P + 1.0) - lgamma((double)k + 1.0)) - lgamma((double)(P - k) + 1.0); }

// THE prior value of cell (t, k), t < M, k < P, of a row with P phonemes and M frames (include/e2etts_align.h): float64 throughout,
// rounded to fp32 once.  `col` and `frame` are the terms above.
__device__ __noinline__ float aln_prior_value(int P, int M, double s, int t, int k, double col, double frame) {
#pragma clang fp contract(off)
  const double a = pp::alpha_of(s, t), b = pp::beta_of(s, M, t);
  const double e = lgamma((double)k + a) + lgamma((double)(P - k) + b);
  return (float)exp((col + frame) + e);
}

// cols[b, k] = log C(txt_lens[b], k) for k < txt_lens[b], 0 beyond (never read)
__global__ void aln_prior_cols_kernel(const int32_t* __restrict__ txt_lens, double* __restrict__ cols, int B, int L) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pp::col_table_doubles(B, L)) return;
  const int b = (int)(i / (size_t)L), k = (int)(i - (size_t)b * L);
  const int P = txt_lens[b];
  cols[pp::col_index(b, k, L)] = k < P ? aln_prior_col_term(P, k) : 0.0;
}

// What a kernel needs to generate the prior: the column table, the frames of every row, the scaling factor (txt_lens travels apart).
struct PriorGen {
  const double* cols;
  const int32_t* mel_lens;
  double s;
};

// The padded [B, T, L] prior: one wavefront per frame (workgroup x = frames 4 x .. 4 x + 3 of utterance blockIdx.y), lanes stride the columns.
__global__ __launch_bounds__(256) void aln_prior_kernel(const int32_t* __restrict__ txt_lens, PriorGen gen, float* __restrict__ out, int T, int L) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, t = blockIdx.x * pp::FRAMES_PER_GROUP + (threadIdx.x >> 6);
  if (t >= T) return;   // wave-uniform
  const int P = txt_lens[b], M = gen.mel_lens[b];
  const bool live = t < M;   // wave-uniform
  const double frame = live ? aln_prior_frame_term(P, M, gen.s, t, lane) : 0.0;
  for (int j = lane; j < L; j += 64)
    out[pp::cell_index(b, t, j, T, L)] = (live && j < P) ? aln_prior_value(P, M, gen.s, t, j, gen.cols[pp::col_index(b, j, L)], frame) : 0.f;
}

// One workgroup = TI = 4 * FPT frames of one utterance against ALL its L keys (padded ones included: the prior's log-softmax runs over
// them).  Phase 1: 64 keys at a time in LDS (row stride odd: conflict-free), thread (wave g, lane j) accumulates the squared distance of key j
// to the FPT frames of wave g in four interleaved fma chains per frame (channel c goes to chain c mod 4; chains summed (0 + 1) + (2 + 3)),
// score = -temperature * d into the tile's score rows in LDS.  Phase 2: wave g owns its FPT rows; lanes stride the columns, so every lane
// rereads only what it wrote: log_softmax over L columns + log(prior + 1e-8) when a prior is given, attn_logprob out, then the masked softmax
// (masked keys exactly 0).  Every global access is guarded by t < T and j < L.  GEN: the prior is not loaded but generated -- cell (t, j) is
// aln_prior_value where t < mel_lens[b] and j < txt_lens[b] (which is then required) and 0 elsewhere, the tensor aln_prior_kernel writes.
template <int FPT, bool GEN>
__global__ __launch_bounds__(256) void aln_attn_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ prior,
                                                       const int32_t* __restrict__ txt_lens, float* __restrict__ attn, float* __restrict__ logp,
                                                       int T, int L, int C, float temperature, PriorGen gen) {
  constexpr int TI = 4 * FPT;
  extern __shared__ __attribute__((aligned(16))) float aln_smem[];
  const int Cs = C | 1;
  float* sq = aln_smem;          // [TI][C]
  float* sk = sq + TI * C;       // [64][Cs]
  float* ss = sk + 64 * Cs;      // [TI][L]
  const int b = blockIdx.y, i0 = blockIdx.x * TI, tid = threadIdx.x;
  const int lane = tid & 63, g = tid >> 6;
  for (int e = tid; e < TI * C; e += 256) {
    const int i = e / C, c = e - i * C, t = i0 + i;
    sq[e] = t < T ? q[((size_t)b * T + t) * C + c] : 0.f;
  }
  for (int j0 = 0; j0 < L; j0 += 64) {
    __syncthreads();   // the previous key tile is consumed (first pass: sq is staged)
    for (int e = tid; e < 64 * C; e += 256) {
      const int j = e / C, c = e - j * C;
      sk[j * Cs + c] = j0 + j < L ? k[((size_t)b * L + j0 + j) * C + c] : 0.f;
    }
    __syncthreads();
    float acc[FPT][4];
#pragma unroll
    for (int f = 0; f < FPT; ++f) acc[f][0] = acc[f][1] = acc[f][2] = acc[f][3] = 0.f;
    const float* kr = sk + lane * Cs;
    int c = 0;
    for (; c + 4 <= C; c += 4) {
      const float k0 = kr[c], k1 = kr[c + 1], k2 = kr[c + 2], k3 = kr[c + 3];
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        const float* qr = sq + (g * FPT + f) * C + c;
        const float d0 = qr[0] - k0, d1 = qr[1] - k1, d2 = qr[2] - k2, d3 = qr[3] - k3;
        acc[f][0] = fmaf(d0, d0, acc[f][0]);
        acc[f][1] = fmaf(d1, d1, acc[f][1]);
        acc[f][2] = fmaf(d2, d2, acc[f][2]);
        acc[f][3] = fmaf(d3, d3, acc[f][3]);
      }
    }
    for (; c < C; ++c) {   // C % 4 channels left: they continue chains 0 .. 2
      const float kc = kr[c];
#pragma unroll
      for (int f = 0; f < FPT; ++f) {
        const float d = sq[(g * FPT + f) * C + c] - kc;
        if ((c & 3) == 0) acc[f][0] = fmaf(d, d, acc[f][0]);
        else if ((c & 3) == 1) acc[f][1] = fmaf(d, d, acc[f][1]);
        else acc[f][2] = fmaf(d, d, acc[f][2]);
      }
    }
    if (j0 + lane < L) {
#pragma unroll
      for (int f = 0; f < FPT; ++f) ss[(g * FPT + f) * L + j0 + lane] = -temperature * ((acc[f][0] + acc[f][1]) + (acc[f][2] + acc[f][3]));
    }
  }
  // phase 2 reads only what the same lane wrote (column j belongs to lane j mod 64 of wave g in both phases): no barrier needed
  const int len = txt_lens ? txt_lens[b] : L;
  for (int f = 0; f < FPT; ++f) {
    const int t = i0 + g * FPT + f;
    if (t >= T) break;   // wave-uniform
    float* row = ss + (g * FPT + f) * L;
    const size_t base = ((size_t)b * T + t) * L;
    if (GEN || prior) {
      float m = -INFINITY;
      for (int j = lane; j < L; j += 64) m = fmaxf(m, row[j]);
      m = wave_max(m);
      float s = 0.f;
      for (int j = lane; j < L; j += 64) s += expf(row[j] - m);
      s = wave_sum(s);
      const float ls = logf(s);
      if constexpr (GEN) {
        const int M = gen.mel_lens[b];
        const bool live = t < M;   // wave-uniform
        const double frame = live ? aln_prior_frame_term(len, M, gen.s, t, lane) : 0.0;
        for (int j = lane; j < L; j += 64) {
          const float p = (live && j < len) ? aln_prior_value(len, M, gen.s, t, j, gen.cols[pp::col_index(b, j, L)], frame) : 0.f;
          row[j] = ((row[j] - m) - ls) + logf(p + 1e-8f);
        }
      } else {
        for (int j = lane; j < L; j += 64) row[j] = ((row[j] - m) - ls) + logf(prior[base + j] + 1e-8f);
      }
    }
    float m2 = -INFINITY;
    for (int j = lane; j < L; j += 64) {
      const float v = row[j];
      logp[base + j] = v;
      if (j < len) m2 = fmaxf(m2, v);
    }
    m2 = wave_max(m2);
    float s2 = 0.f;
    for (int j = lane; j < len; j += 64) s2 += expf(row[j] - m2);
    s2 = wave_sum(s2);
    for (int j = lane; j < L; j += 64) attn[base + j] = j < len ? expf(row[j] - m2) / s2 : 0.f;
  }
}

// Backtracking by one lane, from column n - 1 of the last frame: marks attn_hard, counts the marks per column, follows the back-pointer bits.
__device__ __forceinline__ void mas_backtrack(const uint32_t* bits, int* cnt, float* hard, int b, int n, int m, int T, int L, int W) {
  int idx = n - 1;
  for (int i = m - 1; i >= 1; --i) {
    cnt[idx] += 1;
    if (hard) hard[((size_t)b * T + i) * L + idx] = 1.f;
    if ((bits[(size_t)i * W + (idx >> 5)] >> (idx & 31)) & 1u) idx -= 1;
  }
  cnt[idx] += 1;
  if (hard) hard[(size_t)b * T * L + idx] = 1.f;
  // the reference's closing `opt[0, curr_text_idx] = 1` with curr_text_idx read from prev_ind's row 0, which is all zeros: opt[0, 0]
  if (idx != 0) {
    cnt[0] += 1;
    if (hard) hard[(size_t)b * T * L] = 1.f;
  }
}

// The same search for rows of at most MAS_WAVE_L phonemes in ONE wavefront per utterance: lane l owns the CPL columns CPL l .. CPL l + CPL - 1
// (CPL = 1, 2 or 4 by the row width, so that narrow rows use every lane: the kernel is bound by its instruction count per frame, the fp32
// logarithms first), the previous log_p row lives in registers and only column CPL l - 1 crosses lanes (one shuffle per frame) -- no barrier and no LDS round trip on
// the frame-to-frame chain, which is what bounds the workgroup form.  Same additions, same comparisons, same bit layout of the back-pointers
// (the CPL bits of a lane are merged over groups of 32 / CPL lanes into the word of their 32 columns), same backtracking.
constexpr int MAS_WAVE_L = 256;
constexpr int MAS_WAVE_R = 8;   // frames per register block
template <int CPL>
__global__ __launch_bounds__(64) void aln_mas_wave_kernel(const float* __restrict__ map, int is_log, const int32_t* __restrict__ in_lens,
                                                          const int32_t* __restrict__ out_lens, uint32_t* bits_ws, int bits_in_lds, float* hard,
                                                          float* __restrict__ dur, int T, int L, int W) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mas_smem[];
  int* cnt = (int*)mas_smem;   // [L]
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = in_lens[b], m = out_lens[b];
  const float* a = map + (size_t)b * T * L;
  uint32_t* bits = bits_in_lds ? mas_smem + L : bits_ws + (size_t)b * T * W;
  for (int j = lane; j < L; j += 64) cnt[j] = 0;
  const int j0 = CPL * lane;
  // frames are loaded MAS_WAVE_R at a time, one block ahead of the block being combined: the frame-to-frame chain then waits on registers,
  // not on a global load per frame
  float prev[CPL], cur[MAS_WAVE_R][CPL], nxt[MAS_WAVE_R][CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) prev[c] = -INFINITY;   // row 0: columns >= 1 are -inf
  if (lane == 0) prev[0] = is_log ? a[0] : logf(a[0]);
#pragma unroll
  for (int r = 0; r < MAS_WAVE_R; ++r)
#pragma unroll
    for (int c = 0; c < CPL; ++c) cur[r][c] = (j0 + c < n && 1 + r < m) ? a[(size_t)(1 + r) * L + j0 + c] : 1.f;
  for (int i0 = 1; i0 < m; i0 += MAS_WAVE_R) {
#pragma unroll
    for (int r = 0; r < MAS_WAVE_R; ++r)
#pragma unroll
      for (int c = 0; c < CPL; ++c) nxt[r][c] = (j0 + c < n && i0 + MAS_WAVE_R + r < m) ? a[(size_t)(i0 + MAS_WAVE_R + r) * L + j0 + c] : 1.f;
#pragma unroll
    for (int r = 0; r < MAS_WAVE_R; ++r) {
      const int i = i0 + r;
      if (i >= m) break;   // wavefront-uniform
      const float left = __shfl_up(prev[CPL - 1], 1, 64);   // column CPL l - 1 (lane 0: unused, column 0 has no diagonal)
      uint32_t nib = 0;
      float nw[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int j = j0 + c;
        float p = prev[c];
        const float pd = c == 0 ? left : prev[c - 1];
        if (j >= 1 && j < n && pd >= p) {   // the reference's >= : ties, -inf ties included, take the diagonal
          p = pd;
          nib |= 1u << c;
        }
        nw[c] = (is_log ? cur[r][c] : logf(cur[r][c])) + p;
      }
#pragma unroll
      for (int c = 0; c < CPL; ++c) prev[c] = nw[c];
      if (CPL == 1) {
        const unsigned long long bal = __ballot(nib != 0);
        if (lane == 0) {
          bits[(size_t)i * W] = (uint32_t)bal;
          if (W > 1) bits[(size_t)i * W + 1] = (uint32_t)(bal >> 32);
        }
      } else {
        constexpr int G = 32 / CPL;   // lanes per 32-column word
        uint32_t word = nib << (CPL * (lane & (G - 1)));
#pragma unroll
        for (int o = 1; o < G; o <<= 1) word |= __shfl_xor(word, o, 64);
        if ((lane & (G - 1)) == 0 && lane / G < W) bits[(size_t)i * W + lane / G] = word;
      }
    }
#pragma unroll
    for (int r = 0; r < MAS_WAVE_R; ++r)
#pragma unroll
      for (int c = 0; c < CPL; ++c) cur[r][c] = nxt[r][c];
  }
  __syncthreads();
  if (lane == 0) mas_backtrack(bits, cnt, hard, b, n, m, T, L, W);
  __syncthreads();
  for (int j = lane; j < L; j += 64) dur[(size_t)b * L + j] = (float)cnt[j];
}

// mas_width1 on the slice [:m, :n] of utterance blockIdx.x (m = out_lens[b] frames, n = in_lens[b] phonemes).  Thread tid owns columns
// tid, tid + 256, ... (MAS_COLS of them at most); the next frame's values are loaded before the current frame is combined.  The back-pointer
// of a cell is ONE bit (1 = came from column j - 1), gathered per wavefront by a ballot and written by its first lane: bits[i][j / 32].
// `hard` (optional) was zeroed by the host.  cnt[j] counts the marks of column j = attn_hard.sum over frames.
__global__ __launch_bounds__(MAS_THREADS) void aln_mas_kernel(const float* __restrict__ map, int is_log, const int32_t* __restrict__ in_lens,
                                                              const int32_t* __restrict__ out_lens, uint32_t* bits_ws, int bits_in_lds,
                                                              float* hard, float* __restrict__ dur, int T, int L, int W) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mas_smem[];
  float* pp = (float*)mas_smem;   // [L] previous log_p row
  float* pc = pp + L;             // [L] row being written
  int* cnt = (int*)(pc + L);      // [L]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = in_lens[b], m = out_lens[b];
  const float* a = map + (size_t)b * T * L;
  uint32_t* bits = bits_in_lds ? mas_smem + 3 * (size_t)L : bits_ws + (size_t)b * T * W;
  for (int j = tid; j < L; j += MAS_THREADS) {
    cnt[j] = 0;
    if (j < n) {
      float v = -INFINITY;   // row 0: columns >= 1 are -inf
      if (j == 0) v = is_log ? a[0] : logf(a[0]);
      pp[j] = v;
    }
  }
  float nx[MAS_COLS];
#pragma unroll
  for (int c = 0; c < MAS_COLS; ++c) {
    const int j = tid + c * MAS_THREADS;
    nx[c] = (j < n && 1 < m) ? a[(size_t)L + j] : 1.f;
  }
  __syncthreads();
  for (int i = 1; i < m; ++i) {
    float cur[MAS_COLS];
#pragma unroll
    for (int c = 0; c < MAS_COLS; ++c) {
      cur[c] = nx[c];
      const int j = tid + c * MAS_THREADS;
      nx[c] = (j < n && i + 1 < m) ? a[(size_t)(i + 1) * L + j] : 1.f;
    }
#pragma unroll
    for (int c = 0; c < MAS_COLS; ++c) {
      if (c * MAS_THREADS >= n) break;   // workgroup-uniform: every lane of a wavefront reaches the ballot
      const int j = tid + c * MAS_THREADS;
      bool diag = false;
      if (j < n) {
        float p = pp[j];
        if (j >= 1) {
          const float pd = pp[j - 1];
          if (pd >= p) {   // the reference's >= : ties, -inf ties included, take the diagonal
            p = pd;
            diag = true;
          }
        }
        pc[j] = (is_log ? cur[c] : logf(cur[c])) + p;
      }
      const unsigned long long bal = __ballot(diag);
      if ((tid & 63) == 0) {
        const int w = j >> 5;   // j is a multiple of 64 here
        if (w < W) bits[(size_t)i * W + w] = (uint32_t)bal;
        if (w + 1 < W) bits[(size_t)i * W + w + 1] = (uint32_t)(bal >> 32);
      }
    }
    __syncthreads();
    float* t = pp;
    pp = pc;
    pc = t;
  }
  if (tid == 0) mas_backtrack(bits, cnt, hard, b, n, m, T, L, W);
  __syncthreads();
  for (int j = tid; j < L; j += MAS_THREADS) dur[(size_t)b * L + j] = (float)cnt[j];
}

thread_local std::string g_create_error;

}  // namespace

struct e2ealign_handle : Handle {
  int n_mel = 0, n_att = 0, n_text = 0;
  float temperature = 0.f;
  // weights: one HBM image, pointers into it
  Buf blob{this, Buf::WEIGHTS};
  bool loaded = false;
  const float *k0w = nullptr, *k0b = nullptr, *k2w = nullptr, *k2b = nullptr, *q0w = nullptr, *q0b = nullptr, *q2w = nullptr, *q2b = nullptr,
              *q4w = nullptr, *q4b = nullptr, *kspkw = nullptr, *qspkw = nullptr;
  // workspaces
  Buf kx{this}, ky{this}, kenc{this}, qx{this}, qy{this}, spk{this}, kspk{this}, qspk{this}, prior{this}, attn{this}, logp{this}, hard{this}, dur{this},
      bits{this}, map{this}, lens_txt{this}, lens_in{this}, lens_out{this};
  std::vector<int32_t> host_txt, host_in, host_out;   // int32 images of the length arrays: they outlive the asynchronous copies of a call
  int rB = 0, rT = 0, rL = 0;   // geometry of the resident attn / attn_logprob (0: nothing resident)
};

namespace {

int check_lens(e2ealign_handle* h, const std::vector<int64_t>& v, long long hi, const char* name, const char* hi_name) {
  const int64_t b = pp::first_bad_len(v.data(), (int64_t)v.size(), hi);
  if (b >= 0)
    return h->fail(E2EALIGN_EINVAL, std::string(name) + "[" + std::to_string(b) + "] = " + std::to_string((long long)v[b]) + " outside [1, " + hi_name +
                                        " = " + std::to_string(hi) + "]");
  return E2EALIGN_OK;
}

int check_dims(e2ealign_handle* h, int B, int T, int L) {
  if (B < 1 || T < 1 || L < 1) return h->fail(E2EALIGN_EINVAL, "B, T and L must be positive (got " + std::to_string(B) + ", " + std::to_string(T) + ", " + std::to_string(L) + ")");
  if (B > E2EALIGN_MAX_B) return h->fail(E2EALIGN_EINVAL, "B > " + std::to_string(E2EALIGN_MAX_B));
  if (L > E2EALIGN_MAX_L) return h->fail(E2EALIGN_EINVAL, "L > " + std::to_string(E2EALIGN_MAX_L));
  if ((long long)T * L >= (1LL << 28)) return h->fail(E2EALIGN_EINVAL, "one utterance's map (T * L) must stay below 2^28 cells");
  if ((long long)B * T * L >= (1LL << 33)) return h->fail(E2EALIGN_EINVAL, "B * T * L too large");
  return E2EALIGN_OK;
}

size_t attn_lds_bytes(int TI, int L, int C) { return ((size_t)TI * C + 64 * (size_t)(C | 1) + (size_t)TI * L) * 4; }

// `host` belongs to the handle and is rewritten by the next call only, after this call's stream has drained (begin_call): no wait here
int upload_lens(e2ealign_handle* h, Buf& dst, std::vector<int32_t>& host, const std::vector<int64_t>& v) {
  host.assign(v.begin(), v.end());
  RET(reserve(h, dst, host.size() * 4));
  HIPCHK(h, hipMemcpyAsync(dst.p, host.data(), host.size() * 4, hipMemcpyHostToDevice, h->stream));
  return E2EALIGN_OK;
}

ConvParams conv(const float* in, const float* w, const float* bias, float* out, int B, int N, int Cin, int Cout, int KW, int act) {
  ConvParams p;
  p.in = in; p.w = w; p.bias = bias; p.out = out;
  p.B = B; p.T = N; p.Cin = Cin; p.Cout = Cout; p.KW = KW; p.dil = 1; p.pad = (KW - 1) / 2;
  p.in_ld = Cin; p.out_ld = Cout;
  p.in_bs = (long long)N * Cin; p.out_bs = (long long)N * Cout;
  p.x3 = 0;   // exact fp32
  p.act = act;
  return p;
}

// validated arguments of a forward
struct FwdArgs {
  const float *mel, *keys, *speaker, *prior;
  const std::vector<int64_t>* txt_lens;   // null: no mask
  int B, T, L;
  const std::vector<int64_t>* gen_mel_lens = nullptr;   // not null: the prior is generated from txt_lens, these and gen_scaling (`prior` is NULL)
  double gen_scaling = 0.0;
};

int check_attention_tile(e2ealign_handle* h, int L) {
  if (attn_lds_bytes(4, L, h->n_att) > ATTN_LDS_MAX) return h->fail(E2EALIGN_EINVAL, "L * n_att too large for the attention pass's LDS tile");
  return E2EALIGN_OK;
}

int check_forward(e2ealign_handle* h, const FwdArgs& a) {
  RET(check_dims(h, a.B, a.T, a.L));
  if (!a.mel || !a.keys) return h->fail(E2EALIGN_EINVAL, "mel and keys must not be NULL");
  if (!h->loaded) return h->fail(E2EALIGN_ESTATE, "e2ealign_forward before e2ealign_load_weights");
  // what launch_conv_gemm would refuse (32-bit offsets inside one utterance; widths and alignment are settled by e2ealign_create and the
  // 256-byte aligned buffers): refused here, so that no launcher can object once copies are enqueued
  if ((long long)a.T * 2 * h->n_mel * 4 >= (1LL << 31) || (long long)a.L * 2 * h->n_text * 4 >= (1LL << 31))
    return h->fail(E2EALIGN_EINVAL, "one utterance's widest projection (T * 2 n_mel or L * 2 n_text floats) must stay below 2 GiB");
  return check_attention_tile(h, a.L);
}

// The checks of a generated prior's arguments (prior_plan.h), lengths fetched to the host: what e2ealign_prior and the *_bb entry points
// refuse before they look at anything else.
int check_prior_args(e2ealign_handle* h, const int64_t* txt_lens, const int64_t* mel_lens, int B, int T, int L, double scaling, std::vector<int64_t>& tl,
                     std::vector<int64_t>& ml) {
  if (const char* m = pp::check_shape(B, T, L)) return h->fail(E2EALIGN_EINVAL, m);
  if (!txt_lens || !mel_lens) return h->fail(E2EALIGN_EINVAL, "txt_lens and mel_lens must not be NULL");
  if (const char* m = pp::check_scaling(scaling)) return h->fail(E2EALIGN_EINVAL, m);
  RET(fetch_host(h, txt_lens, B, tl));
  RET(check_lens(h, tl, L, "txt_lens", "L"));
  RET(fetch_host(h, mel_lens, B, ml));
  return check_lens(h, ml, T, "mel_lens", "T");
}

// What the kernels that generate the prior need besides txt_lens, which the caller has uploaded to lens_txt: mel_lens on the device (in
// lens_out, where the search puts them too) and the column table.  The table lives in `ky`, the key projection's intermediate: a forward
// has finished with that buffer when the attention pass starts, so generating the prior holds no memory of its own.
int prepare_prior_gen(e2ealign_handle* h, const std::vector<int64_t>& mel_lens, double scaling, int B, int L, PriorGen& gen) {
  RET(upload_lens(h, h->lens_out, h->host_out, mel_lens));
  const size_t n = pp::col_table_doubles(B, L);
  RET(reserve(h, h->ky, n * sizeof(double)));
  hipLaunchKernelGGL(aln_prior_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const int32_t*)h->lens_txt.p, (double*)h->ky.p, B, L);
  HIPCHK(h, hipGetLastError());
  gen = PriorGen{(const double*)h->ky.p, (const int32_t*)h->lens_out.p, scaling};
  return E2EALIGN_OK;
}

// The attention pass on device q [B, T, n_att] and k [B, L, n_att] into the handle's attn / attn_logprob: the ONE place that chooses the frame
// tile (16 frames per workgroup while the tile fits the LDS limit, 4 otherwise; check_attention_tile has refused what 4 cannot hold).
// run_forward and the test build's e2ealign_debug_attention / _bb launch through it.  `gen` (not null: `prior` is) selects the
// generated-prior form.
int launch_attention(e2ealign_handle* h, const float* q, const float* k, const float* prior, const int32_t* lens, int B, int T, int L,
                     const PriorGen* gen = nullptr) {
  const int A = h->n_att;
  hipStream_t s = h->stream;
  const PriorGen g = gen ? *gen : PriorGen{nullptr, nullptr, 0.0};
#define ALN_ATTN(FPT, GEN)                                                                                                                              \
  hipLaunchKernelGGL((aln_attn_kernel<FPT, GEN>), dim3((T + 4 * FPT - 1) / (4 * FPT), B), dim3(256), attn_lds_bytes(4 * FPT, L, A), s, q, k, prior, lens, \
                     (float*)h->attn.p, (float*)h->logp.p, T, L, A, h->temperature, g)
  if (attn_lds_bytes(16, L, A) <= ATTN_LDS_MAX) {
    if (gen) ALN_ATTN(4, true);
    else ALN_ATTN(4, false);
  } else {
    if (gen) ALN_ATTN(1, true);
    else ALN_ATTN(1, false);
  }
#undef ALN_ATTN
  HIPCHK(h, hipGetLastError());
  return E2EALIGN_OK;
}

int run_forward(e2ealign_handle* h, const FwdArgs& a) {
  const int B = a.B, T = a.T, L = a.L, M = h->n_mel, H = h->n_text, A = h->n_att;
  const size_t BTL = (size_t)B * T * L;
  h->rB = h->rT = h->rL = 0;
  RET(reserve(h, h->kx, (size_t)B * L * H * 4));
  RET(reserve(h, h->ky, (size_t)B * L * 2 * H * 4));
  RET(reserve(h, h->kenc, (size_t)B * L * A * 4));
  RET(reserve(h, h->qx, (size_t)B * T * M * 4));
  RET(reserve(h, h->qy, (size_t)B * T * (2 * M > A ? 2 * M : A) * 4));
  RET(reserve(h, h->attn, BTL * 4));
  RET(reserve(h, h->logp, BTL * 4));
  if (a.txt_lens) RET(upload_lens(h, h->lens_txt, h->host_txt, *a.txt_lens));
  const float* prior = nullptr;
  if (a.prior) {
    if (is_device_pointer(a.prior)) {
      prior = a.prior;
    } else {
      RET(reserve(h, h->prior, BTL * 4));
      HIPCHK(h, hipMemcpyAsync(h->prior.p, a.prior, BTL * 4, hipMemcpyDefault, h->stream));
      prior = (const float*)h->prior.p;
    }
  }
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->kx.p, a.keys, (size_t)B * L * H * 4, hipMemcpyDefault, s));
  HIPCHK(h, hipMemcpyAsync(h->qx.p, a.mel, (size_t)B * T * M * 4, hipMemcpyDefault, s));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[0], s));
  float *kx = (float*)h->kx.p, *ky = (float*)h->ky.p, *kenc = (float*)h->kenc.p, *qx = (float*)h->qx.p, *qy = (float*)h->qy.p;
  if (a.speaker) {
    RET(reserve(h, h->spk, (size_t)B * H * 4));
    RET(reserve(h, h->kspk, (size_t)B * H * 4));
    RET(reserve(h, h->qspk, (size_t)B * M * 4));
    HIPCHK(h, hipMemcpyAsync(h->spk.p, a.speaker, (size_t)B * H * 4, hipMemcpyDefault, s));
    // LinearNorm without bias on the B speaker vectors (one "utterance" of B rows), then added to every position
    KCHK(h, launch_conv_gemm(conv((const float*)h->spk.p, h->kspkw, nullptr, (float*)h->kspk.p, 1, B, H, H, 1, ACT_NONE), s));
    KCHK(h, launch_conv_gemm(conv((const float*)h->spk.p, h->qspkw, nullptr, (float*)h->qspk.p, 1, B, H, M, 1, ACT_NONE), s));
    const long long nk = (long long)B * L * H, nq = (long long)B * T * M;
    hipLaunchKernelGGL(aln_add_rows_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, kx, (const float*)h->kspk.p, B, L, H);
    hipLaunchKernelGGL(aln_add_rows_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, qx, (const float*)h->qspk.p, B, T, M);
  }
  // key_proj: conv k = 3 (H -> 2H), ReLU, conv k = 1 (2H -> n_att); query_proj: conv k = 3 (M -> 2M), ReLU, 1x1 (2M -> M), ReLU, 1x1 (M -> n_att)
  KCHK(h, launch_conv_gemm(conv(kx, h->k0w, h->k0b, ky, B, L, H, 2 * H, 3, ACT_RELU), s));
  KCHK(h, launch_conv_gemm(conv(ky, h->k2w, h->k2b, kenc, B, L, 2 * H, A, 1, ACT_NONE), s));
  KCHK(h, launch_conv_gemm(conv(qx, h->q0w, h->q0b, qy, B, T, M, 2 * M, 3, ACT_RELU), s));
  KCHK(h, launch_conv_gemm(conv(qy, h->q2w, h->q2b, qx, B, T, 2 * M, M, 1, ACT_RELU), s));
  KCHK(h, launch_conv_gemm(conv(qx, h->q4w, h->q4b, qy, B, T, M, A, 1, ACT_NONE), s));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[1], s));
  const int32_t* lens = a.txt_lens ? (const int32_t*)h->lens_txt.p : nullptr;
  if (a.gen_mel_lens) {
    PriorGen gen;
    RET(prepare_prior_gen(h, *a.gen_mel_lens, a.gen_scaling, B, L, gen));   // (ky is free: key_proj has been enqueued)
    RET(launch_attention(h, qy, kenc, nullptr, lens, B, T, L, &gen));
  } else {
    RET(launch_attention(h, qy, kenc, prior, lens, B, T, L));
  }
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[2], s));
  h->rB = B; h->rT = T; h->rL = L;
  return E2EALIGN_OK;
}

// the search on a DEVICE map; lengths already validated
int run_mas(e2ealign_handle* h, const float* dmap, int is_log, const std::vector<int64_t>& in_lens, const std::vector<int64_t>& out_lens, int B, int T,
            int L, bool want_hard) {
  const int W = (L + 31) / 32;
  RET(upload_lens(h, h->lens_in, h->host_in, in_lens));
  RET(upload_lens(h, h->lens_out, h->host_out, out_lens));
  RET(reserve(h, h->dur, (size_t)B * L * 4));
  RET(reserve(h, h->bits, (size_t)B * T * W * 4));
  hipStream_t s = h->stream;
  if (want_hard) {
    RET(reserve(h, h->hard, (size_t)B * T * L * 4));
    HIPCHK(h, hipMemsetAsync(h->hard.p, 0, (size_t)B * T * L * 4, s));
  }
  const bool wave = L <= MAS_WAVE_L;   // one wavefront per utterance, the row in registers; wider rows: one workgroup, the row in LDS
  size_t lds = (wave ? 1 : 3) * (size_t)L * 4;
  const size_t with_bits = lds + (size_t)T * W * 4;
  const int in_lds = with_bits <= MAS_LDS_BUDGET ? 1 : 0;
  if (in_lds) lds = with_bits;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[3], s));
#define ALN_MAS_WAVE(CPL)                                                                                                                              \
  hipLaunchKernelGGL(aln_mas_wave_kernel<CPL>, dim3(B), dim3(64), lds, s, dmap, is_log, (const int32_t*)h->lens_in.p, (const int32_t*)h->lens_out.p, \
                     (uint32_t*)h->bits.p, in_lds, want_hard ? (float*)h->hard.p : nullptr, (float*)h->dur.p, T, L, W)
  if (wave && L <= 64) ALN_MAS_WAVE(1);
  else if (wave && L <= 128) ALN_MAS_WAVE(2);
  else if (wave) ALN_MAS_WAVE(4);
#undef ALN_MAS_WAVE
  else
    hipLaunchKernelGGL(aln_mas_kernel, dim3(B), dim3(MAS_THREADS), lds, s, dmap, is_log, (const int32_t*)h->lens_in.p, (const int32_t*)h->lens_out.p,
                       (uint32_t*)h->bits.p, in_lds, want_hard ? (float*)h->hard.p : nullptr, (float*)h->dur.p, T, L, W);
  HIPCHK(h, hipGetLastError());
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[4], s));
  return E2EALIGN_OK;
}

// the profiled phases: projections (events 0, 1) and attention (1, 2) of a forward, the search (3, 4)
int finish(e2ealign_handle* h, bool fwd, bool mas) {
  const Phase none{-1, -1}, phases[3] = {fwd ? Phase{0, 1} : none, fwd ? Phase{1, 2} : none, mas ? Phase{3, 4} : none};
  return companion::finish(h, phases);
}

struct Want {
  const char* name;
  const float** dst;
  size_t numel;
};

}  // namespace

extern "C" {

const char* e2ealign_version(void) { return "e2etts-align 1 E2EALIGN_SRC_HASH=" E2EALIGN_SRC_HASH; }
int e2ealign_abi_version(void) { return E2EALIGN_ABI_VERSION; }

const char* e2ealign_last_error(const e2ealign_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int e2ealign_create(int device_id, int n_mel, int n_att, int n_text, float temperature, e2ealign_handle** out) {
  if (!out) {
    g_create_error = "out is NULL";
    return E2EALIGN_EINVAL;
  }
  *out = nullptr;
  if (device_id < 0 || n_mel < 4 || n_att < 1 || n_text < 4 || n_mel % 4 || n_text % 4 || n_att > E2EALIGN_MAX_ATT || n_mel > 4096 || n_text > 4096 ||
      !(temperature == temperature)) {
    g_create_error = "e2ealign_create: need device_id >= 0, n_mel and n_text positive multiples of 4 (<= 4096), 1 <= n_att <= " +
                     std::to_string(E2EALIGN_MAX_ATT) + " and a temperature that is a number (got n_mel " + std::to_string(n_mel) + ", n_att " +
                     std::to_string(n_att) + ", n_text " + std::to_string(n_text) + ")";
    return E2EALIGN_EINVAL;
  }
  e2ealign_handle* h = new (std::nothrow) e2ealign_handle();
  if (!h) {
    g_create_error = "out of host memory";
    return E2EALIGN_ENOMEM;
  }
  h->device = device_id;
  h->n_mel = n_mel; h->n_att = n_att; h->n_text = n_text;
  h->temperature = temperature;
  *out = h;
  return E2EALIGN_OK;
}

void e2ealign_destroy(e2ealign_handle* h) { companion::destroy(h); }

int e2ealign_load_weights(e2ealign_handle* h, const void* blob, size_t nbytes) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!blob) return h->fail(E2EALIGN_EINVAL, "blob is NULL");
  if (nbytes < sizeof(BlobHeader)) return h->fail(E2EALIGN_EINVAL, "weight blob too small");
  // header and directory on the host first (a device image is read back; nothing is enqueued until the directory holds every tensor)
  const bool dev = is_device_pointer(blob);
  BlobHeader hd;
  if (dev) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(&hd, blob, sizeof hd, hipMemcpyDefault));
  } else {
    memcpy(&hd, blob, sizeof hd);
  }
  if (const char* m = blob_check_header(hd, nbytes)) return h->fail(E2EALIGN_EINVAL, m);
  std::vector<BlobEntry> dir(hd.n_entries);
  if (hd.n_entries) {
    if (dev) HIPCHK(h, hipMemcpy(dir.data(), (const char*)blob + sizeof hd, dir.size() * sizeof(BlobEntry), hipMemcpyDefault));
    else memcpy(dir.data(), (const char*)blob + sizeof hd, dir.size() * sizeof(BlobEntry));
  }
  std::vector<BlobTensor> tensors;
  std::string bad;
  if (const char* m = blob_check_directory(hd, dir.data(), nbytes, tensors, bad)) return h->fail(E2EALIGN_EINVAL, std::string(m) + ": " + bad);
  const size_t M = h->n_mel, H = h->n_text, A = h->n_att;
  const float *k0w, *k0b, *k2w, *k2b, *q0w, *q0b, *q2w, *q2b, *q4w, *q4b, *kspkw, *qspkw;
  const Want wants[] = {
      {"aln.key.0.w", &k0w, 2 * H * 3 * H}, {"aln.key.0.b", &k0b, 2 * H},   {"aln.key.2.w", &k2w, A * 2 * H},   {"aln.key.2.b", &k2b, A},
      {"aln.query.0.w", &q0w, 2 * M * 3 * M}, {"aln.query.0.b", &q0b, 2 * M}, {"aln.query.2.w", &q2w, M * 2 * M}, {"aln.query.2.b", &q2b, M},
      {"aln.query.4.w", &q4w, A * M},       {"aln.query.4.b", &q4b, A},     {"aln.key_spk.w", &kspkw, H * H},   {"aln.query_spk.w", &qspkw, M * H},
  };
  uint64_t offs[sizeof wants / sizeof wants[0]];
  for (size_t i = 0; i < sizeof wants / sizeof wants[0]; ++i) {
    const BlobTensor* t = nullptr;
    for (const auto& x : tensors)
      if (x.name == wants[i].name) t = &x;
    if (!t) return h->fail(E2EALIGN_EINVAL, std::string("weight blob has no tensor '") + wants[i].name + "'");
    if (t->numel != wants[i].numel)
      return h->fail(E2EALIGN_EINVAL, std::string("tensor '") + wants[i].name + "' has " + std::to_string(t->numel) + " elements, this aligner's dims need " +
                                          std::to_string(wants[i].numel));
    offs[i] = t->offset;
  }
  RET(open_device(h));
  RET(reserve(h, h->blob, nbytes));
  HIPCHK(h, hipMemcpyAsync(h->blob.p, blob, nbytes, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < sizeof wants / sizeof wants[0]; ++i) *wants[i].dst = (const float*)((const char*)h->blob.p + offs[i]);
  h->k0w = k0w; h->k0b = k0b; h->k2w = k2w; h->k2b = k2b; h->q0w = q0w; h->q0b = q0b; h->q2w = q2w; h->q2b = q2b; h->q4w = q4w; h->q4b = q4b;
  h->kspkw = kspkw; h->qspkw = qspkw;
  h->loaded = true;
  return E2EALIGN_OK;
}

void* e2ealign_stream(e2ealign_handle* h) { return companion::stream(h); }
int e2ealign_order_after(e2ealign_handle* h, void* caller_stream) { return companion::order_after(h, caller_stream); }
int e2ealign_sync(e2ealign_handle* h) { return companion::sync(h); }
size_t e2ealign_device_bytes(const e2ealign_handle* h) { return companion::device_bytes(h); }

int e2ealign_forward(e2ealign_handle* h, const float* mel, const float* keys, const float* speaker, const int64_t* txt_lens, const float* prior, int B,
                     int T, int L, float* attn_out, float* attn_logprob_out) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<int64_t> tl;
  FwdArgs a{mel, keys, speaker, prior, nullptr, B, T, L};
  RET(check_forward(h, a));
  if (txt_lens) {
    RET(fetch_host(h, txt_lens, B, tl));
    RET(check_lens(h, tl, L, "txt_lens", "L"));
    a.txt_lens = &tl;
  }
  RET(begin_call(h));
  RET(run_forward(h, a));
  const size_t n = (size_t)B * T * L * 4;
  RET(copy_out(h, attn_out, h->attn.p, n));
  RET(copy_out(h, attn_logprob_out, h->logp.p, n));
  return finish(h, true, false);
}

int e2ealign_mas(e2ealign_handle* h, const float* map, int flags, const int64_t* in_lens, const int64_t* out_lens, int B, int T, int L,
                 float* attn_hard_out, float* dur_out) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(check_dims(h, B, T, L));
  if (flags & ~E2EALIGN_LOG_MAP) return h->fail(E2EALIGN_EINVAL, "unknown flag bits");
  if (!in_lens || !out_lens) return h->fail(E2EALIGN_EINVAL, "in_lens and out_lens must not be NULL");
  if (!map) {
    if (!h->rB) return h->fail(E2EALIGN_EINVAL, "map is NULL and no attn is resident (no e2ealign_forward has completed)");
    if (h->rB != B || h->rT != T || h->rL != L)
      return h->fail(E2EALIGN_EINVAL, "map is NULL and (B, T, L) differ from the resident attn's (" + std::to_string(h->rB) + ", " + std::to_string(h->rT) + ", " +
                                          std::to_string(h->rL) + ")");
    if (flags & E2EALIGN_LOG_MAP) return h->fail(E2EALIGN_EINVAL, "the resident attn is a probability map: E2EALIGN_LOG_MAP does not apply");
  }
  std::vector<int64_t> il, ol;
  RET(fetch_host(h, in_lens, B, il));
  RET(check_lens(h, il, L, "in_lens", "L"));
  RET(fetch_host(h, out_lens, B, ol));
  RET(check_lens(h, ol, T, "out_lens", "T"));
  RET(begin_call(h));
  const size_t n = (size_t)B * T * L * 4;
  const float* dmap = (const float*)h->attn.p;
  if (map) {
    if (is_device_pointer(map)) {
      dmap = map;
    } else {
      RET(reserve(h, h->map, n));
      HIPCHK(h, hipMemcpyAsync(h->map.p, map, n, hipMemcpyDefault, h->stream));
      dmap = (const float*)h->map.p;
    }
  }
  RET(run_mas(h, dmap, (flags & E2EALIGN_LOG_MAP) ? 1 : 0, il, ol, B, T, L, attn_hard_out != nullptr));
  RET(copy_out(h, attn_hard_out, h->hard.p, n));
  RET(copy_out(h, dur_out, h->dur.p, (size_t)B * L * 4));
  return finish(h, false, true);
}

int e2ealign_align(e2ealign_handle* h, const float* mel, const float* keys, const float* speaker, const int64_t* txt_lens, const int64_t* mel_lens,
                   const float* prior, int B, int T, int L, float* dur_out, float* attn_hard_out, float* attn_out, float* attn_logprob_out) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<int64_t> tl, ml;
  FwdArgs a{mel, keys, speaker, prior, &tl, B, T, L};
  RET(check_forward(h, a));
  if (!txt_lens || !mel_lens) return h->fail(E2EALIGN_EINVAL, "txt_lens and mel_lens must not be NULL");
  RET(fetch_host(h, txt_lens, B, tl));
  RET(check_lens(h, tl, L, "txt_lens", "L"));
  RET(fetch_host(h, mel_lens, B, ml));
  RET(check_lens(h, ml, T, "mel_lens", "T"));
  RET(begin_call(h));
  RET(run_forward(h, a));
  RET(run_mas(h, (const float*)h->attn.p, 0, tl, ml, B, T, L, attn_hard_out != nullptr));
  const size_t n = (size_t)B * T * L * 4;
  RET(copy_out(h, dur_out, h->dur.p, (size_t)B * L * 4));
  RET(copy_out(h, attn_hard_out, h->hard.p, n));
  RET(copy_out(h, attn_out, h->attn.p, n));
  RET(copy_out(h, attn_logprob_out, h->logp.p, n));
  return finish(h, true, true);
}

int e2ealign_prior(e2ealign_handle* h, const int64_t* txt_lens, const int64_t* mel_lens, int B, int T, int L, double scaling, float* prior_out) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<int64_t> tl, ml;
  RET(check_prior_args(h, txt_lens, mel_lens, B, T, L, scaling, tl, ml));
  if (!prior_out) return h->fail(E2EALIGN_EINVAL, "prior_out must not be NULL");
  RET(begin_call(h));
  const size_t n = (size_t)B * T * L * 4;
  float* dst = prior_out;
  if (!is_device_pointer(prior_out)) {
    RET(reserve(h, h->prior, n));
    dst = (float*)h->prior.p;
  }
  RET(upload_lens(h, h->lens_txt, h->host_txt, tl));
  PriorGen gen;
  RET(prepare_prior_gen(h, ml, scaling, B, L, gen));
  hipLaunchKernelGGL(aln_prior_kernel, dim3(pp::frame_groups(T), B), dim3(256), 0, h->stream, (const int32_t*)h->lens_txt.p, gen, dst, T, L);
  HIPCHK(h, hipGetLastError());
  if (dst != prior_out) RET(copy_out(h, prior_out, dst, n));
  return finish(h, false, false);
}

int e2ealign_forward_bb(e2ealign_handle* h, const float* mel, const float* keys, const float* speaker, const int64_t* txt_lens, const int64_t* mel_lens,
                        double scaling, int B, int T, int L, float* attn_out, float* attn_logprob_out) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<int64_t> tl, ml;
  RET(check_prior_args(h, txt_lens, mel_lens, B, T, L, scaling, tl, ml));
  FwdArgs a{mel, keys, speaker, nullptr, &tl, B, T, L, &ml, scaling};
  RET(check_forward(h, a));
  RET(begin_call(h));
  RET(run_forward(h, a));
  const size_t n = (size_t)B * T * L * 4;
  RET(copy_out(h, attn_out, h->attn.p, n));
  RET(copy_out(h, attn_logprob_out, h->logp.p, n));
  return finish(h, true, false);
}

int e2ealign_align_bb(e2ealign_handle* h, const float* mel, const float* keys, const float* speaker, const int64_t* txt_lens, const int64_t* mel_lens,
                      double scaling, int B, int T, int L, float* dur_out, float* attn_hard_out, float* attn_out, float* attn_logprob_out) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<int64_t> tl, ml;
  RET(check_prior_args(h, txt_lens, mel_lens, B, T, L, scaling, tl, ml));
  FwdArgs a{mel, keys, speaker, nullptr, &tl, B, T, L, &ml, scaling};
  RET(check_forward(h, a));
  RET(begin_call(h));
  RET(run_forward(h, a));
  RET(run_mas(h, (const float*)h->attn.p, 0, tl, ml, B, T, L, attn_hard_out != nullptr));
  const size_t n = (size_t)B * T * L * 4;
  RET(copy_out(h, dur_out, h->dur.p, (size_t)B * L * 4));
  RET(copy_out(h, attn_hard_out, h->hard.p, n));
  RET(copy_out(h, attn_out, h->attn.p, n));
  RET(copy_out(h, attn_logprob_out, h->logp.p, n));
  return finish(h, true, true);
}

int e2ealign_profile_enable(e2ealign_handle* h, int on) { return companion::profile_enable(h, on); }
int e2ealign_profile_read(e2ealign_handle* h, double ms_out[3]) { return companion::profile_read(h, ms_out); }

#ifdef E2EALIGN_TEST_HOOKS
int e2ealign_debug_poison_workspace(e2ealign_handle* h) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(poison_workspaces(h));
  h->rB = h->rT = h->rL = 0;
  return E2EALIGN_OK;
}

int e2ealign_debug_attention(e2ealign_handle* h, const float* q, const float* k, const float* prior, const int64_t* txt_lens, int B, int T, int L,
                             float* attn_out, float* attn_logprob_out) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(check_dims(h, B, T, L));
  if (!q || !k) return h->fail(E2EALIGN_EINVAL, "q and k must not be NULL");
  RET(check_attention_tile(h, L));
  std::vector<int64_t> tl;
  if (txt_lens) {
    RET(fetch_host(h, txt_lens, B, tl));
    RET(check_lens(h, tl, L, "txt_lens", "L"));
  }
  RET(begin_call(h));
  const size_t A = h->n_att, n = (size_t)B * T * L * 4;
  h->rB = h->rT = h->rL = 0;
  RET(reserve(h, h->qy, (size_t)B * T * A * 4));
  RET(reserve(h, h->kenc, (size_t)B * L * A * 4));
  RET(reserve(h, h->attn, n));
  RET(reserve(h, h->logp, n));
  if (txt_lens) RET(upload_lens(h, h->lens_txt, h->host_txt, tl));
  const float* dprior = nullptr;
  if (prior) {
    RET(reserve(h, h->prior, n));
    HIPCHK(h, hipMemcpyAsync(h->prior.p, prior, n, hipMemcpyDefault, h->stream));
    dprior = (const float*)h->prior.p;
  }
  HIPCHK(h, hipMemcpyAsync(h->qy.p, q, (size_t)B * T * A * 4, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->kenc.p, k, (size_t)B * L * A * 4, hipMemcpyDefault, h->stream));
  RET(launch_attention(h, (const float*)h->qy.p, (const float*)h->kenc.p, dprior, txt_lens ? (const int32_t*)h->lens_txt.p : nullptr, B, T, L));
  h->rB = B; h->rT = T; h->rL = L;
  RET(copy_out(h, attn_out, h->attn.p, n));
  RET(copy_out(h, attn_logprob_out, h->logp.p, n));
  return finish(h, false, false);
}

int e2ealign_debug_attention_bb(e2ealign_handle* h, const float* q, const float* k, const int64_t* txt_lens, const int64_t* mel_lens, double scaling,
                                int B, int T, int L, float* attn_out, float* attn_logprob_out) {
  if (!h) return E2EALIGN_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<int64_t> tl, ml;
  RET(check_prior_args(h, txt_lens, mel_lens, B, T, L, scaling, tl, ml));
  if (!q || !k) return h->fail(E2EALIGN_EINVAL, "q and k must not be NULL");
  RET(check_attention_tile(h, L));
  RET(begin_call(h));
  const size_t A = h->n_att, n = (size_t)B * T * L * 4;
  h->rB = h->rT = h->rL = 0;
  RET(reserve(h, h->qy, (size_t)B * T * A * 4));
  RET(reserve(h, h->kenc, (size_t)B * L * A * 4));
  RET(reserve(h, h->attn, n));
  RET(reserve(h, h->logp, n));
  RET(upload_lens(h, h->lens_txt, h->host_txt, tl));
  PriorGen gen;
  RET(prepare_prior_gen(h, ml, scaling, B, L, gen));
  HIPCHK(h, hipMemcpyAsync(h->qy.p, q, (size_t)B * T * A * 4, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->kenc.p, k, (size_t)B * L * A * 4, hipMemcpyDefault, h->stream));
  RET(launch_attention(h, (const float*)h->qy.p, (const float*)h->kenc.p, nullptr, (const int32_t*)h->lens_txt.p, B, T, L, &gen));
  h->rB = B; h->rT = T; h->rL = L;
  RET(copy_out(h, attn_out, h->attn.p, n));
  RET(copy_out(h, attn_logprob_out, h->logp.p, n));
  return finish(h, false, false);
}
#endif

}  // extern "C"
