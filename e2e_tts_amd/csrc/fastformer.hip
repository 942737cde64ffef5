// Additive attention of the Fastformer block (reference U/blocks/fastformer.py:218-267): the part the GEMM kernels have no form for.
//
// FastAttention pools the sequence twice per layer.  With v = q (first pool) or v = k * pooled_query (second pool), per (batch row b, head h):
//     s[n]   = fl(fl((v[n, :] . W[h, :] + bias[h]) / sqrt(head_size)) + mask_term[n])        (:232-234, :250-253)
//     w[n]   = softmax over the N positions of s                                             (:237, :256)
//     out[h] = sum_n w[n] * v[n, h * head_size .. (h + 1) * head_size)                       (:243, :259)
// The logit layer is a dense Linear(H -> heads), the heads are hidden / n_head slices of n_head values (heads and head size are swapped,
// :152,190-191: 192 heads of size 2 at the shipped size), and the mask term is INVERTED (:223-225): -10000 is added at VALID positions
// (n < lens[b]) and 0 at padded ones, so in a padded row of the batch practically all the weight lies on the padding and every one of the
// N positions takes part; nothing may be skipped.  The -10000 shift also rounds the logit of a valid position to fp32's grid at 1e4
// (2^-10) before the softmax, which is why the two steps above are kept in the reference's order and in fp32 in every precision mode.
//
// ff_pool_partial_kernel: ONE pass over v.  A workgroup owns a run of rows of one utterance and walks it in tiles of 16 rows staged in
// LDS (the second pool forms k * pooled_query while staging: no [B, N, H] product tensor).  The logits of a tile are a [16 x H] . [H x heads]
// product: thread (rp, head) computes its head's logits of 16 / RP rows, each as ONE k-ordered fmaf chain over all H channels -- the
// weights travel transposed, [H][heads], so a wavefront reads consecutive words, and the row values come from LDS as broadcast reads --
// and leaves them in LDS; thread (0, head) applies the division and the shift and folds the 16 rows into its head's running (max, sum,
// weighted sum) in row order.  The chain is never split along K: a logit summed in another order differs in its last bits, lands on
// the other side of a 2^-10 rounding step of the shift that much more often, and a K split four ways inside the workgroup measured
// 8 x the distance to the reference on the tiny fixtures (dec_out mean-L1 1.2e-5 against 1.6e-6).  Parallelism comes from the rows:
// RP = 4 for small launches (the B = 1 latency path: 4 rows per thread, 12 wavefronts per workgroup at 192 heads), RP = 2 for big ones
// (twice the FMAs per weight word).  Same bits for every RP.
// Logits by FMA, not MFMA: they must be exact fp32, and on gfx950 the fp32 MFMA issues at the vector unit's rate (64 FLOP/clk/SIMD
// either way), so the matrix pipe would buy operand bandwidth only, at the price of a C-layout shuffle between the logits and the
// per-head running state.
// N is split over workgroups so that B = 1 fills the chip; ff_pool_merge_kernel then merges the partial triples of a (b, head) in
// split order -- fixed by the shape alone, no atomics: the result is bit-identical from run to run.
#include <math.h>

#include <algorithm>

#include "kernels.h"

namespace e2etts {
namespace {

constexpr int FF_MAX_THREADS = 1024;
constexpr int FF_MAX_HEADS = 512;
constexpr int FF_TARGET_WG = 1024;
constexpr size_t FF_MAX_LDS = 65536;

// MAXT: the workgroup size the instantiation is compiled for (512: 256 VGPRs per lane, the k loop unrolled four times; 1024: 128 VGPRs)
template <int HS, int R, int RP, int MAXT>
__global__ __launch_bounds__(MAXT) void ff_pool_partial_kernel(const float* __restrict__ v, int v_ld, const float* __restrict__ scale,
                                                                         const float* __restrict__ wl, const float* __restrict__ bl,
                                                                         const int32_t* __restrict__ lens, float* __restrict__ part, int N, int H,
                                                                         int NH, int rows_per_wg, int nsplit, float div) {
  extern __shared__ __attribute__((aligned(16))) char ff_smem[];
  float* vt = reinterpret_cast<float*>(ff_smem);  // [R][H]
  float* pl = vt + R * H;                         // [R][NH] logits (RP > 1)
  constexpr int RR = R / RP;                      // rows per thread
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int b = blockIdx.y, sp = blockIdx.x;
  const int n_begin = sp * rows_per_wg;
  const int n_end = min(N, n_begin + rows_per_wg);
  const int len = lens ? max(0, min(lens[b], N)) : N;
  const int H4 = H >> 2;
  const int rp = tid / NH, h = tid - rp * NH;
  const bool active = rp < RP;
  const float* vb = v + (long long)b * N * v_ld;
  const float4* sc4 = scale ? reinterpret_cast<const float4*>(scale + (long long)b * H) : nullptr;

  float m = -INFINITY, l = 0.f, a[HS];
#pragma unroll
  for (int d = 0; d < HS; ++d) a[d] = 0.f;

  for (int n0 = n_begin; n0 < n_end; n0 += R) {
    __syncthreads();  // the previous tile (and its logits) has been consumed
    for (int i = tid; i < R * H4; i += nthreads) {
      const int r = i / H4, c4 = i - r * H4;
      const int n = n0 + r;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n < n_end) {
        x = *reinterpret_cast<const float4*>(vb + (long long)n * v_ld + c4 * 4);
        if (sc4) {  // mixed_key_layer * pooled_query (:248), rounded once as there
          const float4 g = sc4[c4];
          x.x *= g.x; x.y *= g.y; x.z *= g.z; x.w *= g.w;
        }
      }
      reinterpret_cast<float4*>(vt)[i] = x;
    }
    __syncthreads();
    float acc[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) acc[r] = 0.f;
    if (active) {
      constexpr int U = MAXT > 512 ? 2 : 4;   // weight loads in flight per lane: 4 U (more spills at 128 VGPRs)
      const float* vr = vt + rp * RR * H;
#pragma unroll U
      for (int c = 0; c < H; c += 4) {
        const float w0 = wl[(long long)(c + 0) * NH + h], w1 = wl[(long long)(c + 1) * NH + h];
        const float w2 = wl[(long long)(c + 2) * NH + h], w3 = wl[(long long)(c + 3) * NH + h];
#pragma unroll
        for (int r = 0; r < RR; ++r) {
          const float4 x = *reinterpret_cast<const float4*>(vr + r * H + c);
          acc[r] = fmaf(x.x, w0, acc[r]);
          acc[r] = fmaf(x.y, w1, acc[r]);
          acc[r] = fmaf(x.z, w2, acc[r]);
          acc[r] = fmaf(x.w, w3, acc[r]);
        }
      }
    }
    float lg[R];
    if constexpr (RP > 1) {
      if (active) {
#pragma unroll
        for (int r = 0; r < RR; ++r) pl[(rp * RR + r) * NH + h] = acc[r];
      }
      __syncthreads();
      if (rp == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) lg[r] = pl[r * NH + h];
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) lg[r] = acc[r];
    }
    if (rp == 0) {
      const float bias = bl[h];
      float mt = -INFINITY;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int n = n0 + r;
        float s = (lg[r] + bias) / div;            // :232 / :250 (true division by fl32(sqrt(head_size)))
        s = s + (n < len ? -10000.0f : 0.0f);       // :223-225, :234, :253: the shift lands on the VALID positions
        lg[r] = n < n_end ? s : -INFINITY;         // rows past the run take no part
        mt = fmaxf(mt, lg[r]);
      }
      const float mn = fmaxf(m, mt);                // finite: every tile holds at least one row
      const float sc = expf(m - mn);                // first tile: exp(-inf) = 0
      l *= sc;
#pragma unroll
      for (int d = 0; d < HS; ++d) a[d] *= sc;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float p = expf(lg[r] - mn);
        l += p;
#pragma unroll
        for (int d = 0; d < HS; ++d) a[d] = fmaf(p, vt[r * H + h * HS + d], a[d]);
      }
      m = mn;
    }
  }
  if (rp == 0) {
    float* o = part + (((long long)b * nsplit + sp) * NH + h) * (HS + 2);
    o[0] = m;
    o[1] = l;
#pragma unroll
    for (int d = 0; d < HS; ++d) o[2 + d] = a[d];
  }
}

// out[b, h * HS + d] = (sum_s a_s[d] e^(m_s - M)) / (sum_s l_s e^(m_s - M)), s in split order
template <int HS>
__global__ __launch_bounds__(64) void ff_pool_merge_kernel(const float* __restrict__ part, float* __restrict__ out, int NH, int nsplit) {
  const int b = blockIdx.y;
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= NH) return;
  const float* p = part + ((long long)b * nsplit * NH + h) * (HS + 2);
  const long long step = (long long)NH * (HS + 2);
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, p[s * step]);
  float L = 0.f, A[HS];
#pragma unroll
  for (int d = 0; d < HS; ++d) A[d] = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* q = p + s * step;
    const float w = expf(q[0] - M);
    L = fmaf(q[1], w, L);
#pragma unroll
    for (int d = 0; d < HS; ++d) A[d] = fmaf(q[2 + d], w, A[d]);
  }
#pragma unroll
  for (int d = 0; d < HS; ++d) out[((long long)b * NH + h) * HS + d] = A[d] / L;
}

// wv[row, :] = gk[b, :] * q[row, :] (:262), qx[row, :] = q[row, :] + x[row, :] (the two residuals of the attention sub-block, :265 and :169)
__global__ __launch_bounds__(256) void ff_scale_kernel(const float* __restrict__ q, int q_ld, const float* __restrict__ gk,
                                                       const float* __restrict__ x, float* __restrict__ wv, float* __restrict__ qx,
                                                       long long total4, int N, int H4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long long row = i / H4;
  const int c4 = (int)(i - row * H4);
  const long long b = row / N;
  const float4 qv = *reinterpret_cast<const float4*>(q + row * q_ld + c4 * 4);
  const float4 g = reinterpret_cast<const float4*>(gk)[b * H4 + c4];
  const float4 xv = reinterpret_cast<const float4*>(x)[i];
  reinterpret_cast<float4*>(wv)[i] = make_float4(g.x * qv.x, g.y * qv.y, g.z * qv.z, g.w * qv.w);
  reinterpret_cast<float4*>(qx)[i] = make_float4(qv.x + xv.x, qv.y + xv.y, qv.z + xv.z, qv.w + xv.w);
}

// The launch shape: RP (here `kp`) by the size of the launch and what fits (threads, LDS), then the rows per workgroup
struct FfShape {
  int kp = 0, r = 0, threads = 0, rows_per_wg = 0, nsplit = 0;
  size_t lds = 0;
};
bool ff_shape_fits(int H, int NH, int kp, int r, FfShape& s) {
  if ((long long)NH * kp > FF_MAX_THREADS) return false;
  s.kp = kp;
  s.r = r;
  s.threads = (NH * kp + 63) / 64 * 64;
  s.lds = ((size_t)r * H + (kp > 1 ? (size_t)r * NH : 0)) * sizeof(float);
  return s.lds <= FF_MAX_LDS;
}
FfShape ff_shape(int B, int N, int H, int hs) {
  const int NH = H / hs;
  FfShape s;
  const bool small = (long long)B * N < 8192;
  if (!(small && ff_shape_fits(H, NH, 4, 16, s)) && !ff_shape_fits(H, NH, 2, 16, s)) (void)ff_shape_fits(H, NH, 1, 16, s);  // the last always fits
  const long long tiles = (long long)B * ((N + s.r - 1) / s.r);
  const long long per = std::max<long long>(1, (tiles + FF_TARGET_WG - 1) / FF_TARGET_WG);
  s.rows_per_wg = (int)std::min<long long>(per * s.r, (long long)(N + s.r - 1) / s.r * s.r);
  s.nsplit = (N + s.rows_per_wg - 1) / s.rows_per_wg;
  return s;
}

const char* ff_check(int B, int N, int H, int hs) {
  if (B <= 0 || B > 65535 || N <= 0 || N > (1 << 24)) return "ff_pool: bad batch / sequence size";
  if (H <= 0 || H > 1024 || (H & 3)) return "ff_pool: hidden must be a multiple of 4 in (0, 1024]";
  if (hs != 1 && hs != 2 && hs != 4 && hs != 8) return "ff_pool: head size must be 1, 2, 4 or 8";
  if (H % hs || H / hs > FF_MAX_HEADS) return "ff_pool: hidden / head size must be an integer of at most 512";
  return nullptr;
}

template <int HS>
void ff_launch(const float* v, int v_ld, const float* scale, const float* wl, const float* bl, const int32_t* lens, float* out, float* ws, int B,
               int N, int H, hipStream_t s) {
  const int NH = H / HS;
  const FfShape sh = ff_shape(B, N, H, HS);
  const dim3 grid(sh.nsplit, B);
  const float div = (float)sqrt((double)HS);  // the Python float attention_head_size ** 0.5, cast to the tensor's fp32
#define FF_GO(R_, KP_, MAXT_)                                                                                                                \
  hipLaunchKernelGGL((ff_pool_partial_kernel<HS, R_, KP_, MAXT_>), grid, dim3(sh.threads), sh.lds, s, v, v_ld, scale, wl, bl, lens, ws, N, H, NH, \
                     sh.rows_per_wg, sh.nsplit, div)
  const bool big = sh.threads > 512;
  if (sh.kp == 4) { if (big) FF_GO(16, 4, 1024); else FF_GO(16, 4, 512); }
  else if (sh.kp == 2) { if (big) FF_GO(16, 2, 1024); else FF_GO(16, 2, 512); }
  else FF_GO(16, 1, 512);   // heads <= 512
#undef FF_GO
  hipLaunchKernelGGL(ff_pool_merge_kernel<HS>, dim3((NH + 63) / 64, B), dim3(64), 0, s, ws, out, NH, sh.nsplit);
}

}  // namespace

size_t ff_pool_workspace_bytes(int B, int N, int H, int head_size) {
  if (ff_check(B, N, H, head_size)) return 0;
  return (size_t)B * ff_shape(B, N, H, head_size).nsplit * (H / head_size) * (head_size + 2) * sizeof(float);
}

int ff_pool_splits(int B, int N, int H, int head_size) { return ff_check(B, N, H, head_size) ? 0 : ff_shape(B, N, H, head_size).nsplit; }

const char* launch_ff_pool(const float* v, int v_ld, const float* scale, const float* wl, const float* bl, const int32_t* lens, float* out, float* ws,
                           size_t ws_bytes, int B, int N, int H, int head_size, hipStream_t s) {
  if (!v || !wl || !bl || !out || !ws) return "ff_pool: null pointer";
  if (const char* m = ff_check(B, N, H, head_size)) return m;
  if (v_ld < H || (v_ld & 3)) return "ff_pool: row stride must be a multiple of 4 and at least hidden";
  if (((uintptr_t)v | (uintptr_t)scale | (uintptr_t)out | (uintptr_t)ws) & 15) return "ff_pool: unaligned pointer";
  if (ws_bytes < ff_pool_workspace_bytes(B, N, H, head_size)) return "ff_pool: workspace too small";
  switch (head_size) {
    case 1: ff_launch<1>(v, v_ld, scale, wl, bl, lens, out, ws, B, N, H, s); break;
    case 2: ff_launch<2>(v, v_ld, scale, wl, bl, lens, out, ws, B, N, H, s); break;
    case 4: ff_launch<4>(v, v_ld, scale, wl, bl, lens, out, ws, B, N, H, s); break;
    default: ff_launch<8>(v, v_ld, scale, wl, bl, lens, out, ws, B, N, H, s); break;
  }
  return hipGetLastError() == hipSuccess ? nullptr : "ff_pool: launch failed";
}

const char* launch_ff_scale(const float* q, int q_ld, const float* gk, const float* x, float* wv, float* qx, int B, int N, int H, hipStream_t s) {
  if (!q || !gk || !x || !wv || !qx) return "ff_scale: null pointer";
  if (B <= 0 || N <= 0 || H <= 0 || (H & 3) || q_ld < H || (q_ld & 3)) return "ff_scale: bad dims";
  if (((uintptr_t)q | (uintptr_t)gk | (uintptr_t)x | (uintptr_t)wv | (uintptr_t)qx) & 15) return "ff_scale: unaligned pointer";
  const long long total4 = (long long)B * N * (H / 4);
  if ((total4 + 255) / 256 > 0x7fffffffLL) return "ff_scale: too many elements";
  hipLaunchKernelGGL(ff_scale_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, q, q_ld, gk, x, wv, qx, total4, N, H / 4);
  return hipGetLastError() == hipSuccess ? nullptr : "ff_scale: launch failed";
}

}  // namespace e2etts
