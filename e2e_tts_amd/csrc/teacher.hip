// The kernels of the teacher-forced acoustic pass (include/e2etts_forced.h: e2etts_acoustic_forced; reference U/layers.py:175-272 with
// attn_prior given): the soft expansion x = bmm(attn_soft, x) in exact fp32 on the fp32 MFMA, the duration scan of GIVEN durations fused
// with the per-phoneme means of frame-resolved targets (U/function.py:155-175), and the bucket / embedding epilogue of the variance
// adaptor fed from targets instead of predictions.  fp32 throughout; every global access is bounds-checked.
#include <math.h>

#include <algorithm>

#include "kernels.h"

namespace e2etts {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CHECK_LAUNCH(name) (hipGetLastError() == hipSuccess ? nullptr : name ": launch failed")

// ---------------------------------------------------------------- soft expansion
// out[b, t, :] = sum_{l < len_b} attn[b, t, l] * x[b, l, :] (+ pos[t, :]): M = frames, N = H, K = the utterance's own phoneme count.
// One workgroup = one 32-row tile of one utterance x up to four 32-column tiles (one wavefront each, one accumulator: the
// 32x32x2 fp32 MFMA issues every 64 cycles and its dependent latency is 64).  The A operand (the map) is staged through LDS in chunks
// of SE_KC columns -- its rows are L floats apart, a wavefront's 32 rows would be 32 separate lines from global memory --; the B operand
// (the utterance's phoneme rows) is read from global / L2 as 128-byte row segments, one k per half-wavefront.  Columns k >= len_b take
// part neither as map nor as phoneme row: both operands are SELECTED to 0 there (never multiplied), so whatever an earlier call left in
// the padded rows of x cannot reach the sum.  The order of the terms is k = 0, 1, 2, ... in one chain whatever T, L or B are: an
// utterance gives the same bits alone and inside a batch.
constexpr int SE_KC = 64;

__global__ __launch_bounds__(256) void soft_expand_kernel(const float* __restrict__ attn, const float* __restrict__ x,
                                                          const int32_t* __restrict__ txt_lens, const int32_t* __restrict__ act_rows,
                                                          const float* __restrict__ pos, float* __restrict__ out, int B, int T, int L, int H,
                                                          int waves, RowMap rm) {
  __shared__ float As[32][SE_KC + 1];
  int b, tile;
  if (rm.n) {
    if (!rowmap_find(rm, blockIdx.x, b, tile)) return;
  } else {
    const int tiles = (T + 31) / 32;
    b = blockIdx.x / tiles;
    tile = blockIdx.x - b * tiles;
  }
  if (b >= B) return;
  const int t0 = tile * 32;
  if (t0 >= T || (act_rows && t0 >= act_rows[b])) return;   // (uniform over the workgroup: before any barrier)
  const int len = min(max(txt_lens[b], 0), L);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int n0 = (blockIdx.y * waves + wave) * 32;
  const bool active = n0 < H;   // H % 32 == 0: a tile is inside or outside as a whole
  const float* ab = attn + (long long)b * T * L;
  const float* xb = x + (long long)b * L * H;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < len; k0 += SE_KC) {
    __syncthreads();   // the waves are done with the chunk before
    for (int i = tid; i < 32 * SE_KC; i += blockDim.x) {
      const int r = i / SE_KC, c = i - r * SE_KC;
      const int t = t0 + r, k = k0 + c;
      As[r][c] = (t < T && k < len) ? ab[(long long)t * L + k] : 0.f;
    }
    __syncthreads();
    if (active) {
      const int kc = min(SE_KC, len - k0);
      float bv[SE_KC / 2];
#pragma unroll
      for (int j = 0; j < SE_KC / 2; ++j) {
        const int k = k0 + 2 * j + lh;
        bv[j] = (2 * j < kc && k < len) ? xb[(long long)k * H + n0 + li] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < SE_KC / 2; ++j)
        if (2 * j < kc) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[li][2 * j + lh], bv[j], acc, 0, 0, 0);
    }
  }
  if (!active) return;
  float* ob = out + (long long)b * T * H;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (t >= T) continue;
    float v = acc[r];
    if (pos) v += pos[(long long)t * H + n0 + li];
    ob[(long long)t * H + n0 + li] = v;
  }
}

// ---------------------------------------------------------------- duration scan of given durations + per-phoneme means
// numpy's float32 sum of n consecutive elements (np.mean -> np.add.reduce on a contiguous slice: pairwise summation, 8 running sums per
// block of at most 128 elements, blocks joined as a binary tree), term for term, so that a mean is the reference's to the bit.
// rd(i): element i of the slice.
template <class R>
__device__ float np_block_sum(R rd, int lo, int n) {   // n <= 128
  if (n < 8) {
    float res = 0.f;
    for (int i = 0; i < n; ++i) res = __fadd_rn(res, rd(lo + i));
    return res;
  }
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = rd(lo + j);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = __fadd_rn(r[j], rd(lo + i + j));
  }
  float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])), __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
  for (; i < n; ++i) res = __fadd_rn(res, rd(lo + i));
  return res;
}
constexpr int kTeacherMaxFrames = 1 << 20;   // T and every duration: the predicted path's cap
constexpr int kTreeStack = 20;
template <class R>
__device__ __noinline__ float np_tree_sum(R rd, int lo, int n) {   // n > 128: a phoneme of more than 128 frames (rare: kept out of line)
  // sum(a, n) = sum(a, n2) + sum(a + n2, n - n2), n2 = n / 2 rounded down to a multiple of 8: post-order walk with explicit stacks.
  // Depth: a child holds at most n / 2 + 7 elements, so a node k levels down holds at most n / 2^k + 14; it has children only above
  // 128 elements.  With n <= kTeacherMaxFrames = 2^20 level 13 holds at most 142 and may split, level 14 at most 85 and is a leaf: the
  // node stack holds levels 0 .. 14 = 15 entries, the value stack one finished left sum per level above the current leaf plus that
  // leaf = 15.  kTreeStack leaves room beyond that; launch_teacher_scan refuses T above kTeacherMaxFrames.
  static_assert((kTeacherMaxFrames >> 13) + 14 > 128 && (kTeacherMaxFrames >> 14) + 14 <= 128, "np_tree_sum: 15 levels are derived for 2^20 frames");
  static_assert(kTreeStack >= 15 + 4, "np_tree_sum: stacks need the 15 levels of kTeacherMaxFrames, with headroom");
  int slo[kTreeStack], sn[kTreeStack], sph[kTreeStack];
  float val[kTreeStack];
  int sp = 0, vp = 0;
  slo[0] = lo; sn[0] = n; sph[0] = 0; sp = 1;
  while (sp > 0) {
    const int c = sp - 1;
    if (sn[c] <= 128) { val[vp++] = np_block_sum(rd, slo[c], sn[c]); --sp; continue; }
    int n2 = sn[c] / 2;
    n2 -= n2 % 8;
    if (sph[c] == 0) { sph[c] = 1; slo[sp] = slo[c]; sn[sp] = n2; sph[sp] = 0; ++sp; }
    else if (sph[c] == 1) { sph[c] = 2; slo[sp] = slo[c] + n2; sn[sp] = sn[c] - n2; sph[sp] = 0; ++sp; }
    else { const float rr = val[--vp], ll = val[--vp]; val[vp++] = __fadd_rn(ll, rr); --sp; }
  }
  return val[0];
}
template <class R>
__device__ __forceinline__ float np_sum(R rd, int lo, int n) {
  return n <= 128 ? np_block_sum(rd, lo, n) : np_tree_sum(rd, lo, n);
}

// One wavefront per utterance.  Pass 1 (duration_kernel's scan on given values): d = the duration clamped as include/e2etts_forced.h says
// (NaN / negative -> 0, fraction truncated, at most 2^20, 0 at and past the utterance's length), written back, inclusive scan -> cum,
// mel lengths = the sums, or the given ones (soft mode) clamped to [0, T].  Pass 2: the means of frames [pos, pos + d) of every target,
// pos = the exclusive scan, frames at or past T left out (numpy's slice), 0 for an empty span.  The reference overwrites the frame array
// with the means as it goes (frame2phoneme works in place), so phoneme i reads at frame f < i the MEAN of phoneme f instead of the frame:
// that can only happen when some pos_i < i, i.e. after a zero duration.  Utterances without such a phoneme take one lane per phoneme;
// the others are walked by lane 0 in phoneme order, reading dst[f] for f < i.  The order of the terms of a mean is the same on both paths.
__global__ __launch_bounds__(64) void teacher_scan_kernel(TeacherScanParams p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int L = p.L, T = p.T;
  const int len = min(max(p.txt_lens[b], 0), L);
  float* dur = p.dur + (long long)b * L;
  int32_t* cum = p.cum + (long long)b * L;
  long long carry = 0;
  bool quirk = false;
  for (int l0 = 0; l0 < L; l0 += 64) {
    const int l = l0 + lane;
    float d = 0.f;
    if (l < L) {
      const float g = dur[l];
      d = (l < len && g == g && g > 0.f) ? floorf(fminf(g, (float)kTeacherMaxFrames)) : 0.f;
      dur[l] = d;
    }
    const int dv = (int)d;
    int v = dv;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o);
      if (lane >= o) v += u;
    }
    if (l < L) cum[l] = (int32_t)min(carry + v, 0x7fffffffLL);
    const bool q = l < len && dv > 0 && carry + v - dv < (long long)l;
    quirk = quirk || __any(q);
    carry += __shfl(v, 63);
  }
  if (lane == 0) {
    long long m = carry;
    if (p.mel_given) m = min(max((long long)p.mel_given[b], 0LL), (long long)T);
    p.mel64[b] = m;
    p.mel32[b] = (int32_t)min(m, 0x7fffffffLL);
  }
  if (p.n_tg <= 0) return;
  __syncthreads();   // cum and dur of this utterance, written above by other lanes
  for (int k = 0; k < p.n_tg; ++k) {
    const float* src = p.tg[k].src + (long long)b * T;
    float* dst = p.tg[k].dst + (long long)b * L;
    const bool uv = p.tg[k].uv != 0;
    if (!quirk) {
      for (int l = lane; l < L; l += 64) {
        float m = 0.f;
        if (l < len) {
          const int d = (int)dur[l];
          const long long hi64 = cum[l], lo64 = hi64 - d;
          const int lo = (int)min(lo64, (long long)T), hi = (int)min(hi64, (long long)T);
          if (hi > lo) m = __fdiv_rn(np_sum([&](int f) { return src[f]; }, lo, hi - lo), (float)(hi - lo));
        }
        dst[l] = uv ? (m == 1.0f ? 1.0f : 0.f) : m;
      }
    } else if (lane == 0) {
      for (int l = 0; l < L; ++l) {
        float m = 0.f;
        if (l < len) {
          const int d = (int)dur[l];
          const long long hi64 = cum[l], lo64 = hi64 - d;
          const int lo = (int)min(lo64, (long long)T), hi = (int)min(hi64, (long long)T);
          if (hi > lo) m = __fdiv_rn(np_sum([&](int f) { return f < l ? dst[f] : src[f]; }, lo, hi - lo), (float)(hi - lo));
        }
        dst[l] = m;   // the raw mean: what a later phoneme reads; the uv rule follows the whole pass (U/layers.py:230-231)
      }
      if (uv)
        for (int l = 0; l < L; ++l) dst[l] = dst[l] == 1.0f ? 1.0f : 0.f;
    }
  }
}

// ---------------------------------------------------------------- pitch / energy buckets + embedding add, from targets
// variance_embed_kernel (small_kernels.hip) with each feature taken from its target when one is given (U/layers.py:136-171: f0s / uvs =
// target, no control; energy = target) and from prediction * control as there otherwise; the same separately rounded operations.
// Row r = (b, t) of [B, N] reads its targets at b * tld + t.  The prediction of a feature that has a target is left as the predictor
// wrote it (the reference returns it before any control).
__global__ __launch_bounds__(128) void target_embed_kernel(float* __restrict__ x, float* __restrict__ pitch_pred, const float* __restrict__ energy_pred,
                                                           TargetEmbedParams q, float mel_min, float mel_range) {
  const int row = blockIdx.x;
  const int b = row / q.N, t = row - b * q.N;
  const long long ti = (long long)b * q.tld + t;
  float p_control = q.p_control, e_control = q.e_control;
  const VarCtl& ctl = q.ctl;
  if (ctl.p.p || ctl.e.p) {
    int l = t;
    if (ctl.cum) {
      const int32_t* c = ctl.cum + (long long)b * ctl.Lp;
      int lo = 0, hi = ctl.Lp - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] > t) hi = mid; else lo = mid + 1;
      }
      l = lo;
    }
    if (ctl.p.p) p_control = ctl.p.p[(long long)b * ctl.p.sb + (long long)l * ctl.p.sl];
    if (ctl.e.p) e_control = ctl.e.p[(long long)b * ctl.e.sb + (long long)l * ctl.e.sl];
  }
  const int n_bins = q.n_bins, feat = q.feat, H = q.H;
  const bool p_tgt = q.pitch_t != nullptr, e_tgt = q.energy_t != nullptr;
  float f0 = 0.f, uvl = 0.f;
  int pidx = 0;
  if (!(feat & 1)) {
  } else if (q.pitch_mode == 2) {
    f0 = p_tgt ? q.pitch_t[ti] : mul_rn(pitch_pred[row], p_control);
    int lo = 0, hi = n_bins - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (!(q.pitch_bins[mid] >= f0)) lo = mid + 1; else hi = mid;   // (NaN: past the last boundary, as torch.bucketize)
    }
    pidx = lo;
  } else {
    if (p_tgt) {
      f0 = q.pitch_t[ti];
      uvl = q.uv_t[ti];
    } else {
      f0 = mul_rn(pitch_pred[2 * row], p_control);
      uvl = mul_rn(pitch_pred[2 * row + 1], p_control);
    }
    float f0d = q.pitch_mode == 1 ? powf(2.0f, f0) : __fadd_rn(mul_rn(f0, q.f0_std), q.f0_mean);
    if (uvl > 0.f) f0d = 0.f;
    float mel = mul_rn(1127.0f, logf(__fadd_rn(1.0f, __fdiv_rn(f0d, 700.0f))));
    if (mel > 0.f) mel = __fadd_rn(__fdiv_rn(mul_rn(__fsub_rn(mel, mel_min), 254.0f), mel_range), 1.0f);
    if (mel <= 1.f) mel = 1.f;
    if (mel > 255.f) mel = 255.f;
    pidx = (int)__fadd_rn(mel, 0.5f);
    pidx = pidx < 0 ? 0 : (pidx > n_bins - 1 ? n_bins - 1 : pidx);
  }
  int eidx = 0;
  if (feat & 2) {
    const float e = e_tgt ? q.energy_t[ti] : mul_rn(energy_pred[row], e_control);
    int lo = 0, hi = n_bins - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (!(q.energy_bins[mid] >= e)) lo = mid + 1; else hi = mid;
    }
    eidx = lo;
  }
  __syncthreads();  // every wave has read the prediction before thread 0 scales it in place
  if (threadIdx.x == 0) {
    if ((feat & 1) && q.pitch_mode != 2 && !p_tgt) {
      pitch_pred[2 * row] = f0;
      pitch_pred[2 * row + 1] = uvl;
    }
    if (feat & 1) q.pitch_idx[row] = pidx;
    if (feat & 2) q.energy_idx[row] = eidx;
  }
  float4* xr = reinterpret_cast<float4*>(x + (long long)row * H);
  const float4* pe = reinterpret_cast<const float4*>(q.pitch_emb + (long long)pidx * H);
  const float4* ee = reinterpret_cast<const float4*>(q.energy_emb + (long long)eidx * H);
  if (feat == 3) {
    for (int i = threadIdx.x; i < H / 4; i += blockDim.x) {
      const float4 a = xr[i], p = pe[i], e = ee[i];
      xr[i] = make_float4((a.x + p.x) + e.x, (a.y + p.y) + e.y, (a.z + p.z) + e.z, (a.w + p.w) + e.w);
    }
  } else {
    const float4* oe = (feat & 1) ? pe : ee;
    for (int i = threadIdx.x; i < H / 4; i += blockDim.x) {
      const float4 a = xr[i], p = oe[i];
      xr[i] = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
    }
  }
}

}  // namespace

const char* launch_soft_expand(const SoftExpandParams& p, hipStream_t s) {
  if (!p.attn || !p.x || !p.txt_lens || !p.out) return "soft_expand: null pointer";
  if (p.B <= 0 || p.T <= 0 || p.L <= 0 || p.H <= 0 || p.H % 32) return "soft_expand: bad dims (H must be a multiple of 32)";
  if ((long long)p.B * p.T * std::max(p.L, p.H) > (1LL << 40)) return "soft_expand: shape too large";
  const int tiles_n = p.H / 32, waves = std::min(4, tiles_n), gy = (tiles_n + waves - 1) / waves;
  const int tiles_t = (p.T + 31) / 32;
  RowMap rm;
  long long gx = (long long)p.B * tiles_t;
  if (p.act_rows_host && p.act_rows && p.B <= ROWMAP_MAX) {   // compact grid: only the row tiles that exist
    rm.n = p.B;
    rm.identity();
    rm.cum[0] = 0;
    for (int b = 0; b < p.B; ++b) {
      const int rows = std::min(std::max((int)p.act_rows_host[b], 0), p.T);
      rm.cum[b + 1] = rm.cum[b] + (rows + 31) / 32;
    }
    gx = rm.cum[p.B];
    if (gx == 0) return nullptr;
  }
  if (gx > 0x7fffffffLL) return "soft_expand: grid too large";
  hipLaunchKernelGGL(soft_expand_kernel, dim3((unsigned)gx, gy), dim3(64 * waves), 0, s, p.attn, p.x, p.txt_lens, p.act_rows, p.pos, p.out, p.B, p.T,
                     p.L, p.H, waves, rm);
  return CHECK_LAUNCH("soft_expand");
}
double soft_expand_flops(const SoftExpandParams& p) { return 2.0 * p.B * p.T * (double)p.L * p.H; }

const char* launch_teacher_scan(const TeacherScanParams& p, hipStream_t s) {
  if (!p.dur || !p.txt_lens || !p.cum || !p.mel64 || !p.mel32) return "teacher_scan: null pointer";
  if (p.B <= 0 || p.L <= 0) return "teacher_scan: bad dims";
  if (p.n_tg < 0 || p.n_tg > 3) return "teacher_scan: at most three targets";
  if ((p.n_tg > 0 || p.mel_given) && p.T <= 0) return "teacher_scan: T must be positive";
  if (p.T > kTeacherMaxFrames) return "teacher_scan: T above 2^20 frames";   // (np_tree_sum's stacks are sized for that)
  for (int k = 0; k < p.n_tg; ++k)
    if (!p.tg[k].src || !p.tg[k].dst) return "teacher_scan: null target";
  hipLaunchKernelGGL(teacher_scan_kernel, dim3(p.B), dim3(64), 0, s, p);
  return CHECK_LAUNCH("teacher_scan");
}

const char* launch_target_embed(float* x, float* pitch_pred, const float* energy_pred, const TargetEmbedParams& q, int B, hipStream_t s) {
  if (!x || !pitch_pred || !energy_pred || !q.energy_bins || !q.pitch_emb || !q.energy_emb || !q.pitch_idx || !q.energy_idx)
    return "target_embed: null pointer";
  if (B <= 0 || q.N <= 0 || q.H <= 0 || q.H % 4 || q.tld < q.N) return "target_embed: bad dims";
  if ((q.ctl.p.p || q.ctl.e.p) && (q.ctl.N != q.N || (q.ctl.cum && q.ctl.Lp <= 0))) return "target_embed: bad control geometry";
  if (q.feat < 1 || q.feat > 3) return "target_embed: bad feature mask";
  if (q.pitch_mode < 0 || q.pitch_mode > 2 || (q.pitch_mode == 2 && !q.pitch_bins)) return "target_embed: bad pitch mode";
  if (q.pitch_t && q.pitch_mode != 2 && !q.uv_t) return "target_embed: an f0 target needs its uv target";
  if (q.n_bins != 256) return "target_embed: the f0 coarse coding is defined for 256 bins (reference U/function.py:9)";
  if ((long long)B * q.N > 0x7fffffffLL) return "target_embed: grid too large";
  const double mel_min = 1127.0 * log(1.0 + 50.0 / 700.0), mel_max = 1127.0 * log(1.0 + 1100.0 / 700.0);   // as launch_variance_embed
  hipLaunchKernelGGL(target_embed_kernel, dim3(B * q.N), dim3(128), 0, s, x, pitch_pred, energy_pred, q, (float)mel_min, (float)(mel_max - mel_min));
  return CHECK_LAUNCH("target_embed");
}

}  // namespace e2etts
