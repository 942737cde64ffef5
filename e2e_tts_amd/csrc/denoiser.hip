// Vocoder-bias denoiser (reference V/denoiser.py: STFT :55-153, Denoiser :156-186): the passes around the two convolutions.
//
// The reference's STFT is a strided convolution with the windowed Fourier basis and its inverse a transposed convolution with the
// windowed pseudo-inverse.  With hop = filter_length / n_overlap both are "same" convolutions over ROWS of hop samples, which
// conv_gemm computes in exact fp32 (engine_denoise.hip: denoise_impl):
//   forward   the reflect-padded signal as rows [B, F + n_overlap - 1, hop]; frame f is rows f .. f + n_overlap - 1, so the
//             spectrum is a KW = n_overlap, Cin = hop, Cout = filter_length + 2, pad = 0 convolution;
//   inverse   Cin = filter_length + 2, Cout = hop, the taps reversed: output row q = sum_s frame[q - s] . W_s holds samples q * hop ..
//             q * hop + hop - 1 of the overlap-add.  Run as one accumulated KW = 1 launch per tap (engine_denoise.hip: denoise_impl says why).
// What is left are three HBM-bound passes, each a sweep of float4 rows:
//   stft_pad_kernel            F.pad(mode = 'reflect') per utterance at ITS OWN end, into the row layout (:98-101)
//   spectral_subtract_kernel   magnitude, - strength * bias, clamp at 0, back to re / im without the three transcendentals (:115-123, :182-184)
//   ola_norm_kernel            / window sum-square envelope, * filter_length / hop, trim filter_length / 2 per end (:131-146), fp32 and int16
// and bias_frame_kernel, the magnitudes of one frame (the bias spectrum, :177-179).
#include "kernels.h"

#include <cfloat>
#include <climits>

namespace e2etts {
namespace {

#define CHECK_LAUNCH(name) (hipGetLastError() == hipSuccess ? nullptr : name ": launch failed")

// Every arithmetic step of these passes is ONE correctly rounded float32 operation (kernels.h states the contract; the per-kernel tests
// compare bit for bit).  Products go through mul_rn: __fmul_rn is a plain product here, which the compiler contracts into the add or subtract
// that consumes it.  The root is sqrtf, which compiles to the hardware estimate plus the correction against its neighbours; __fsqrt_rn
// compiles to the bare estimate.
__device__ __forceinline__ float magnitude(float re, float im) { return sqrtf(__fadd_rn(mul_rn(re, re), mul_rn(im, im))); }

// One thread per 4 consecutive positions of the padded signal of utterance blockIdx.y (hop % 32 == 0: rows and float4s line up).
__global__ void __launch_bounds__(256) stft_pad_kernel(const float* __restrict__ wav, long long wav_bs, const int32_t* __restrict__ n_valid,
                                                       float* __restrict__ out, int R, int hop, int half, bool vec_in) {
  const int b = blockIdx.y;
  const long long total4 = (long long)R * hop / 4;
  const long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 >= total4) return;
  const int nb = n_valid[b];
  const long long p0 = i4 * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* w = wav + (long long)b * wav_bs;
  if (nb > half) {  // (a row that cannot be reflected is passed through by ola_norm_kernel; its rows here are zeros)
    const long long padded = (long long)nb + 2 * half;
    const long long s0 = p0 - half;
    if (vec_in && s0 >= 0 && s0 + 3 < nb) {
      v = *reinterpret_cast<const float4*>(w + s0);
    } else {
      float t[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long p = p0 + k;
        long long s = p - half;
        if (s < 0) s = -s;                                // left reflection, edge sample not repeated
        else if (s >= nb) s = 2LL * (nb - 1) - s;         // right reflection at the utterance's own end
        t[k] = p < padded ? w[s] : 0.f;                   // nb > half keeps s in [0, nb)
      }
      v = make_float4(t[0], t[1], t[2], t[3]);
    }
  }
  *reinterpret_cast<float4*>(out + ((long long)b * R * hop + p0)) = v;
}

// One workgroup per spectrum row [Cpad] = re[0 .. bins) | im[0 .. bins) | zero padding.  bins is odd, so the imaginary half starts off a
// 16-byte boundary: the row goes through LDS, in and out as whole float4s.
__global__ void __launch_bounds__(256) spectral_subtract_kernel(float* __restrict__ spec, const float* __restrict__ bias, const int32_t* __restrict__ frames,
                                                                int R, int Cpad, int bins, int n_overlap, float strength) {
  extern __shared__ __attribute__((aligned(16))) float row[];
  const int b = blockIdx.y, f = blockIdx.x;
  const int Fb = frames[b];
  if (f >= Fb + n_overlap - 1) return;   // beyond what the inverse convolution reads for this utterance's samples
  float4* g = reinterpret_cast<float4*>(spec + ((long long)b * R + f) * Cpad);
  const int n4 = Cpad / 4;
  if (f >= Fb) {  // the zero frames the transposed convolution sees past the last one
    for (int i = threadIdx.x; i < n4; i += blockDim.x) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  float4* r4 = reinterpret_cast<float4*>(row);
  for (int i = threadIdx.x; i < n4; i += blockDim.x) r4[i] = g[i];
  __syncthreads();
  for (int k = threadIdx.x; k < bins; k += blockDim.x) {
    const float re = row[k], im = row[bins + k];
    const float mag = magnitude(re, im);
    const float md = fmaxf(__fsub_rn(mag, mul_rn(bias[k], strength)), 0.f);
    const float sc = mag > 0.f ? __fdiv_rn(md, mag) : 0.f;   // mag_d * cos / sin(atan2(im, re)) = (re, im) * mag_d / mag
    row[k] = mul_rn(re, sc);
    row[bins + k] = mul_rn(im, sc);
  }
  for (int k = 2 * bins + threadIdx.x; k < Cpad; k += blockDim.x) row[k] = 0.f;
  __syncthreads();
  for (int i = threadIdx.x; i < n4; i += blockDim.x) g[i] = r4[i];
}

// bias[k] = |spectrum row `f` of utterance 0|[k]
__global__ void bias_frame_kernel(const float* __restrict__ spec, float* __restrict__ bias, int bins) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= bins) return;
  const float re = spec[k], im = spec[bins + k];
  bias[k] = magnitude(re, im);
}

__device__ __forceinline__ int16_t pcm_sat(float v) {
  const float s = truncf(v * 32768.0f);
  return (int16_t)(int)fminf(fmaxf(s, -32768.0f), 32767.0f);
}

// One thread per 4 consecutive output samples of utterance blockIdx.y.  y: the inverse convolution's rows, [B, R * hop] = the overlap-add.
// The envelope is librosa's window_sumsquare as the reference calls it (:12-52): a float32 accumulator that takes the float64 squared
// window of every frame covering the sample, frame by frame.
__global__ void __launch_bounds__(256) ola_norm_kernel(const float* __restrict__ y, const float* __restrict__ in, long long in_bs, const int32_t* __restrict__ n_valid,
                                                       const int32_t* __restrict__ frames, const double* __restrict__ win_sq, float* __restrict__ wav,
                                                       int16_t* __restrict__ pcm, long long n, int R, int hop, int nfft, float scale, bool vec_out) {
  const int b = blockIdx.y;
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  const int nb = n_valid[b], Fb = frames[b], half = nfft / 2;
  float t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = i0 + k;
    float v = 0.f;
    if (i < n && i < nb) {
      if (nb <= half) {
        v = in[(long long)b * in_bs + i];   // too short to reflect (the reference raises): passed through
      } else {
        const long long p = i + half;
        v = y[(long long)b * R * hop + p];
        long long f_lo = p - nfft + 1 <= 0 ? 0 : (p - nfft + hop) / hop;
        long long f_hi = p / hop;
        if (f_hi > Fb - 1) f_hi = Fb - 1;
        float env = 0.f;
        for (long long f = f_lo; f <= f_hi; ++f) env = (float)((double)env + win_sq[p - f * hop]);
        if (env > FLT_MIN) v = __fdiv_rn(v, env);
        v = mul_rn(v, scale);
      }
    }
    t[k] = v;
  }
  const long long o = (long long)b * n + i0;
  if (vec_out && i0 + 3 < n) {
    if (wav) *reinterpret_cast<float4*>(wav + o) = make_float4(t[0], t[1], t[2], t[3]);
    if (pcm) {
      short4 s;
      s.x = pcm_sat(t[0]); s.y = pcm_sat(t[1]); s.z = pcm_sat(t[2]); s.w = pcm_sat(t[3]);
      *reinterpret_cast<short4*>(pcm + o) = s;
    }
  } else {
    for (int k = 0; k < 4 && i0 + k < n; ++k) {
      if (wav) wav[o + k] = t[k];
      if (pcm) pcm[o + k] = pcm_sat(t[k]);
    }
  }
}

// ---- stream forms (e2etts_vocoder_stream_begin_denoised): one WINDOW of a longer signal, every row alike.  The window's L samples sit at
// absolute position S0 of a signal whose ends may lie outside it: an edge that is a real end of the signal is reflected as above, an edge
// that is context is copied plainly, and the frames stay on the signal's absolute hop grid (S0 and filter_length / 2 are multiples of hop).

// out [B, Rq, hop], Rq * hop = L + half at each real edge.  seg: the window's samples, rows of stride seg_bs.
__global__ void __launch_bounds__(256) stft_pad_stream_kernel(const float* __restrict__ seg, long long seg_bs, float* __restrict__ out, long long L,
                                                              int Rq, int hop, int half, bool left_real, bool right_real, bool vec_in) {
  const int b = blockIdx.y;
  const long long total4 = (long long)Rq * hop / 4;
  const long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 >= total4) return;
  const long long p0 = i4 * 4, lead = left_real ? half : 0;
  const long long padded = L + lead + (right_real ? half : 0);
  const float* w = seg + (long long)b * seg_bs;
  float4 v;
  const long long s0 = p0 - lead;
  if (vec_in && s0 >= 0 && s0 + 3 < L) {
    v = *reinterpret_cast<const float4*>(w + s0);
  } else {
    float t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long p = p0 + k;
      long long s = p - lead;
      if (s < 0) s = -s;                                  // the signal's start: reflected, edge sample not repeated
      else if (s >= L) s = 2LL * (L - 1) - s;             // the signal's end (only a real right edge has positions past L)
      s = s < 0 ? 0 : (s >= L ? L - 1 : s);               // (L > half wherever an edge is real: the launcher checks; never out of the window)
      t[k] = p < padded ? w[s] : 0.f;
    }
    v = make_float4(t[0], t[1], t[2], t[3]);
  }
  *reinterpret_cast<float4*>(out + ((long long)b * Rq * hop + p0)) = v;
}

// frames[b] = v for every row: the table spectral_subtract_kernel reads, written on the stream that uses it
__global__ void fill_i32_kernel(int32_t* __restrict__ p, int n, int32_t v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// One thread per 4 consecutive EMITTED samples of row blockIdx.y: sample k is y[b, y_off + k], at absolute padded position p_abs0 + k of the
// signal.  The envelope is ola_norm_kernel's, frame by frame in ascending order over the absolute frames covering the position: clamped at
// frame 0 by the position itself, and at the last frame F_abs - 1 only where the signal's end is known (F_abs = LLONG_MAX otherwise: the
// emitted samples of such a window lie more than a filter before anything not yet pushed).  pass: a signal too short to reflect, copied.
__global__ void __launch_bounds__(256) ola_norm_stream_kernel(const float* __restrict__ y, long long y_bs, long long y_off, const float* __restrict__ in,
                                                              long long in_bs, const double* __restrict__ win_sq, float* __restrict__ wav,
                                                              int16_t* __restrict__ pcm, long long n, long long p_abs0, long long F_abs, int hop,
                                                              int nfft, float scale, bool pass, bool vec_out) {
  const int b = blockIdx.y;
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  float t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = i0 + k;
    float v = 0.f;
    if (i < n) {
      if (pass) {
        v = in[(long long)b * in_bs + i];
      } else {
        const long long p = p_abs0 + i;
        v = y[(long long)b * y_bs + y_off + i];
        long long f_lo = p - nfft + 1 <= 0 ? 0 : (p - nfft + hop) / hop;
        long long f_hi = p / hop;
        if (f_hi > F_abs - 1) f_hi = F_abs - 1;
        float env = 0.f;
        for (long long f = f_lo; f <= f_hi; ++f) env = (float)((double)env + win_sq[p - f * hop]);
        if (env > FLT_MIN) v = __fdiv_rn(v, env);
        v = mul_rn(v, scale);
      }
    }
    t[k] = v;
  }
  const long long o = (long long)b * n + i0;
  if (vec_out && i0 + 3 < n) {
    if (wav) *reinterpret_cast<float4*>(wav + o) = make_float4(t[0], t[1], t[2], t[3]);
    if (pcm) {
      short4 s;
      s.x = pcm_sat(t[0]); s.y = pcm_sat(t[1]); s.z = pcm_sat(t[2]); s.w = pcm_sat(t[3]);
      *reinterpret_cast<short4*>(pcm + o) = s;
    }
  } else {
    for (int k = 0; k < 4 && i0 + k < n; ++k) {
      if (wav) wav[o + k] = t[k];
      if (pcm) pcm[o + k] = pcm_sat(t[k]);
    }
  }
}

}  // namespace

const char* denoiser_geometry_check(int filter_length, int hop, int* n_overlap_out) {
  if (filter_length <= 0 || hop <= 0 || filter_length % hop) return "denoiser: filter_length must be hop * n_overlap";
  const int v = filter_length / hop;
  if (v != 2 && v != 4 && v != 8) return "denoiser: n_overlap = filter_length / hop must be 2, 4 or 8";
  if (hop % 32) return "denoiser: hop must be a multiple of 32";
  // spectral_subtract_kernel keeps one spectrum row, filter_length + 2 floats padded to 32, in dynamic LDS: 32.1 KiB at hop 1024 x 8, inside
  // the 64 KiB a kernel gets without opting in; launch_spectral_subtract checks the same limit (Cpad <= 16384 floats)
  if (hop > 1024) return "denoiser: hop must not exceed 1024 (one spectrum row is held in LDS)";
  if (n_overlap_out) *n_overlap_out = v;
  return nullptr;
}

const char* launch_stft_pad(const float* wav, long long wav_bs, const int32_t* n_valid, float* out, int B, int R, int filter_length, int hop,
                            hipStream_t s) {
  if (!wav || !n_valid || !out) return "stft_pad: null pointer";
  if (const char* m = denoiser_geometry_check(filter_length, hop, nullptr)) return m;
  if (B <= 0 || B > 65535 || R <= 0 || wav_bs < 0) return "stft_pad: bad dims";
  if ((uintptr_t)out & 15) return "stft_pad: out must be 16-byte aligned";
  const bool vec_in = (wav_bs % 4 == 0) && (((uintptr_t)wav & 15) == 0);
  const long long total4 = (long long)R * hop / 4;
  if ((total4 + 255) / 256 >= (1LL << 31)) return "stft_pad: grid too large";
  hipLaunchKernelGGL(stft_pad_kernel, dim3((unsigned)((total4 + 255) / 256), B), dim3(256), 0, s, wav, wav_bs, n_valid, out, R, hop,
                     filter_length / 2, vec_in);
  return CHECK_LAUNCH("stft_pad");
}

const char* launch_spectral_subtract(float* spec, const float* bias, const int32_t* frames, int B, int R, int Cpad, int filter_length, int n_overlap,
                                     float strength, hipStream_t s) {
  if (!spec || !bias || !frames) return "spectral_subtract: null pointer";
  const int bins = filter_length / 2 + 1;
  if (B <= 0 || B > 65535 || R <= 0 || filter_length <= 0 || filter_length % 2 || Cpad % 4 || Cpad < 2 * bins || Cpad > 16384)
    return "spectral_subtract: bad dims";
  // (rows frames[b] .. frames[b] + n_overlap - 2 are zeroed: a stray n_overlap would wipe rows the caller owns or leave the inverse's unzeroed)
  if (n_overlap != 2 && n_overlap != 4 && n_overlap != 8) return "spectral_subtract: n_overlap must be 2, 4 or 8";
  if ((uintptr_t)spec & 15) return "spectral_subtract: spec must be 16-byte aligned";
  hipLaunchKernelGGL(spectral_subtract_kernel, dim3(R, B), dim3(256), (size_t)Cpad * sizeof(float), s, spec, bias, frames, R, Cpad, bins, n_overlap,
                     strength);
  return CHECK_LAUNCH("spectral_subtract");
}

const char* launch_bias_frame(const float* spec_row, float* bias, int filter_length, hipStream_t s) {
  if (!spec_row || !bias || filter_length <= 0 || filter_length % 2) return "bias_frame: bad arguments";
  const int bins = filter_length / 2 + 1;
  hipLaunchKernelGGL(bias_frame_kernel, dim3((bins + 255) / 256), dim3(256), 0, s, spec_row, bias, bins);
  return CHECK_LAUNCH("bias_frame");
}

const char* launch_ola_norm(const float* y, const float* in, long long in_bs, const int32_t* n_valid, const int32_t* frames, const double* win_sq,
                            float* wav, int16_t* pcm, int B, long long n, int R, int filter_length, int hop, hipStream_t s) {
  if (!y || !in || !n_valid || !frames || !win_sq || (!wav && !pcm)) return "ola_norm: null pointer";
  if (const char* m = denoiser_geometry_check(filter_length, hop, nullptr)) return m;
  if (B <= 0 || B > 65535 || n <= 0 || R <= 0 || in_bs < 0) return "ola_norm: bad dims";
  const bool vec_out = (n % 4 == 0) && (!wav || ((uintptr_t)wav & 15) == 0) && (!pcm || ((uintptr_t)pcm & 7) == 0);
  const long long total4 = (n + 3) / 4;
  if ((total4 + 255) / 256 >= (1LL << 31)) return "ola_norm: grid too large";
  hipLaunchKernelGGL(ola_norm_kernel, dim3((unsigned)((total4 + 255) / 256), B), dim3(256), 0, s, y, in, in_bs, n_valid, frames, win_sq, wav, pcm, n, R,
                     hop, filter_length, (float)filter_length / (float)hop, vec_out);
  return CHECK_LAUNCH("ola_norm");
}

const char* launch_stft_pad_stream(const float* seg, long long seg_bs, float* out, int B, long long L, int Rq, int filter_length, int hop, bool left_real,
                                   bool right_real, hipStream_t s) {
  if (!seg || !out) return "stft_pad_stream: null pointer";
  if (const char* m = denoiser_geometry_check(filter_length, hop, nullptr)) return m;
  const int half = filter_length / 2;
  if (B <= 0 || B > 65535 || L <= 0 || Rq <= 0 || seg_bs < L) return "stft_pad_stream: bad dims";
  if ((left_real || right_real) && L <= half) return "stft_pad_stream: a window with a real edge must be longer than filter_length / 2";
  if ((long long)Rq * hop != L + (left_real ? half : 0) + (right_real ? half : 0)) return "stft_pad_stream: rows do not match the window";
  if ((uintptr_t)out & 15) return "stft_pad_stream: out must be 16-byte aligned";
  const bool vec_in = (seg_bs % 4 == 0) && (((uintptr_t)seg & 15) == 0);
  const long long total4 = (long long)Rq * hop / 4;
  if ((total4 + 255) / 256 >= (1LL << 31)) return "stft_pad_stream: grid too large";
  hipLaunchKernelGGL(stft_pad_stream_kernel, dim3((unsigned)((total4 + 255) / 256), B), dim3(256), 0, s, seg, seg_bs, out, L, Rq, hop, half, left_real,
                     right_real, vec_in);
  return CHECK_LAUNCH("stft_pad_stream");
}

const char* launch_fill_i32(int32_t* p, int n, int32_t v, hipStream_t s) {
  if (!p || n <= 0) return "fill_i32: bad arguments";
  hipLaunchKernelGGL(fill_i32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p, n, v);
  return CHECK_LAUNCH("fill_i32");
}

const char* launch_ola_norm_stream(const float* y, long long y_bs, long long y_off, const float* in, long long in_bs, const double* win_sq, float* wav,
                                   int16_t* pcm, int B, long long n, long long p_abs0, long long F_abs, int filter_length, int hop, bool pass,
                                   hipStream_t s) {
  if (!in || !win_sq || (!wav && !pcm) || (!pass && !y)) return "ola_norm_stream: null pointer";
  if (const char* m = denoiser_geometry_check(filter_length, hop, nullptr)) return m;
  if (B <= 0 || B > 65535 || n <= 0 || in_bs < n || p_abs0 < 0 || F_abs <= 0) return "ola_norm_stream: bad dims";
  if (!pass && (y_off < 0 || y_off + n > y_bs)) return "ola_norm_stream: emitted range outside the overlap-add";
  if (p_abs0 > LLONG_MAX - n) return "ola_norm_stream: absolute position overflows";
  const bool vec_out = (n % 4 == 0) && (!wav || ((uintptr_t)wav & 15) == 0) && (!pcm || ((uintptr_t)pcm & 7) == 0);
  const long long total4 = (n + 3) / 4;
  if ((total4 + 255) / 256 >= (1LL << 31)) return "ola_norm_stream: grid too large";
  hipLaunchKernelGGL(ola_norm_stream_kernel, dim3((unsigned)((total4 + 255) / 256), B), dim3(256), 0, s, y, y_bs, y_off, in, in_bs, win_sq, wav, pcm, n,
                     p_abs0, F_abs, hop, filter_length, (float)filter_length / (float)hop, pass, vec_out);
  return CHECK_LAUNCH("ola_norm_stream");
}

}  // namespace e2etts
