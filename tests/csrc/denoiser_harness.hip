// Test-only C entry points (e2ekt_*) of libe2etts_kernels_test.so around the seven launch wrappers of csrc/denoiser.hip (the reflect-pad, the
// spectral subtraction, the bias frame, the overlap-add normalisation, their two stream forms and the table fill): a fifth source beside
// kernel_harness.hip, kernel_harness_act16.hip, forced_harness.hip and small_harness.hip, linked into the same library, with a staleness
// marker of its own (e2ekt_denoiser_version).  Thin on purpose: flat arguments in, the wrapper's own `const char*` (nullptr = launched) out,
// on the stream given.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#ifndef E2EKT_DN_SRC_HASH
#define E2EKT_DN_SRC_HASH "unknown"
#endif
#define KT_API extern "C" __attribute__((visibility("default")))

using namespace e2etts;

KT_API const char* e2ekt_denoiser_version() { return "E2EKT_DN_SRC_HASH=" E2EKT_DN_SRC_HASH; }

KT_API const char* e2ekt_stft_pad(const float* wav, long long wav_bs, const int32_t* n_valid, float* out, int B, int R, int filter_length, int hop,
                                  void* stream) {
  return launch_stft_pad(wav, wav_bs, n_valid, out, B, R, filter_length, hop, (hipStream_t)stream);
}

KT_API const char* e2ekt_spectral_subtract(float* spec, const float* bias, const int32_t* frames, int B, int R, int Cpad, int filter_length,
                                           int n_overlap, float strength, void* stream) {
  return launch_spectral_subtract(spec, bias, frames, B, R, Cpad, filter_length, n_overlap, strength, (hipStream_t)stream);
}

KT_API const char* e2ekt_bias_frame(const float* spec_row, float* bias, int filter_length, void* stream) {
  return launch_bias_frame(spec_row, bias, filter_length, (hipStream_t)stream);
}

KT_API const char* e2ekt_ola_norm(const float* y, const float* in, long long in_bs, const int32_t* n_valid, const int32_t* frames, const double* win_sq,
                                  float* wav, int16_t* pcm, int B, long long n, int R, int filter_length, int hop, void* stream) {
  return launch_ola_norm(y, in, in_bs, n_valid, frames, win_sq, wav, pcm, B, n, R, filter_length, hop, (hipStream_t)stream);
}

KT_API const char* e2ekt_stft_pad_stream(const float* seg, long long seg_bs, float* out, int B, long long L, int Rq, int filter_length, int hop,
                                         int left_real, int right_real, void* stream) {
  return launch_stft_pad_stream(seg, seg_bs, out, B, L, Rq, filter_length, hop, left_real != 0, right_real != 0, (hipStream_t)stream);
}

KT_API const char* e2ekt_fill_i32(int32_t* p, int n, int32_t v, void* stream) { return launch_fill_i32(p, n, v, (hipStream_t)stream); }

KT_API const char* e2ekt_ola_norm_stream(const float* y, long long y_bs, long long y_off, const float* in, long long in_bs, const double* win_sq,
                                         float* wav, int16_t* pcm, int B, long long n, long long p_abs0, long long F_abs, int filter_length, int hop,
                                         int pass, void* stream) {
  return launch_ola_norm_stream(y, y_bs, y_off, in, in_bs, win_sq, wav, pcm, B, n, p_abs0, F_abs, filter_length, hop, pass != 0, (hipStream_t)stream);
}
