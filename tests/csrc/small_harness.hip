// Test-only C entry points (e2ekt_*) of libe2etts_kernels_test.so around the launch wrappers of the integer-decision and index kernels of
// csrc/small_kernels.hip (embedding, speaker add, predictor positions, rowdot, duration, variance_embed, the length regulator, act_rows,
// the join, the transpose, the iSTFT tail): a fourth source beside kernel_harness.hip, kernel_harness_act16.hip and forced_harness.hip,
// linked into the same library, with a staleness marker of its own (e2ekt_small_version).  Thin on purpose: flat arguments in, the
// wrapper's own `const char*` (nullptr = launched) out, on the stream given.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#ifndef E2EKT_SMALL_SRC_HASH
#define E2EKT_SMALL_SRC_HASH "unknown"
#endif
#define KT_API extern "C" __attribute__((visibility("default")))

using namespace e2etts;

KT_API const char* e2ekt_small_version() { return "E2EKT_SMALL_SRC_HASH=" E2EKT_SMALL_SRC_HASH; }

KT_API const char* e2ekt_embed(const int64_t* ids, const float* emb, const float* pos, float* x, int B, int L, int H, int n_rows, void* stream) {
  return launch_embed(ids, emb, pos, x, B, L, H, n_rows, (hipStream_t)stream);
}

KT_API const char* e2ekt_add_speaker(const float* xin, float* x, const float* spk, const int64_t* speaker, int n_spk_ids, int n_speakers, int B, int L,
                                     int H, void* stream) {
  return launch_add_speaker(xin, x, spk, speaker, n_spk_ids, n_speakers, B, L, H, (hipStream_t)stream);
}

KT_API const char* e2ekt_var_positions(const float* x, int32_t* posbuf, const float* table, int table_rows, const float* alpha, float* y, int B, int L,
                                       int H, int compute_positions, void* stream) {
  return launch_var_positions(x, posbuf, table, table_rows, alpha, y, B, L, H, (hipStream_t)stream, compute_positions != 0);
}

KT_API const char* e2ekt_rowdot(const float* x, const float* w, const float* b, float* out, const int32_t* lens, int B, int L, int C, int O, void* stream) {
  return launch_rowdot(x, w, b, out, lens, B, L, C, O, (hipStream_t)stream);
}

// the control as CtlRef's three fields (p == nullptr: the scalar d_control)
KT_API const char* e2ekt_duration(const float* log_d, float d_control, const float* p, int sb, int sl, float* dur, int32_t* cum, int64_t* mel64,
                                  int32_t* mel32, int B, int L, void* stream) {
  CtlRef c;
  c.p = p; c.sb = sb; c.sl = sl;
  return launch_duration(log_d, d_control, dur, cum, mel64, mel32, B, L, (hipStream_t)stream, c);
}

// VarCtl as two CtlRefs (pp, psb, psl | ep, esb, esl), N, cum, Lp
KT_API const char* e2ekt_variance_embed(float* x, float* pitch_pred, const float* energy_pred, float p_control, float e_control, float f0_mean,
                                        float f0_std, const float* energy_bins, int n_bins, const float* pitch_emb, const float* energy_emb,
                                        int32_t* pitch_idx, int32_t* energy_idx, int B, int L, int H, int pitch_mode, const float* pitch_bins, int feat,
                                        const float* pp, int psb, int psl, const float* ep, int esb, int esl, int N, const int32_t* cum, int Lp,
                                        void* stream) {
  VarCtl c;
  c.p.p = pp; c.p.sb = psb; c.p.sl = psl;
  c.e.p = ep; c.e.sb = esb; c.e.sl = esl;
  c.N = N; c.cum = cum; c.Lp = Lp;
  return launch_variance_embed(x, pitch_pred, energy_pred, p_control, e_control, f0_mean, f0_std, energy_bins, n_bins, pitch_emb, energy_emb, pitch_idx,
                               energy_idx, B, L, H, (hipStream_t)stream, pitch_mode, pitch_bins, feat, c);
}

KT_API const char* e2ekt_length_regulate(const float* x, const int32_t* cum, const int32_t* mel_lens, const float* pos, float* y, int B, int L, int T,
                                         int H, void* stream) {
  return launch_length_regulate(x, cum, mel_lens, pos, y, B, L, T, H, (hipStream_t)stream);
}

KT_API const char* e2ekt_add_positions(float* y, const float* pos, int B, int T, int H, void* stream) {
  return launch_add_positions(y, pos, B, T, H, (hipStream_t)stream);
}

KT_API const char* e2ekt_act_rows(const int32_t* lens, int32_t* out, int B, int add, int mul, long long cap, long long add_rows, void* stream) {
  return launch_act_rows(lens, out, B, add, mul, cap, (hipStream_t)stream, add_rows);
}

KT_API const char* e2ekt_accum_div(float* S, const float* Sj, const float* Sk, long long n, float div, void* stream) {
  return launch_accum_div(S, Sj, n, div, (hipStream_t)stream, Sk);
}

KT_API const char* e2ekt_transpose_bct_btc(const float* in, float* out, int B, int C, int T, void* stream) {
  return launch_transpose_bct_btc(in, out, B, C, T, (hipStream_t)stream);
}

KT_API const char* e2ekt_reflect_lrelu(const float* in, float* out, int B, long long n, int C, float slope, void* stream) {
  return launch_reflect_lrelu(in, out, B, n, C, slope, (hipStream_t)stream);
}

KT_API const char* e2ekt_istft(const float* q, int ldq, float* specphase, float* ri, float* wav, int16_t* pcm, int B, long long F, int nfft, int hop,
                               void* stream) {
  return launch_istft(q, ldq, specphase, ri, wav, pcm, B, F, nfft, hop, (hipStream_t)stream);
}
