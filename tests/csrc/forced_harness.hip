// Test-only C entry points (e2ekt_*) of libe2etts_kernels_test.so around the three launch wrappers of csrc/teacher.hip (the teacher-forced
// pass): a third source beside kernel_harness.hip and kernel_harness_act16.hip, linked into the same library, with a staleness marker of
// its own (e2ekt_forced_version).  Thin on purpose: flat arguments in, the wrapper's own `const char*` (nullptr = launched) out, on the
// stream given.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#ifndef E2EKT_FZ_SRC_HASH
#define E2EKT_FZ_SRC_HASH "unknown"
#endif
#define KT_API extern "C" __attribute__((visibility("default")))

using namespace e2etts;

KT_API const char* e2ekt_forced_version() { return "E2EKT_FZ_SRC_HASH=" E2EKT_FZ_SRC_HASH; }

KT_API const char* e2ekt_soft_expand(const float* attn, const float* x, const int32_t* txt_lens, const int32_t* act_rows, const int32_t* act_rows_host,
                                     const float* pos, float* out, int B, int T, int L, int H, void* stream) {
  SoftExpandParams p;
  p.attn = attn; p.x = x; p.txt_lens = txt_lens; p.act_rows = act_rows; p.act_rows_host = act_rows_host; p.pos = pos; p.out = out;
  p.B = B; p.T = T; p.L = L; p.H = H;
  return launch_soft_expand(p, (hipStream_t)stream);
}

// up to three targets: src[k] [B, T] frames -> dst[k] [B, L] means, uv[k] != 0: the uv rule
KT_API const char* e2ekt_teacher_scan(float* dur, const int32_t* txt_lens, int32_t* cum, int64_t* mel64, int32_t* mel32, const int64_t* mel_given,
                                      int n_tg, const float* const* src, float* const* dst, const int* uv, int B, int L, int T, void* stream) {
  TeacherScanParams p;
  p.dur = dur; p.txt_lens = txt_lens; p.cum = cum; p.mel64 = mel64; p.mel32 = mel32; p.mel_given = mel_given;
  if (n_tg < 0 || n_tg > 3) return "e2ekt_teacher_scan: 0 .. 3 targets";
  p.n_tg = n_tg;
  for (int k = 0; k < n_tg; ++k) { p.tg[k].src = src[k]; p.tg[k].dst = dst[k]; p.tg[k].uv = uv[k]; }
  p.B = B; p.L = L; p.T = T;
  return launch_teacher_scan(p, (hipStream_t)stream);
}

// scalar controls only (the array controls are launch_variance_embed's, covered by the engine tests)
KT_API const char* e2ekt_target_embed(float* x, float* pitch_pred, const float* energy_pred, const float* pitch_t, const float* uv_t, const float* energy_t,
                                      int tld, int N, int H, float p_control, float e_control, float f0_mean, float f0_std, const float* energy_bins,
                                      const float* pitch_bins, int n_bins, int pitch_mode, int feat, const float* pitch_emb, const float* energy_emb,
                                      int32_t* pitch_idx, int32_t* energy_idx, int B, void* stream) {
  TargetEmbedParams q;
  q.pitch_t = pitch_t; q.uv_t = uv_t; q.energy_t = energy_t; q.tld = tld; q.N = N; q.H = H; q.p_control = p_control; q.e_control = e_control;
  q.f0_mean = f0_mean; q.f0_std = f0_std; q.energy_bins = energy_bins; q.pitch_bins = pitch_bins; q.n_bins = n_bins; q.pitch_mode = pitch_mode;
  q.feat = feat; q.pitch_emb = pitch_emb; q.energy_emb = energy_emb; q.pitch_idx = pitch_idx; q.energy_idx = energy_idx;
  return launch_target_embed(x, pitch_pred, energy_pred, q, B, (hipStream_t)stream);
}
