// The HIP-free half of libe2etts_f0.so (include/e2etts_f0.h): the window and lag formulas, the argument checks, the frame grid in int64
// sample positions, the tile choice of the analysis kernel and its LDS plan.  f0.hip includes it on both its host and its device side;
// tests/csrc/f0_plan_test.cc builds it with g++ under AddressSanitizer + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define E2EF0_HD __host__ __device__
#else
#define E2EF0_HD
#endif

namespace e2ef0_plan {

constexpr int MIN_RATE = 1000;
constexpr int MAX_RATE = 384000;
constexpr int MAX_B = 4096;
constexpr int MAX_K = 16;                      // candidates per frame: a 4-bit back-pointer names one
constexpr int64_t MAX_N = (int64_t)1 << 32;    // samples per row
constexpr int64_t MAX_T = (int64_t)1 << 24;    // frames per row
constexpr int64_t MAX_CELLS = (int64_t)1 << 31;   // B * T * max(K, lags): 32-bit safe counts of the workspaces' elements
constexpr int THREADS = 256;                   // of the analysis kernel: WAVES wavefronts, one frame each at a time
constexpr int WAVES = 4;
constexpr int LANE_LAGS = 4;                   // lags per lane and pass: one 16-byte LDS read serves four of them
constexpr int PASS_LAGS = 64 * LANE_LAGS;
// a lag's products are summed in chunks of CHUNK consecutive i and the chunk sums are then added in ascending order: the rounding-error
// bound of the sum is gamma(CHUNK + ceil(Wp / CHUNK)) instead of gamma(W) (tests/f0_ref.py derives the bar from these two numbers)
constexpr int CHUNK = 32;
constexpr int MAX_TILE = 16;                   // frames per workgroup at most
constexpr int LDS_BYTES = 65536;               // what one workgroup may take

E2EF0_HD inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }   // a >= 0, b > 0
E2EF0_HD inline int round_up(int a, int m) { return (a + m - 1) / m * m; }

// ---- the frame grid: int64 sample positions
E2EF0_HD inline int64_t frames_of(int64_t n, int hop) { return n / hop; }
E2EF0_HD inline int64_t centre(int64_t t, int hop) { return t * hop + hop / 2; }

// ---- the geometry of (sample_rate, hop, floor, ceiling)
struct Geometry {
  int sr = 0, hop = 0;
  int W = 0, h = 0;              // window samples (odd), half width
  int tau_min = 0, tau_max = 0;
  int NL = 0;                    // lags 0 .. tau_max + 1
  // the analysis kernel's LDS plan, in floats
  int NL4 = 0;                   // NL rounded up to 4: one wavefront's row of lags
  int Wp = 0;                    // W rounded up to 4: the i loop runs in steps of 4 over a zero tail
  int AL = 0;                    // one wavefront's `a`: Wp + NL4 + 4, zeros from W on (a[i + tau] past the window reads 0)
  int NC = 0;                    // local maxima one frame can have at most, + 1
  int F = 0;                     // frames per workgroup (a multiple of WAVES)
  int stage = 0;                 // the tile's samples: (F - 1) * hop + W
  int lds_floats = 0;            // stage | WAVES * AL | WAVES * NL4
};

E2EF0_HD inline int stage_floats(int F, int hop, int W) { return (F - 1) * hop + W; }
E2EF0_HD inline int lds_floats_for(int F, int hop, int W, int AL, int NL4) { return round_up(stage_floats(F, hop, W), 4) + WAVES * AL + WAVES * NL4; }

// NULL, or why the geometry is refused.  `g` is filled on success.
inline const char* geometry(int64_t sr, int64_t hop, double floor_hz, double ceiling_hz, Geometry* g) {
  if (sr < MIN_RATE || sr > MAX_RATE) return "sample_rate must lie in [1000, 384000]";
  if (hop < 1 || hop > sr) return "hop must lie in [1, sample_rate]";
  if (!(floor_hz > 0) || !std::isfinite(floor_hz) || !std::isfinite(ceiling_hz) || !(ceiling_hz > floor_hz)) return "need 0 < floor < ceiling, both finite";
  if (3.0 * (double)sr / floor_hz > 1e6) return "floor is too low for this sample rate: the window does not fit the kernel's LDS plan";
  Geometry q;
  q.sr = (int)sr;
  q.hop = (int)hop;
  q.W = (int)std::floor(3.0 * (double)sr / floor_hz);
  if (q.W % 2 == 0) q.W += 1;
  q.h = (q.W - 1) / 2;
  q.tau_max = (int)std::floor((double)sr / floor_hz);
  q.tau_min = (int)std::ceil((double)sr / ceiling_hz);
  if (q.tau_min < 2) return "tau_min = ceil(sample_rate / ceiling) must be at least 2";
  if (q.tau_min > q.tau_max) return "no lag lies in [ceil(sample_rate / ceiling), floor(sample_rate / floor)]";
  q.NL = q.tau_max + 2;
  if (q.NL >= q.W) return "the lag range must be shorter than the window";
  q.NL4 = round_up(q.NL, 4);
  q.Wp = round_up(q.W, 4);
  q.AL = q.Wp + q.NL4 + 4;
  q.NC = q.NL / 2 + 2;
  if (3 * q.NC > q.AL) return "the candidate list does not fit the window buffer";
  q.F = 0;
  for (int F = MAX_TILE; F >= WAVES; F -= WAVES)
    if ((int64_t)(F - 1) * hop + q.W < ((int64_t)1 << 24) && (int64_t)lds_floats_for(F, q.hop, q.W, q.AL, q.NL4) * 4 <= LDS_BYTES) {
      q.F = F;
      break;
    }
  // the limit: 4 * (round_up(3 hop + W, 4) + 4 (Wp + NL4 + 4) + 4 NL4) <= 65536 bytes
  if (!q.F) return "the window and the lag table do not fit the kernel's LDS plan (four frames' windows, four rows of lags and four frames' samples in 64 KiB)";
  q.stage = stage_floats(q.F, q.hop, q.W);
  q.lds_floats = lds_floats_for(q.F, q.hop, q.W, q.AL, q.NL4);
  *g = q;
  return nullptr;
}

// ---- the other checks: NULL, or the message
inline const char* params_check(size_t struct_size, size_t expected, double voicing_threshold, double silence_threshold, double octave_cost, double octave_jump_cost,
                                double voiced_unvoiced_cost, int64_t K) {
  if (struct_size != expected) return "params.struct_size is not sizeof(e2ef0_params)";
  if (!std::isfinite(voicing_threshold) || voicing_threshold < 0) return "voicing_threshold must be finite and not negative";
  if (!std::isfinite(silence_threshold) || !(silence_threshold > 0)) return "silence_threshold must be finite and positive";
  if (!std::isfinite(octave_cost) || octave_cost < 0) return "octave_cost must be finite and not negative";
  if (!std::isfinite(octave_jump_cost) || octave_jump_cost < 0) return "octave_jump_cost must be finite and not negative";
  if (!std::isfinite(voiced_unvoiced_cost) || voiced_unvoiced_cost < 0) return "voiced_unvoiced_cost must be finite and not negative";
  if (K < 2 || K > MAX_K) return "max_candidates must lie in [2, 16]";
  return nullptr;
}
inline const char* batch_check(int64_t B, int64_t n, int64_t stride, int hop, int64_t per_frame) {
  if (B < 1 || B > MAX_B) return "B must lie in [1, 4096]";
  if (n < 1 || n > MAX_N) return "n must lie in [1, 2^32]";
  if (stride < n) return "audio_stride must be at least n";
  const int64_t T = frames_of(n, hop);
  if (T > MAX_T) return "a row holds at most 2^24 frames";
  if (B * (T > 0 ? T : 1) * per_frame > MAX_CELLS) return "B * T * max(K, lags) must stay below 2^31";
  return nullptr;
}

// ---- a tile of the analysis kernel: frames [t0, t0 + F) of a row.  Staged float j holds sample first_sample(t0) + j; frame t's window
// starts at staged offset (t - t0) * hop.
E2EF0_HD inline int64_t first_sample(int64_t t0, int hop, int h) { return centre(t0, hop) - h; }
E2EF0_HD inline int frame_offset(int64_t t, int64_t t0, int hop) { return (int)((t - t0) * hop); }
E2EF0_HD inline int64_t tiles_of(int64_t T, int F) { return ceil_div(T, F); }

}  // namespace e2ef0_plan
