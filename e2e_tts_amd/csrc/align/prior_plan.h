// The HIP-free half of the aligner's generated attention prior (include/e2etts_align.h: e2ealign_prior, e2ealign_forward_bb,
// e2ealign_align_bb): the argument checks, the beta-binomial parameters of a cell, and the size and index formula of the one table the
// kernels share.  aligner.hip includes it on both its host and its device side; tests/csrc/align_prior_plan_test.cc builds it with g++
// under AddressSanitizer + UBSan.
//
// The value of cell (t, k) of a row with P phonemes and M frames is exp of
//     [lgamma(P + 1) - lgamma(k + 1) - lgamma(P - k + 1)]                                      the COLUMN term: log C(P, k)
//   + [lgamma(a + b) - (lgamma(a) + lgamma(b)) - lgamma(P + a + b)]                            the FRAME term
//   + [lgamma(k + a) + lgamma(P - k + b)]                                                      per cell
// with a = s (t + 1), b = s (M - t).  The column terms of a batch are a table of B * L doubles (columns k >= P hold 0 and are never
// read), formed once per call; a frame term is formed once per frame by the wavefront that owns the frame.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define E2EALIGN_HD __host__ __device__
#else
#define E2EALIGN_HD
#endif

namespace e2ealign_prior_plan {

constexpr int MAX_B = 4096;                        // E2EALIGN_MAX_B
constexpr int MAX_L = 2048;                        // E2EALIGN_MAX_L
constexpr int64_t MAX_ROW_CELLS = (int64_t)1 << 28;   // T * L of one utterance stays below this
constexpr int64_t MAX_CELLS = (int64_t)1 << 33;       // B * T * L stays below this
// E2EALIGN_MAX_PRIOR_SCALING.  The largest log-gamma argument is P + s (M + 1) <= 2^11 + 2^20 * 2^28 < 2^49: an exact double whose
// log-gamma (about 2^49 * 33) is finite.
constexpr double MAX_SCALING = 1048576.0;
constexpr int FRAMES_PER_GROUP = 4;                // aln_prior_kernel: one wavefront per frame, four frames per workgroup

// ---- the checks: NULL, or why the call is refused
inline const char* check_shape(int64_t B, int64_t T, int64_t L) {
  if (B < 1 || T < 1 || L < 1) return "B, T and L must be positive";
  if (B > MAX_B) return "B > 4096";
  if (L > MAX_L) return "L > 2048";
  if (T * L >= MAX_ROW_CELLS) return "one utterance's map (T * L) must stay below 2^28 cells";
  if (B * T * L >= MAX_CELLS) return "B * T * L too large";
  return nullptr;
}

inline const char* check_scaling(double s) {
  if (!std::isfinite(s) || !(s > 0)) return "scaling must be finite and positive";
  if (s > MAX_SCALING) return "scaling above E2EALIGN_MAX_PRIOR_SCALING (2^20)";
  return nullptr;
}

// index of the first length outside [1, hi], or -1
inline int64_t first_bad_len(const int64_t* v, int64_t n, int64_t hi) {
  for (int64_t b = 0; b < n; ++b)
    if (v[b] < 1 || v[b] > hi) return b;
  return -1;
}

// ---- the parameters of frame t (0-based) of a row with M frames
E2EALIGN_HD inline double alpha_of(double s, int t) { return s * (double)(t + 1); }
E2EALIGN_HD inline double beta_of(double s, int M, int t) { return s * (double)(M - t); }

// ---- the column table: cols[b * L + k] = log C(txt_lens[b], k) for k < txt_lens[b]
E2EALIGN_HD inline size_t col_table_doubles(int B, int L) { return (size_t)B * (size_t)L; }
E2EALIGN_HD inline size_t col_index(int b, int k, int L) { return (size_t)b * (size_t)L + (size_t)k; }

// ---- aln_prior_kernel's grid: workgroup x covers frames [x * FRAMES_PER_GROUP, ...), wavefront g of it frame x * FRAMES_PER_GROUP + g
E2EALIGN_HD inline int frame_groups(int T) { return (T + FRAMES_PER_GROUP - 1) / FRAMES_PER_GROUP; }
E2EALIGN_HD inline size_t cell_index(int b, int t, int k, int T, int L) { return ((size_t)b * (size_t)T + (size_t)t) * (size_t)L + (size_t)k; }

}  // namespace e2ealign_prior_plan
