// e2e_tts_amd/csrc/align/prior_plan.h as a stand-alone CPU program, built by tests/test_align_prior_sanitizer.py with
// g++ -fsanitize=address,undefined.  Every table is a heap allocation of exactly the size prior_plan.h promises, so an index outside it
// is a sanitizer report.
// Modes: walk | checks | value P M S T K
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "../../e2e_tts_amd/csrc/align/prior_plan.h"

namespace pl = e2ealign_prior_plan;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(2);                                                              \
    }                                                                       \
  } while (0)

// the three terms of prior_plan.h's formula with the host's lgamma, the order of aligner.hip
static double col_term(int P, int k) { return (lgamma((double)P + 1.0) - lgamma((double)k + 1.0)) - lgamma((double)(P - k) + 1.0); }
static double frame_term(int P, int M, double s, int t) {
  const double a = pl::alpha_of(s, t), b = pl::beta_of(s, M, t);
  return (lgamma(a + b) - (lgamma(a) + lgamma(b))) - lgamma((double)P + (a + b));
}
static float value(int P, int M, double s, int t, int k, double col, double frame) {
  const double a = pl::alpha_of(s, t), b = pl::beta_of(s, M, t);
  return (float)exp((col + frame) + (lgamma((double)k + a) + lgamma((double)(P - k) + b)));
}

// aln_prior_cols_kernel's and aln_prior_kernel's walk over a batch, thread for thread, on heap buffers of the planned sizes
static long walk_batch(const std::vector<int>& txt, const std::vector<int>& mel, int T, int L, double s) {
  const int B = (int)txt.size();
  CHECK(pl::check_shape(B, T, L) == nullptr && pl::check_scaling(s) == nullptr);
  std::vector<double> cols(pl::col_table_doubles(B, L));
  std::vector<char> col_written(cols.size(), 0);
  const size_t n_cols = pl::col_table_doubles(B, L);
  for (size_t i = 0; i < (n_cols + 255) / 256 * 256; ++i) {   // the launched threads, the tail of the last workgroup included
    if (i >= n_cols) continue;
    const int b = (int)(i / (size_t)L), k = (int)(i - (size_t)b * L);
    const size_t at = pl::col_index(b, k, L);
    CHECK(at == i && !col_written[at]);
    col_written[at] = 1;
    cols[at] = k < txt[b] ? col_term(txt[b], k) : 0.0;
  }
  std::vector<float> out((size_t)B * T * L);
  std::vector<char> written(out.size(), 0);
  long cells = 0;
  for (int b = 0; b < B; ++b)
    for (int x = 0; x < pl::frame_groups(T); ++x)
      for (int g = 0; g < pl::FRAMES_PER_GROUP; ++g) {
        const int t = x * pl::FRAMES_PER_GROUP + g;
        if (t >= T) continue;
        const int P = txt[b], M = mel[b];
        const bool live = t < M;
        const double frame = live ? frame_term(P, M, s, t) : 0.0;
        for (int lane = 0; lane < 64; ++lane)
          for (int j = lane; j < L; j += 64) {
            const size_t at = pl::cell_index(b, t, j, T, L);
            CHECK(!written[at]);
            written[at] = 1;
            out[at] = (live && j < P) ? value(P, M, s, t, j, cols[pl::col_index(b, j, L)], frame) : 0.f;
            ++cells;
          }
      }
  CHECK(cells == (long)out.size());   // every cell exactly once, zeros included
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t < T; ++t) {
      double sum = 0;
      for (int k = 0; k < L; ++k) {
        const float v = out[pl::cell_index(b, t, k, T, L)];
        CHECK(v == v && v >= 0.f && v <= 1.f);
        if (t >= mel[b] || k >= txt[b]) CHECK(v == 0.f);
        sum += v;
      }
      if (t < mel[b]) CHECK(sum > 0 && sum < 1.0 + 1e-6);   // outcome P is not stored: below 1
    }
  }
  return cells;
}

static int walk() {
  long cells = 0;
  cells += walk_batch({1}, {1}, 1, 1, 1.0);
  cells += walk_batch({5}, {1}, 1, 5, 1.0);
  cells += walk_batch({7}, {3}, 3, 7, 1.0);
  cells += walk_batch({12, 7, 1}, {70, 33, 5}, 70, 12, 1.0);
  cells += walk_batch({12, 7, 1}, {70, 33, 5}, 81, 70, 1.0);
  cells += walk_batch({65, 64}, {129, 1}, 130, 65, 0.5);
  cells += walk_batch({40}, {300}, 301, 41, 2.5);
  cells += walk_batch({130}, {9}, 9, 130, pl::MAX_SCALING);
  cells += walk_batch({3, 2}, {2, 2}, 2, 3, 4.9e-324);   // the smallest positive scaling: alpha and beta stay positive
  // a row of the widest batch the checks admit, the last column of the last row: the index formulas in size_t
  CHECK(pl::col_index(pl::MAX_B - 1, pl::MAX_L - 1, pl::MAX_L) == pl::col_table_doubles(pl::MAX_B, pl::MAX_L) - 1);
  CHECK(pl::check_shape(4096, 1023, 2048) == nullptr);
  CHECK(pl::cell_index(4095, 1022, 2047, 1023, 2048) == (size_t)4096 * 1023 * 2048 - 1);   // beyond 2^32: no 32-bit product
  printf("OK %ld cells\n", cells);
  return 0;
}

static int checks() {
  CHECK(pl::check_shape(1, 1, 1) == nullptr && pl::check_shape(pl::MAX_B, 1, pl::MAX_L) == nullptr);
  CHECK(pl::check_shape(0, 1, 1) && pl::check_shape(1, 0, 1) && pl::check_shape(1, 1, 0) && pl::check_shape(-1, 5, 5));
  CHECK(pl::check_shape(pl::MAX_B + 1, 1, 1) && pl::check_shape(1, 1, pl::MAX_L + 1));
  CHECK(pl::check_shape(1, (int64_t)1 << 28, 1) && pl::check_shape(1, ((int64_t)1 << 28) - 1, 1) == nullptr);
  CHECK(pl::check_shape(1, 2147483647, 2048));                       // the products are formed in int64
  CHECK(pl::check_shape(4096, 1024, 2048) && pl::check_shape(4096, 1023, 2048) == nullptr);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(pl::check_scaling(1.0) == nullptr && pl::check_scaling(4.9e-324) == nullptr && pl::check_scaling(pl::MAX_SCALING) == nullptr);
  CHECK(pl::check_scaling(0.0) && pl::check_scaling(-0.0) && pl::check_scaling(-1.0) && pl::check_scaling(inf) && pl::check_scaling(-inf) && pl::check_scaling(nan));
  CHECK(pl::check_scaling(std::nextafter(pl::MAX_SCALING, inf)) && pl::check_scaling(1e300));
  // the stated limit keeps every log-gamma argument, and the log-gamma itself, finite at the largest frame count a shape admits
  const int M = (1 << 28) - 1;
  const double a = pl::alpha_of(pl::MAX_SCALING, M - 1), b = pl::beta_of(pl::MAX_SCALING, M, 0), top = (double)pl::MAX_L + (a + pl::MAX_SCALING);
  CHECK(std::isfinite(a) && std::isfinite(b) && a == b && std::isfinite(top) && std::isfinite(lgamma(top)));
  CHECK(pl::alpha_of(4.9e-324, 0) > 0 && pl::beta_of(4.9e-324, 1, 0) > 0 && std::isfinite(lgamma(4.9e-324)));
  const int64_t good[3] = {1, 5, 3}, low[3] = {1, 0, 3}, high[3] = {1, 5, 6}, neg[2] = {-7, 1};
  CHECK(pl::first_bad_len(good, 3, 5) == -1 && pl::first_bad_len(low, 3, 5) == 1 && pl::first_bad_len(high, 3, 5) == 2 && pl::first_bad_len(neg, 2, 5) == 0);
  CHECK(pl::first_bad_len(good, 0, 5) == -1);
  printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "walk") return walk();
  if (mode == "checks") return checks();
  if (mode == "value" && argc == 7) {
    const int P = atoi(argv[2]), M = atoi(argv[3]), t = atoi(argv[5]), k = atoi(argv[6]);
    const double s = atof(argv[4]);
    if (pl::check_shape(1, M, P) || pl::check_scaling(s) || t < 0 || t >= M || k < 0 || k >= P) {
      printf("ERR\n");
      return 0;
    }
    printf("%.9g\n", (double)value(P, M, s, t, k, col_term(P, k), frame_term(P, M, s, t)));
    return 0;
  }
  fprintf(stderr, "usage: align_prior_plan_test walk | checks | value P M S T K\n");
  return 1;
}
