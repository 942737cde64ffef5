// e2e_tts_amd/csrc/stats/plan.h stand-alone under AddressSanitizer + UBSan (tests/test_stats_sanitizer.py): the virtual indices of the
// percentiles against __int128, the bitonic stage schedule on a scalar model of the kernel -- the keys a thread holds, the shuffles inside
// a wavefront, an LDS image of exactly the planned size --, the key transform, the argument checks and the caps.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../e2e_tts_amd/csrc/stats/plan.h"

namespace pl = e2est_plan;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

// the kernel's sort on a scalar model: keys[r][t] is key r of thread t; the image is a heap block of exactly lds_bytes(P)
static void model_sort(std::vector<uint32_t>& row) {
  const int n = (int)row.size();
  const int P = pl::image(n), E = pl::elems(P), NT = pl::threads(P);
  CHECK(E * NT == P && NT % pl::WAVE == 0 && NT <= pl::MAX_THREADS && E <= pl::MAX_E && P >= n && (P == pl::MIN_IMAGE || P < 2 * n));
  CHECK(pl::lds_bytes(P) <= pl::LDS_BYTES && pl::lds_bytes(P) >= (NT / pl::WAVE) * 8);
  uint32_t* image = new uint32_t[(size_t)pl::lds_bytes(P) / 4];
  for (int i = 0; i < P; ++i) image[i] = i < n ? row[i] : pl::KEY_PAD;
  std::vector<std::vector<uint32_t>> key(E, std::vector<uint32_t>(NT));
  for (int r = 0; r < E; ++r)
    for (int t = 0; t < NT; ++t) key[r][t] = image[r * NT + t];
  int stages = 0;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= 1; j >>= 1, ++stages) {
      const int cls = pl::stage_class(j, NT);
      if (cls == pl::STAGE_REG) {
        CHECK(j % NT == 0);
        const int d = j / NT;
        CHECK(d >= 1 && d < E && (d & (d - 1)) == 0);
        for (int t = 0; t < NT; ++t)
          for (int r = 0; r < E; ++r) {
            if (r & d) continue;
            const int i = r * NT + t;
            CHECK(pl::partner(i, j) == (r | d) * NT + t);
            const bool asc = pl::keeps_min(i, j, k);
            CHECK(pl::keeps_min(pl::partner(i, j), j, k) == !asc);
            const uint32_t a = key[r][t], b = key[r | d][t];
            key[r][t] = asc ? std::min(a, b) : std::max(a, b);
            key[r | d][t] = asc ? std::max(a, b) : std::min(a, b);
          }
      } else if (cls == pl::STAGE_SHFL) {
        CHECK(j < pl::WAVE);
        for (int r = 0; r < E; ++r) {
          std::vector<uint32_t> next(NT);
          for (int t = 0; t < NT; ++t) {
            const int i = r * NT + t, o = t ^ j;
            CHECK(o / pl::WAVE == t / pl::WAVE && pl::partner(i, j) == r * NT + o);   // the partner is a lane of the same wavefront
            const uint32_t other = key[r][o];
            next[t] = pl::keeps_min(i, j, k) ? std::min(key[r][t], other) : std::max(key[r][t], other);
          }
          key[r] = next;
        }
      } else {
        CHECK(cls == pl::STAGE_LDS && j >= pl::WAVE && j < NT);
        for (int r = 0; r < E; ++r)
          for (int t = 0; t < NT; ++t) image[r * NT + t] = key[r][t];
        for (int r = 0; r < E; ++r)
          for (int t = 0; t < NT; ++t) {
            const int i = r * NT + t;
            const uint32_t other = image[pl::partner(i, j)];
            key[r][t] = pl::keeps_min(i, j, k) ? std::min(key[r][t], other) : std::max(key[r][t], other);
          }
      }
    }
  }
  CHECK(stages == pl::stage_count(P));
  for (int r = 0; r < E; ++r)
    for (int t = 0; t < NT; ++t) image[r * NT + t] = key[r][t];
  std::vector<uint32_t> want(row);
  std::sort(want.begin(), want.end());
  for (int i = 0; i < n; ++i) CHECK(image[i] == want[i]);
  for (int i = n; i < P; ++i) CHECK(image[i] == pl::KEY_PAD);
  // what the kernel reads of the sorted image
  for (int q : {25, 75}) {
    const pl::VIndex v = pl::vindex(n, q);
    CHECK(v.lo >= 0 && v.lo <= v.hi && v.hi < n);
  }
  std::copy(image, image + n, row.begin());
  delete[] image;
}

static uint32_t bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

static int vindex_mode() {
  for (int64_t n = 1; n <= 70000; ++n)
    for (int q : {25, 75}) {
      const __int128 num = (__int128)(n - 1) * q;   // v = num / 100
      const int64_t lo = (int64_t)(num / 100);
      const int64_t rem = (int64_t)(num % 100);     // v - lo = rem / 100, a multiple of 1/4
      const pl::VIndex v = pl::vindex(n, q);
      CHECK(rem % 25 == 0);
      CHECK(v.lo == lo && v.hi == std::min<int64_t>(lo + 1, n - 1) && v.gamma == (float)rem / 100.0f && v.gamma == (float)((double)(n - 1) * (q / 100.0) - (double)lo));
    }
  const pl::VIndex one = pl::vindex(1, 75), two = pl::vindex(2, 25);
  CHECK(one.lo == 0 && one.hi == 0 && one.gamma == 0.f && two.lo == 0 && two.hi == 1 && two.gamma == 0.25f);
  printf("OK\n");
  return 0;
}

static int perm_mode() {
  long sorts = 0;
  for (int n = 1; n <= 8; ++n) {
    std::vector<uint32_t> p(n);
    for (int i = 0; i < n; ++i) p[i] = pl::key_of(bits((float)(i / 2) - 1.0f));   // ties too: values -1, -1, 0, 0, 1, 1 ..
    std::sort(p.begin(), p.end());
    do {
      std::vector<uint32_t> row(p);
      model_sort(row);
      ++sorts;
    } while (std::next_permutation(p.begin(), p.end()));
    std::vector<uint32_t> q(n);
    for (int i = 0; i < n; ++i) q[i] = pl::key_of(bits((float)i * 1.5f - 3.0f));  // all distinct: every permutation
    std::sort(q.begin(), q.end());
    do {
      std::vector<uint32_t> row(q);
      model_sort(row);
      ++sorts;
    } while (std::next_permutation(q.begin(), q.end()));
  }
  printf("OK %ld\n", sorts);
  return 0;
}

static int random_mode() {
  std::mt19937 rng(7);
  std::vector<int> lens = {1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
                           8191, 8192, 8193, 16383, pl::MAX_ROW};
  for (int i = 0; i < 40; ++i) lens.push_back(1 + (int)(rng() % pl::MAX_ROW));
  for (int n : lens) {
    std::vector<uint32_t> row(n);
    const int mode = (int)(rng() % 3);
    for (auto& v : row) {
      float f = mode == 0 ? (float)(int32_t)rng() / 65536.0f : mode == 1 ? (float)(rng() % 7) - 3.0f : (rng() % 2 ? -0.0f : 0.0f);
      v = pl::key_of(bits(f));
    }
    model_sort(row);
  }
  printf("OK %zu\n", lens.size());
  return 0;
}

static int checks_mode() {
  CHECK(!pl::kind_check(0) && !pl::kind_check(2) && pl::kind_check(3) && pl::kind_check(-1));
  CHECK(!pl::shape_check(1, 1, 1) && !pl::shape_check(pl::MAX_B, 100, 100) && pl::shape_check(0, 1, 1) && pl::shape_check(pl::MAX_B + 1, 1, 1));
  CHECK(pl::shape_check(1, 0, 1) && pl::shape_check(1, 5, 4) && pl::shape_check(1, (int64_t)1 << 31, (int64_t)1 << 31) && pl::shape_check(1, 5, (int64_t)1 << 31));
  CHECK(!pl::len_check(1, 1) && !pl::len_check(pl::MAX_ROW, pl::MAX_ROW) && pl::len_check(0, 5) && pl::len_check(-3, 5) && pl::len_check(6, 5));
  CHECK(std::string(pl::len_check(pl::MAX_ROW + 1, 1 << 20)).find("E2EST_MAX_ROW") != std::string::npos);
  CHECK(!pl::norm_len_check(0, 5) && !pl::norm_len_check(5, 5) && pl::norm_len_check(6, 5) && pl::norm_len_check(-1, 5));
  // the plan by length class
  const int P[] = {64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384}, E[] = {1, 2, 4, 4, 4, 8, 8, 8, 16}, NT[] = {64, 64, 64, 128, 256, 256, 512, 1024, 1024};
  int last = 0;
  for (int i = 0; i < 9; ++i) {
    CHECK(pl::image(P[i]) == P[i] && pl::image(P[i] / 2 + 1) == P[i] && (P[i] == pl::MAX_ROW || pl::image(P[i] + 1) == 2 * P[i]));
    CHECK(pl::elems(P[i]) == E[i] && pl::threads(P[i]) == NT[i] && pl::threads(P[i]) >= last && pl::lds_bytes(P[i]) == 4 * P[i]);   // a batch's block covers every row's
    last = pl::threads(P[i]);
  }
  CHECK(pl::image(1) == 64 && pl::image(pl::MAX_ROW) == pl::MAX_ROW && pl::lds_bytes(pl::MAX_ROW) == pl::LDS_BYTES && pl::stage_count(64) == 21 && pl::stage_count(16384) == 105);
  // the keys: unsigned order is float order with -0 below +0; the transform inverts; what counts as non-finite
  const float f[] = {-INFINITY, -3.5f, -1e-30f, -0.0f, 0.0f, 1e-30f, 2.0f, 3.4e38f, INFINITY};
  for (int i = 0; i < 9; ++i) {
    CHECK(pl::bits_of(pl::key_of(bits(f[i]))) == bits(f[i]));
    if (i) CHECK(pl::key_of(bits(f[i - 1])) < pl::key_of(bits(f[i])));
    CHECK(pl::non_finite(bits(f[i])) == (i == 0 || i == 8));
  }
  CHECK(pl::key_of(bits(INFINITY)) == pl::KEY_PAD && pl::key_of(bits(-INFINITY)) == pl::KEY_NEG_INF);
  CHECK(pl::non_finite(0x7fc00000u) && pl::non_finite(0xffc00001u) && pl::key_of(0x7fc00000u) > pl::KEY_PAD && pl::key_of(0xffc00001u) < pl::KEY_NEG_INF);
  printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "vindex") return vindex_mode();
  if (mode == "perm") return perm_mode();
  if (mode == "random") return random_mode();
  if (mode == "checks") return checks_mode();
  fprintf(stderr, "usage: stats_plan_test vindex | perm | random | checks\n");
  return 2;
}
