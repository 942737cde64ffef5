// e2e_tts_amd/csrc/condition/plan.h as a stand-alone CPU program, built by tests/test_condition_sanitizer.py with
// g++ -fsanitize=address,undefined.  Every buffer is a heap allocation of exactly the size plan.h promises, so an index outside it is a
// sanitizer report.  Modes: sweep | big | checks | tile W
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../e2e_tts_amd/csrc/condition/plan.h"

namespace pl = e2econd_plan;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(2);                                                       \
    }                                                                \
  } while (0)

static uint64_t lcg_state = 1;
static uint32_t lcg() {
  lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (uint32_t)(lcg_state >> 33);
}

// quiet and loud stretches of 20 .. 420 ms
static std::vector<int16_t> make_signal(int64_t N, int rate, uint64_t seed) {
  lcg_state = seed;
  std::vector<int16_t> x((size_t)N);
  int64_t j = 0;
  bool quiet = lcg() & 1;
  while (j < N) {
    const int64_t d = (int64_t)(20 + lcg() % 400) * rate / 1000;
    const int amp = quiet ? 60 : 9000;
    for (int64_t e = j + d < N ? j + d : N; j < e; ++j) x[(size_t)j] = (int16_t)((int)(lcg() % (2 * amp + 1)) - amp);
    quiet = !quiet;
  }
  return x;
}

// the definition, directly on the samples
struct Direct {
  std::vector<int32_t> ranges;
  int64_t len = 0;
};
static Direct direct(const std::vector<int16_t>& x, int rate, int W, int k) {
  Direct d;
  const int64_t N = (int64_t)x.size();
  d.len = pl::len_ms(N, rate);
  if (d.len < W) return d;
  std::vector<uint64_t> c((size_t)N + 1, 0);
  for (int64_t j = 0; j < N; ++j) c[(size_t)j + 1] = c[(size_t)j] + (uint64_t)((int)x[(size_t)j] * (int)x[(size_t)j]);
  int64_t prev = -1;
  for (int64_t i = 0; i + W <= d.len; ++i) {
    const int64_t a = pl::pos(i, rate), b = pl::pos(i + W, rate);
    const uint64_t S = c[(size_t)(b < N ? b : N)] - c[(size_t)(a < N ? a : N)];
    if (!(S < (uint64_t)(k + 1) * (k + 1) * (uint64_t)(b - a))) continue;
    if (prev < 0 || i > prev + W) {
      d.ranges.push_back((int32_t)i);
      d.ranges.push_back((int32_t)(i + W));
    } else {
      d.ranges.back() = (int32_t)(i + W);
    }
    prev = i;
  }
  return d;
}

static long sweep_one(int rate, int64_t N, int W, int k, int T, uint64_t seed) {
  const std::vector<int16_t> x = make_signal(N, rate, seed);
  const Direct d = direct(x, rate, W, k);
  const int64_t len = pl::len_ms(N, rate), nb = pl::n_bins(N, rate, len), starts = pl::n_starts(len, W);
  CHECK(len == d.len && nb >= len && pl::pos(nb, rate) >= N);
  // the bins, by bin_of
  std::vector<uint64_t> bins((size_t)nb, 0);
  for (int64_t j = 0; j < N; ++j) {
    const int64_t p = pl::bin_of(j, rate);
    CHECK(p >= 0 && p < nb && pl::pos(p, rate) <= j && j < pl::pos(p + 1, rate));
    bins[(size_t)p] += (uint64_t)((int)x[(size_t)j] * (int)x[(size_t)j]);
  }
  // the window test, tile by tile
  const pl::Tile tile = T ? pl::make_tile(T, W) : pl::choose_tile(W);
  CHECK(tile.T % 64 == 0 && tile.lds_words <= pl::LDS_WORDS);
  std::vector<uint64_t> P((size_t)tile.lds_words);
  std::vector<uint64_t> flags((size_t)pl::ceil_div(starts, 64), ~(uint64_t)0);
  for (int64_t i0 = 0; i0 < starts; i0 += tile.T) pl::window_tile(bins.data(), i0, starts, tile, W, k, rate, P.data(), flags.data());
  // the walk, word by word, with room for every range and with room for one
  const int64_t true_count = (int64_t)d.ranges.size() / 2;
  CHECK(true_count <= pl::max_ranges(len, W) || true_count == 0);
  for (int64_t cap : {pl::max_ranges(len, W) > 0 ? pl::max_ranges(len, W) : (int64_t)1, (int64_t)1}) {
    std::vector<int32_t> rg((size_t)cap * 2, 0);
    pl::Walk w;
    for (size_t i = 0; i < flags.size(); ++i) pl::walk_word(w, flags[i], (int64_t)i * 64, W, cap, rg.data());
    pl::walk_end(w, W, cap, rg.data());
    CHECK(w.count == true_count);   // the true count, also past cap
    const int64_t listed = true_count < cap ? true_count : cap;
    CHECK(listed == 0 || memcmp(rg.data(), d.ranges.data(), (size_t)listed * 8) == 0);
    for (int trim : {pl::TRIM_NONE, pl::TRIM_REFERENCE, pl::TRIM_BOTH}) {
      const pl::Span sp = pl::kept_span(w.count, w.first_start, w.first_end, w.last_start, w.last + W, trim, len, N, rate);
      int64_t s = 0, e = len, n = N;
      if (true_count && trim != pl::TRIM_NONE) {
        if (d.ranges[0] == 0) s = d.ranges[1];
        if (trim == pl::TRIM_BOTH && d.ranges[(size_t)true_count * 2 - 1] == len) e = d.ranges[(size_t)true_count * 2 - 2];
        n = pl::pos(e, rate) - pl::pos(s, rate);
        if (n < 0) n = 0;
      }
      CHECK(sp.s_ms == s && sp.e_ms == e && sp.n_out == n);
      CHECK(sp.bin_lo >= 0 && sp.bin_lo <= sp.bin_hi && sp.bin_hi <= nb);
      // the span's bins sum to the span's samples
      uint64_t S = 0, D = 0;
      for (int64_t p = sp.bin_lo; p < sp.bin_hi; ++p) S += bins[(size_t)p];
      const int64_t a = (true_count && trim != pl::TRIM_NONE) ? pl::pos(s, rate) : 0;
      for (int64_t j = a; j < a + n && j < N; ++j) D += (uint64_t)((int)x[(size_t)j] * (int)x[(size_t)j]);
      CHECK(S == D);
    }
  }
  return (long)true_count;
}

static int sweep() {
  long cases = 0, ranges = 0;
  const int rates[] = {8000, 11025, 16000, 22050, 44100, 48000};
  for (int rate : rates)
    for (int ms : {1000, 1999, 3000})
      for (int extra : {0, 1, rate / 2000 + 1})
        for (int W : {100, 7})
          for (int T : {0, 64, 128, 448}) {
            ranges += sweep_one(rate, pl::pos(ms, rate) + extra, W, W == 100 ? 103 : 200, T, (uint64_t)(rate + ms * 7 + extra));
            ++cases;
          }
  // rows shorter than a window, and one sample
  for (int64_t N : {(int64_t)1, (int64_t)7, (int64_t)791, (int64_t)800, (int64_t)801}) sweep_one(8000, N, 100, 103, 0, 5), ++cases;
  CHECK(ranges > cases);   // the signals do have silences
  printf("OK %ld cases, %ld ranges\n", cases, ranges);
  return 0;
}

static int big() {
  const int rates[] = {1000, 8000, 11025, 22050, 44100, 48000, 384000};
  for (int rate : rates)
    for (int64_t p : {(int64_t)0, (int64_t)1, (int64_t)699999, (int64_t)1 << 24, ((int64_t)1 << 30) - 1, (int64_t)1 << 30}) {
      CHECK((__int128)pl::pos(p, rate) == (__int128)p * rate / 1000);
      for (int64_t j : {pl::pos(p, rate), pl::pos(p + 1, rate) - 1}) {   // the first and the last sample of ms p
        const __int128 q = ((__int128)(j + 1) * 1000 - 1) / rate;
        CHECK((__int128)pl::bin_of(j, rate) == q && pl::bin_of(j, rate) == p);
      }
    }
  for (int rate : rates) {
    const int64_t N = pl::MAX_N;
    const int64_t len = pl::len_ms(N, rate);
    CHECK(pl::n_bins(N, rate, len) >= len && pl::pos(pl::n_bins(N, rate, len), rate) >= N);
    CHECK((__int128)pl::ceil_div(N * 1000, rate) == ((__int128)N * 1000 + rate - 1) / rate);
  }
  // len_ms rounds half to even, as Python's round does
  CHECK(pl::len_ms(4, 8000) == 0 && pl::len_ms(12, 8000) == 2 && pl::len_ms(5, 8000) == 1 && pl::len_ms(20, 8000) == 2);
  printf("OK\n");
  return 0;
}

static int checks() {
  CHECK(!pl::config_check(22050, 100, 103) && !pl::config_check(1000, 1, 0) && !pl::config_check(384000, 4096, 32767));
  CHECK(pl::config_check(999, 100, 103) && pl::config_check(384001, 100, 103) && pl::config_check(22050, 0, 103) && pl::config_check(22050, 4097, 103));
  CHECK(pl::config_check(22050, 100, -1) && pl::config_check(22050, 100, 32768));
  CHECK(!pl::batch_check(1, 1, 1) && !pl::batch_check(4096, pl::MAX_N, pl::MAX_N));
  CHECK(pl::batch_check(0, 1, 1) && pl::batch_check(4097, 1, 1) && pl::batch_check(1, 0, 1) && pl::batch_check(1, pl::MAX_N + 1, pl::MAX_N + 1) && pl::batch_check(1, 8, 7));
  CHECK(!pl::analyze_check(2, 8, 8, pl::TRIM_BOTH, 1) && !pl::analyze_check(2, 8, 9, pl::TRIM_NONE, pl::MAX_CAP));
  CHECK(pl::analyze_check(2, 8, 8, 3, 1) && pl::analyze_check(2, 8, 8, -1, 1) && pl::analyze_check(2, 8, 8, 0, 0) && pl::analyze_check(2, 8, 8, 0, pl::MAX_CAP + 1));
  CHECK(pl::out_stride(0) == 0 && pl::out_stride(1) == 8 && pl::out_stride(8) == 8 && pl::out_stride(9) == 16);
  CHECK(pl::max_ranges(99, 100) == 0 && pl::max_ranges(100, 100) == 1 && pl::max_ranges(201, 100) == 2);
  printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "sweep") return sweep();
  if (mode == "big") return big();
  if (mode == "checks") return checks();
  if (mode == "tile" && argc > 2) {
    const pl::Tile t = pl::choose_tile(atoi(argv[2]));
    printf("T=%d lds_words=%d\n", t.T, t.lds_words);
    return 0;
  }
  fprintf(stderr, "usage: condition_plan_test sweep | big | checks | tile W\n");
  return 1;
}
