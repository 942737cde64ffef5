// The HIP-free half of libe2etts_condition.so (include/e2etts_condition.h): millisecond positions, the argument checks, the capacities,
// the tile choice of the window test, and a scalar restatement of the window test and of the range walk.  condition.hip includes it on
// both its host and its device side; tests/csrc/condition_plan_test.cc builds it with g++ under AddressSanitizer + UBSan.  Everything
// is integer: positions are int64, sums of squares uint64 (a row of 2^32 samples of +-32768 sums to 2^62).
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define E2ECOND_HD __host__ __device__
#else
#define E2ECOND_HD
#endif

namespace e2econd_plan {

constexpr int MIN_RATE = 1000;                 // a millisecond holds at least one sample: no bin is empty
constexpr int MAX_RATE = 384000;
constexpr int MAX_W = 4096;                    // min_silence_len in ms
constexpr int MAX_K = 32767;                   // the threshold in int16 units
constexpr int MAX_B = 4096;
constexpr int64_t MAX_N = (int64_t)1 << 32;    // samples per row
constexpr int MAX_CAP = 1 << 20;               // ranges per row a caller may ask for
constexpr int THREADS = 256;
constexpr int BIN_TILE = 128;                  // ms bins one workgroup of the bin kernel sums
constexpr int SPAN_TILE = 4096;                // ms bins one workgroup of the span sum adds
constexpr int LDS_WORDS = 7680;                // 60 KiB of uint64: the window kernel keeps 4 KiB of scan partials beside them
constexpr int TRIM_NONE = 0, TRIM_REFERENCE = 1, TRIM_BOTH = 2;

// ---- positions
E2ECOND_HD inline int64_t pos(int64_t ms, int rate) { return ms * rate / 1000; }   // sample index of millisecond ms
// the millisecond bin of sample j: the p with pos(p) <= j < pos(p + 1)
E2ECOND_HD inline int64_t bin_of(int64_t j, int rate) { return ((j + 1) * 1000 - 1) / rate; }
E2ECOND_HD inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }   // a >= 0, b > 0

// round(1000 * (N / rate)) as Python evaluates it: two roundings in double, then half-to-even (the default rounding mode).  Host only.
inline int64_t len_ms(int64_t N, int rate) { return (int64_t)std::nearbyint(1000.0 * ((double)N / (double)rate)); }
// bins that cover both [0, pos(len_ms)) and [0, N): len_ms rounds down as often as up
E2ECOND_HD inline int64_t n_bins(int64_t N, int rate, int64_t len) {
  const int64_t c = ceil_div(N * 1000, rate);
  return c > len ? c : len;
}
E2ECOND_HD inline int64_t n_starts(int64_t len, int W) { return len >= W ? len - W + 1 : 0; }
// the most ranges a row of `len` ms can have: consecutive range starts are more than W apart
inline int64_t max_ranges(int64_t len, int W) { return ceil_div(n_starts(len, W), (int64_t)W + 1); }

// ---- checks: NULL, or the message
inline const char* config_check(int64_t rate, int64_t W, int64_t k) {
  if (rate < MIN_RATE || rate > MAX_RATE) return "rate must lie in [1000, 384000]";
  if (W < 1 || W > MAX_W) return "min_silence_len must lie in [1, 4096] ms";
  if (k < 0 || k > MAX_K) return "the threshold k must lie in [0, 32767]";
  return nullptr;
}
inline const char* batch_check(int64_t B, int64_t n, int64_t stride) {
  if (B < 1 || B > MAX_B) return "B must lie in [1, 4096]";
  if (n < 1 || n > MAX_N) return "n must lie in [1, 2^32]";
  if (stride < n) return "the row stride must be at least n";
  return nullptr;
}
inline const char* analyze_check(int64_t B, int64_t n, int64_t stride, int trim, int64_t cap) {
  if (const char* m = batch_check(B, n, stride)) return m;
  if (trim != TRIM_NONE && trim != TRIM_REFERENCE && trim != TRIM_BOTH) return "trim must be E2ECOND_TRIM_NONE, _REFERENCE or _BOTH";
  if (cap < 1 || cap > MAX_CAP) return "cap must lie in [1, 2^20]";
  return nullptr;
}

// ---- the window test.  A tile of T starts [i0, i0 + cnt) reads the cnt + W - 1 bins from i0 on; with their exclusive prefix sums
// P[0 .. cnt + W - 1] start i0 + t is silent iff P[t + W] - P[t] < (k + 1)^2 * (pos(i0 + t + W) - pos(i0 + t)).
struct Tile {
  int T = 0;           // starts per workgroup, a multiple of 64 (one flag word per wavefront ballot)
  int lds_words = 0;   // T + W: the prefix sums of T + W - 1 bins
};
inline Tile make_tile(int T, int W) {
  Tile t;
  t.T = T;
  t.lds_words = T + W;
  return t;
}
inline Tile choose_tile(int W) {   // about four windows of starts per tile: one fifth of the bins is read twice
  int T = (4 * W + 255) / 256 * 256;
  if (T < 256) T = 256;
  while (T > 64 && T + W > LDS_WORDS) T -= 64;
  return make_tile(T, W);
}
E2ECOND_HD inline bool window_silent(uint64_t sum, int64_t i, int W, int k, int rate) {
  return sum < (uint64_t)(k + 1) * (uint64_t)(k + 1) * (uint64_t)(pos(i + W, rate) - pos(i, rate));
}
// scalar restatement of one tile: bins of the row, P a scratch of tile.lds_words, flags the row's words (bit i % 64 of word i / 64)
inline void window_tile(const uint64_t* bins, int64_t i0, int64_t starts, const Tile& tile, int W, int k, int rate, uint64_t* P, uint64_t* flags) {
  const int64_t cnt = starts - i0 < tile.T ? starts - i0 : tile.T;
  uint64_t run = 0;
  for (int64_t t = 0; t < cnt + W - 1; ++t) {
    P[t] = run;
    run += bins[i0 + t];
  }
  P[cnt + W - 1] = run;
  for (int64_t t0 = 0; t0 < cnt; t0 += 64) {
    uint64_t m = 0;
    for (int l = 0; l < 64 && t0 + l < cnt; ++l)
      if (window_silent(P[t0 + l + W] - P[t0 + l], i0 + t0 + l, W, k, rate)) m |= (uint64_t)1 << l;
    flags[(i0 + t0) / 64] = m;
  }
}

// ---- the range walk.  Silent starts in order; a start more than W after its silent predecessor opens a new range; a range is
// [first start, last start + W].  The walk carries (last silent start, ranges so far) from word to word; the first range and the last
// range's start are kept beside the capped list, so the kept span does not depend on cap.
struct Walk {
  int64_t last = -1;          // last silent start so far
  int64_t count = 0;          // ranges opened so far (the true count, also past cap)
  int64_t first_start = 0, first_end = 0, last_start = 0;
};
E2ECOND_HD inline bool opens(int64_t b, int64_t prev, int W) { return prev < 0 || b > prev + W; }

// one word of 64 flags from start `base` on; ranges [cap][2]
inline void walk_word(Walk& w, uint64_t m, int64_t base, int W, int64_t cap, int32_t* ranges) {
  for (int l = 0; l < 64; ++l) {
    if (!((m >> l) & 1)) continue;
    const int64_t b = base + l;
    if (opens(b, w.last, W)) {
      const int64_t r = w.count++;
      if (r < cap) ranges[2 * r] = (int32_t)b;
      if (r >= 1 && r - 1 < cap) ranges[2 * (r - 1) + 1] = (int32_t)(w.last + W);
      if (r == 0) w.first_start = b;
      if (r == 1) w.first_end = w.last + W;
      w.last_start = b;
    }
    w.last = b;
  }
}
inline void walk_end(Walk& w, int W, int64_t cap, int32_t* ranges) {
  if (w.count == 0) return;
  if (w.count - 1 < cap) ranges[2 * (w.count - 1) + 1] = (int32_t)(w.last + W);
  if (w.count == 1) w.first_end = w.last + W;
}

// ---- the kept span of a row
struct Span {
  int64_t s_ms = 0, e_ms = 0, n_out = 0;
  int64_t bin_lo = 0, bin_hi = 0;   // the bins whose sum is the span's sum of squares
};
// count, first_start, first_end, last_start, last_end: of the walk (last_end = last silent start + W)
E2ECOND_HD inline Span kept_span(int64_t count, int64_t first_start, int64_t first_end, int64_t last_start, int64_t last_end, int trim, int64_t len, int64_t N,
                                 int rate) {
  Span sp;
  sp.e_ms = len;
  if (count == 0 || trim == TRIM_NONE) {   // unsliced: the N samples
    sp.n_out = N;
    sp.bin_hi = n_bins(N, rate, len);
    return sp;
  }
  if (first_start == 0) sp.s_ms = first_end;
  if (trim == TRIM_BOTH && last_end == len) sp.e_ms = last_start;
  const int64_t n = pos(sp.e_ms, rate) - pos(sp.s_ms, rate);
  sp.n_out = n > 0 ? n : 0;
  sp.bin_lo = sp.s_ms;
  sp.bin_hi = sp.e_ms > sp.s_ms ? sp.e_ms : sp.s_ms;
  return sp;
}

// row stride of the resident outputs: whole 16-byte stores of int16
inline int64_t out_stride(int64_t width) { return (width + 7) / 8 * 8; }

}  // namespace e2econd_plan
