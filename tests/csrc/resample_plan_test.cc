// Stand-alone test of e2e_tts_amd/csrc/resample/plan.h (the HIP-free half of libe2etts_resample.so), built by
// tests/test_resample_sanitizer.py with g++ -fsanitize=address,undefined.  Every buffer below is a heap allocation of exactly the size
// plan.h says it needs, and is indexed the way resample.hip indexes it: an index formula that is off shows as a sanitizer report, a wrong
// value as a non-zero exit.
//
//   resample_plan_test sweep    exhaustive small (L, M, n_taps, n, chunking): table, window, LDS image, tile map, stream history
//   resample_plan_test big      int64 positions around n = 2^31 against __int128
//   resample_plan_test checks   the argument checks
//   resample_plan_test tile L M n_taps    prints the tile choice
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../e2e_tts_amd/csrc/resample/plan.h"

namespace pl = e2ers_plan;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

// integer-valued signal and taps: every sum below is exact in double, so "equal" means equal
static double sample(int64_t k) { return (double)((k * 7 + 3) % 11 - 5); }
static float tap(int64_t j) { return (float)((j * 5 + 1) % 7 - 3); }

// the definition, straight from the header
static double direct(int64_t m, int64_t n, const std::vector<float>& h, const pl::Filter& f) {
  double y = 0;
  const int64_t c = m * f.M + f.half;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t j = c - k * f.L;
    if (j >= 0 && j <= 2 * (int64_t)f.half) y += sample(k) * h[j];
  }
  return y;
}

// the kernel's walk of one launch: outputs [m_off, m_off + width) from a buffer whose element 0 is sample k_off and which holds samples
// up to n_valid; buf has exactly n_valid - k_off elements
static void launch(const pl::Filter& f, const pl::Tile& t, const float* G, const double* buf, int64_t k_off, int64_t n_valid, int64_t n_out_row,
                   int64_t m_off, int64_t width, double* out) {
  const int64_t tiles = pl::ceil_div(width, t.outputs);
  for (int64_t tile = 0; tile < tiles; ++tile) {
    const int64_t j0 = tile * t.outputs, m0 = m_off + j0;
    const int64_t in_tile = t.outputs < width - j0 ? t.outputs : width - j0;
    if (m0 >= n_out_row) {
      for (int64_t j = 0; j < in_tile; ++j) out[j0 + j] = 0;
      continue;
    }
    std::unique_ptr<double[]> lds(new double[t.lds_floats]);
    for (int i = 0; i < t.lds_floats; ++i) lds[i] = 1e300;   // a pad slot that is read shows in the sums
    const int64_t kb = pl::window_start(m0, f);
    for (int w = 0; w < t.window; ++w) {
      const int64_t k = kb + w;
      double v = 0;
      if (k >= 0 && k >= k_off && k < n_valid) v = buf[k - k_off];
      lds[pl::pad_index(w, t.shift)] = v;
    }
    for (int64_t o = 0; o < t.outputs; ++o) {
      const int64_t j = pl::tile_offset(o, t.S, f.L);
      CHECK(j >= 0 && j < t.outputs);
      if (j >= in_tile) continue;
      const int64_t m = m0 + j;
      double y = 0;
      if (m < n_out_row) {
        const int64_t c = pl::centre(m, f);
        CHECK(c % f.L == pl::phase(m, f) && c / f.L == pl::k_hi(m, f));
        const float* g = G + (c % f.L) * f.P;
        const int top = (int)(c / f.L - kb);
        CHECK(top >= f.P - 1 && top < t.window);
        for (int i = f.P - 1; i >= 0; --i) y += lds[pl::pad_index(top - i, t.shift)] * g[i];
      }
      out[j0 + j] = y;
    }
  }
}

static void one_case(int L, int M, int n_taps, pl::Tile t_override, bool use_override) {
  CHECK(pl::filter_check(n_taps, L, M) == nullptr);
  const pl::Filter f = pl::make_filter(n_taps, L, M);
  CHECK(f.half * 2 + 1 == n_taps && f.P == (n_taps + L - 1) / L);
  std::vector<float> h(n_taps);
  for (int j = 0; j < n_taps; ++j) h[j] = tap(j);
  std::unique_ptr<float[]> G(new float[pl::table_floats(f)]);
  pl::build_table(h.data(), f, G.get());
  for (int r = 0; r < L; ++r)
    for (int i = 0; i < f.P; ++i) CHECK(G[r * f.P + i] == (r + (int64_t)i * L < n_taps ? h[r + i * L] : 0.f));
  pl::Tile t = use_override ? t_override : pl::choose_tile(f);
  CHECK(t.S >= 1 && t.nrep >= 1 && t.outputs == (int64_t)t.S * L * t.nrep && t.window == t.S * t.nrep * M + f.P);
  CHECK(t.lds_floats == pl::pad_index(t.window - 1, t.shift) + 1);
  if (!use_override) CHECK(t.lds_floats <= pl::LDS_FLOATS);
  {   // the tile map is a permutation; the LDS image is injective and, for S lanes M apart, strided by an odd number
    std::vector<char> seen(t.outputs, 0);
    for (int64_t o = 0; o < t.outputs; ++o) {
      const int64_t j = pl::tile_offset(o, t.S, L);
      CHECK(j >= 0 && j < t.outputs && !seen[j]);
      seen[j] = 1;
      if (o % t.S) CHECK(j - pl::tile_offset(o - 1, t.S, L) == L);   // lanes of a group: outputs L apart, one phase
    }
    for (int w = 1; w < t.window; ++w) CHECK(pl::pad_index(w, t.shift) > pl::pad_index(w - 1, t.shift));
    if (t.window > M) CHECK(((pl::pad_index(M, t.shift) - pl::pad_index(0, t.shift)) & 1) == 1);
  }
  for (int n = 1; n <= 24; n += (n < 8 ? 1 : 5)) {
    const int64_t W = pl::n_out(n, L, M);
    CHECK(W == (n * (int64_t)L + M - 1) / M);
    std::unique_ptr<double[]> x(new double[n]);
    for (int k = 0; k < n; ++k) x[k] = sample(k);
    // one-shot, with a shorter valid length in a wider layout as well
    for (int nv : {n, n / 2, 0}) {
      const int64_t rows_out = pl::n_out(nv, L, M);
      std::unique_ptr<double[]> y(new double[W]);
      launch(f, t, G.get(), x.get(), 0, nv, rows_out, 0, W, y.get());
      for (int64_t m = 0; m < W; ++m) CHECK(y[m] == (m < rows_out ? direct(m, nv, h, f) : 0.0));
      for (int64_t m = 0; m < rows_out; ++m) {
        // (fewer taps than L: an output may have no tap at all, k_lo = k_hi + 1)
        CHECK(pl::centre(m, f) - pl::k_lo(m, f) * L <= 2 * (int64_t)f.half && pl::centre(m, f) - (pl::k_lo(m, f) - 1) * L > 2 * (int64_t)f.half);
        CHECK(pl::k_lo(m, f) <= pl::k_hi(m, f) + 1);
        CHECK(pl::k_hi(m, f) - pl::k_lo(m, f) < f.P);   // the P table columns cover every tap of the output
      }
    }
    // streams: every chunking below reproduces the one-shot outputs, each exactly once, from the history plan.h says to keep
    std::unique_ptr<double[]> want(new double[W]);
    for (int64_t m = 0; m < W; ++m) want[m] = direct(m, n, h, f);
    for (int scheme = 0; scheme < 8; ++scheme) {
      uint32_t lcg = 12345u + scheme;
      int64_t N = 0, E = 0, kbuf = 0;
      std::unique_ptr<double[]> hist(new double[0]);
      std::vector<double> got;
      bool closed = false;
      while (!closed) {
        int64_t c;
        if (scheme == 0) c = 1;
        else if (scheme == 1) c = 2;
        else if (scheme == 2) c = 3;
        else if (scheme == 3) c = n;        // everything at once
        else {
          lcg = lcg * 1664525u + 1013904223u;
          c = (lcg >> 16) % 6;              // zero-length chunks included
        }
        if (c > n - N) c = n - N;
        // schemes 0 .. 5 mark the final chunk `last`; 6 and 7 flush with an empty push afterwards
        const int last = (N + c == n && (scheme < 6 || c == 0)) ? 1 : 0;
        const int64_t N2 = N + c, E2 = pl::emitted(N2, last, f);
        CHECK(E2 >= E && E2 <= W);
        const int64_t keep = std::max<int64_t>(kbuf, pl::history_keep(E, N, f));
        CHECK(keep >= kbuf && keep <= N);
        if (E < W) CHECK(keep <= (pl::k_lo(E, f) < 0 ? 0 : pl::k_lo(E, f)) || keep == N);   // never above the first sample output E reads
        const int64_t tail = N - keep;
        std::unique_ptr<double[]> nb(new double[tail + c]);
        for (int64_t i = 0; i < tail; ++i) nb[i] = hist[keep - kbuf + i];
        for (int64_t i = 0; i < c; ++i) nb[tail + i] = x[N + i];
        hist = std::move(nb);
        kbuf = keep;
        N = N2;
        if (E2 > E) {
          std::unique_ptr<double[]> out(new double[E2 - E]);
          launch(f, t, G.get(), hist.get(), kbuf, N, E2, E, E2 - E, out.get());
          for (int64_t i = 0; i < E2 - E; ++i) got.push_back(out[i]);
          E = E2;
        }
        if (!last) {   // what exists without `last` needs no sample that has not arrived
          if (E > 0) CHECK(pl::k_hi(E - 1, f) <= N - 1);
          CHECK(pl::k_hi(E, f) >= N);
        }
        closed = last != 0;
      }
      CHECK(N == n && (int64_t)got.size() == W);
      for (int64_t m = 0; m < W; ++m) CHECK(got[m] == want[m]);
    }
  }
}

static int sweep() {
  long cases = 0;
  for (int L = 1; L <= 6; ++L)
    for (int M = 1; M <= 6; ++M) {
      if (pl::gcd(L, M) != 1) continue;
      for (int n_taps = 1; n_taps <= 15; n_taps += 2) {
        one_case(L, M, n_taps, pl::Tile(), false);
        // small tiles, so that rows span several: S and nrep forced
        for (int S : {1, 2, 4})
          for (int nrep : {1, 2}) {
            const pl::Filter f = pl::make_filter(n_taps, L, M);
            pl::Tile t;
            for (int m = M; !(m & 1); m >>= 1) ++t.shift;
            t.S = S;
            t.nrep = nrep;
            t.window = pl::tile_window(S, nrep, f);
            t.lds_floats = pl::pad_index(t.window - 1, t.shift) + 1;
            t.outputs = (int64_t)S * L * nrep;
            one_case(L, M, n_taps, t, true);
            ++cases;
          }
        ++cases;
      }
    }
  // the tile choice of the ratios served and of the corners of the limits
  const int shapes[][3] = {{160, 441, 14113}, {320, 441, 14113}, {320, 147, 10241}, {1, 6, 193}, {147, 320, 10241}, {2, 1, 65}, {1, 2, 65}, {3, 7, 29},
                           {1024, 1023, 32737}, {1023, 1024, 32769}, {1, 1024, 1023}, {1024, 1, 1024 * 1024 - 1}, {1, 1, 1}, {1, 1, 1023}};
  for (const auto& s : shapes) {
    CHECK(pl::filter_check(s[2], s[0], s[1]) == nullptr);
    const pl::Filter f = pl::make_filter(s[2], s[0], s[1]);
    const pl::Tile t = pl::choose_tile(f);
    CHECK(t.S >= 1 && t.S <= 64 && (t.S & (t.S - 1)) == 0 && pl::THREADS % t.S == 0 && t.nrep >= 1);
    CHECK(t.lds_floats <= pl::LDS_FLOATS && t.window == t.S * t.nrep * f.M + f.P && t.outputs >= 1);
    CHECK(((f.M + (t.shift ? f.M >> t.shift : 0)) & 1) == 1);   // the LDS stride of lanes M apart is odd
  }
  printf("OK %ld cases\n", cases);
  return 0;
}

static int big() {
  typedef __int128 i128;
  const int ratios[][3] = {{320, 441, 14113}, {160, 441, 14113}, {1024, 1023, 32737}, {1, 1024, 1023}, {1024, 1, 32767}};
  for (const auto& r : ratios) {
    const pl::Filter f = pl::make_filter(r[2], r[0], r[1]);
    for (int64_t n : {(int64_t)1 << 31, ((int64_t)1 << 31) + 12345, (int64_t)7000000, pl::MAX_N}) {
      const int64_t W = pl::n_out(n, f.L, f.M);
      CHECK((i128)W * f.M >= (i128)n * f.L && (i128)(W - 1) * f.M < (i128)n * f.L);
      for (int64_t m : {W - 1, W - 2, W / 2, (int64_t)0}) {
        if (m < 0) continue;
        const i128 c = (i128)m * f.M + f.half;
        CHECK((i128)pl::centre(m, f) == c);
        CHECK((i128)pl::k_hi(m, f) * f.L <= c && c - (i128)pl::k_hi(m, f) * f.L < f.L);
        CHECK((i128)pl::k_hi(m, f) * f.L + pl::phase(m, f) == c);
        const i128 lo = c - 2 * (i128)f.half;
        CHECK((i128)pl::k_lo(m, f) * f.L >= lo && ((i128)pl::k_lo(m, f) - 1) * f.L < lo);
        CHECK(pl::window_start(m, f) == pl::k_hi(m, f) - (f.P - 1));
      }
      if (f.M > 1 && n >= ((int64_t)1 << 31) && f.L >= 160) CHECK(pl::centre(W - 1, f) > ((int64_t)1 << 31));   // past int32
      const int64_t E = pl::emitted(n, 0, f);
      CHECK(E <= W && (E == 0 || pl::k_hi(E - 1, f) <= n - 1) && pl::k_hi(E, f) >= n);
      CHECK(pl::emitted(n, 1, f) == W);
      const int64_t hs = pl::history_start(E, f);
      CHECK(hs >= 0 && (hs == 0 || hs == pl::k_lo(E, f)));
      CHECK(pl::history_keep(E, n, f) <= n && n - pl::history_keep(E, n, f) <= (2 * (int64_t)f.half) / f.L + f.M / f.L + 2);   // bounded history
    }
  }
  printf("OK\n");
  return 0;
}

static int checks() {
  CHECK(pl::filter_check(65, 2, 1) == nullptr);
  CHECK(pl::filter_check(64, 2, 1) && pl::filter_check(0, 2, 1) && pl::filter_check(-3, 2, 1));                  // even / no taps
  CHECK(pl::filter_check(65, 2, 4) && pl::filter_check(65, 6, 3));                                                 // not coprime
  CHECK(pl::filter_check(65, 0, 1) && pl::filter_check(65, 1, 0) && pl::filter_check(65, 1025, 1) && pl::filter_check(65, 1, 1025) &&
        pl::filter_check(65, -2, 1));
  CHECK(pl::filter_check(1025, 1, 2) && pl::filter_check(1023, 1, 2) == nullptr);                                 // P <= 1024
  CHECK(pl::filter_check((int64_t)1024 * 1024 + 1, 1024, 1) && pl::filter_check((int64_t)1024 * 1024 - 1, 1024, 1) == nullptr);
  CHECK(pl::filter_check(INT64_MAX, 1024, 1023) && pl::filter_check(INT64_MIN + 1, 3, 2));
  CHECK(pl::forward_check(0, 10, 1, 10) == nullptr && pl::forward_check(1, 12, 4096, 10) == nullptr);
  CHECK(pl::forward_check(2, 10, 1, 10) && pl::forward_check(-1, 10, 1, 10));
  CHECK(pl::forward_check(0, 10, 0, 10) && pl::forward_check(0, 10, 4097, 10));
  CHECK(pl::forward_check(0, 10, 1, 0) && pl::forward_check(0, 9, 1, 10) && pl::forward_check(0, INT64_MAX, 1, pl::MAX_N + 1));
  CHECK(pl::floor_div(-1, 3) == -1 && pl::floor_div(-3, 3) == -1 && pl::floor_div(2, 3) == 0 && pl::ceil_div(1, 3) == 1 && pl::ceil_div(-1, 3) == 0 &&
        pl::ceil_div(0, 3) == 0 && pl::ceil_div(3, 3) == 1);
  printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc >= 2 && !strcmp(argv[1], "big")) return big();
  if (argc >= 2 && !strcmp(argv[1], "checks")) return checks();
  if (argc >= 5 && !strcmp(argv[1], "tile")) {
    const int L = atoi(argv[2]), M = atoi(argv[3]), n_taps = atoi(argv[4]);
    if (const char* m = pl::filter_check(n_taps, L, M)) {
      printf("ERR %s\n", m);
      return 0;
    }
    const pl::Filter f = pl::make_filter(n_taps, L, M);
    const pl::Tile t = pl::choose_tile(f);
    printf("S=%d nrep=%d shift=%d window=%d lds=%d outputs=%lld P=%d half=%d\n", t.S, t.nrep, t.shift, t.window, t.lds_floats, (long long)t.outputs, f.P, f.half);
    return 0;
  }
  fprintf(stderr, "usage: resample_plan_test sweep | big | checks | tile L M n_taps\n");
  return 2;
}
