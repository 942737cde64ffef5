// e2e_tts_amd/csrc/f0/plan.h as a stand-alone CPU program, built by tests/test_f0_sanitizer.py with g++ -fsanitize=address,undefined.
// Every buffer is a heap allocation of exactly the size plan.h promises, so an index outside it is a sanitizer report.
// Modes: sweep | big | checks | tile SR HOP FLOOR CEILING
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../e2e_tts_amd/csrc/f0/plan.h"

namespace pl = e2ef0_plan;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(2);                                                              \
    }                                                                       \
  } while (0)

// the analysis kernel's walk over one row of n samples, on heap buffers of the planned sizes: what it stages, where a wavefront's `a`,
// its row of lags and its candidate list lie, and the furthest element the lag loop reads
static long walk_row(const pl::Geometry& g, int64_t n) {
  const int64_t T = pl::frames_of(n, g.hop);
  std::vector<float> x((size_t)n);
  for (int64_t s = 0; s < n; ++s) x[(size_t)s] = (float)(s % 251) - 125.f;
  long frames = 0;
  for (int64_t tile = 0; tile < pl::tiles_of(T, g.F); ++tile) {
    std::vector<float> lds((size_t)g.lds_floats);   // exactly the dynamic LDS of the launch
    const int stage4 = pl::round_up(g.stage, 4);
    CHECK(stage4 + pl::WAVES * g.AL + pl::WAVES * g.NL4 == g.lds_floats && (int64_t)g.lds_floats * 4 <= pl::LDS_BYTES);
    const int64_t t0 = tile * g.F;
    const int nf = (int)(T - t0 < g.F ? T - t0 : g.F);
    const int64_t s0 = pl::first_sample(t0, g.hop, g.h);
    const int need = (nf - 1) * g.hop + g.W;
    CHECK(need <= g.stage);
    for (int j = 0; j < need; ++j) {
      const int64_t s = s0 + j;
      lds[(size_t)j] = (s >= 0 && s < n) ? x[(size_t)s] : 0.f;
    }
    for (int fi = 0; fi < nf; ++fi) {
      const int wv = fi % pl::WAVES;
      const int64_t t = t0 + fi;
      const float* xs = lds.data() + pl::frame_offset(t, t0, g.hop);
      float* a = lds.data() + stage4 + wv * g.AL;
      float* r = lds.data() + stage4 + pl::WAVES * g.AL + wv * g.NL4;
      CHECK((stage4 + wv * g.AL) % 4 == 0 && (stage4 + pl::WAVES * g.AL + wv * g.NL4) % 4 == 0);   // 16-byte words
      // the window is the definition's: sample centre(t) - h + i, zeros outside [0, n)
      for (int i = 0; i < g.W; ++i) {
        const int64_t s = pl::centre(t, g.hop) - g.h + i;
        CHECK(xs[i] == ((s >= 0 && s < n) ? x[(size_t)s] : 0.f));
      }
      for (int i = 0; i < g.AL; ++i) a[i] = i < g.W ? xs[i] : 0.f;
      for (int tau0 = 0; tau0 < g.NL4; tau0 += 4) {
        float acc[4] = {0, 0, 0, 0};
        for (int i0 = 0; i0 < g.Wp; i0 += 4)
          for (int q = 0; q < 4; ++q)
            for (int k = 0; k < 4; ++k) acc[k] += a[i0 + q] * a[i0 + q + tau0 + k];   // the words [i0 + tau0, i0 + tau0 + 8) are read whole
        CHECK(g.Wp - 4 + tau0 + 7 < g.AL);
        (void)a[g.Wp - 4 + tau0 + 7];
        for (int k = 0; k < 4; ++k) r[tau0 + k] = acc[k];
      }
      // the zero tail makes the padded sum the definition's: lag tau over i < W - tau
      for (int tau = 0; tau < g.NL; tau += (g.NL > 8 ? g.NL / 8 : 1)) {
        float d = 0.f;
        for (int i = 0; i + tau < g.W; ++i) d += a[i] * a[i + tau];
        CHECK(d == r[tau] || (d != d));
      }
      // the candidate list reuses `a`: three arrays of NC entries; at most every second lag of [tau_min, tau_max] is a maximum
      CHECK(3 * g.NC <= g.AL && (g.tau_max - g.tau_min + 2) / 2 <= g.NC);
      for (int c = 0; c < 3 * g.NC; ++c) a[c] = 0.f;
      CHECK(g.tau_min - 1 >= 1 && g.tau_max + 1 <= g.NL - 1);   // r[tau - 1] and r[tau + 1] of every candidate lag exist
      ++frames;
    }
  }
  CHECK(frames == T);
  return frames;
}

static int sweep() {
  long frames = 0, geos = 0;
  const int rates[] = {1000, 1600, 2205, 4000, 8000};
  const double floors[] = {40.0, 61.5, 80.0, 133.0};
  for (int sr : rates)
    for (double fl : floors)
      for (int hop : {1, 7, 16, 50, 128, 257}) {
        pl::Geometry g;
        const double ce = fl * 6.3;
        const char* m = pl::geometry(sr, hop, fl, ce, &g);
        if (m) continue;
        ++geos;
        CHECK(g.W % 2 == 1 && g.h * 2 + 1 == g.W && g.W >= (int)(3.0 * sr / fl) && g.W <= (int)(3.0 * sr / fl) + 1);
        CHECK(g.tau_max == (int)(sr / fl) && g.tau_min >= 2 && (double)g.tau_min * ce >= sr && (double)(g.tau_min - 1) * ce < sr);
        CHECK(g.NL == g.tau_max + 2 && g.NL < g.W && g.F % pl::WAVES == 0 && g.F >= pl::WAVES && g.F <= pl::MAX_TILE);
        for (int64_t n : {(int64_t)0, (int64_t)hop - 1, (int64_t)hop, (int64_t)g.W - 1, (int64_t)2 * g.F * hop + hop / 2, (int64_t)(g.F + 1) * hop + 1})
          if (n >= 0 && n < 40000) frames += walk_row(g, n);
      }
  CHECK(geos >= 40);
  printf("OK %ld geometries, %ld frames\n", geos, frames);
  return 0;
}

static int big() {
  // frame positions near the limits against __int128
  for (int hop : {1, 128, 256, 512, 48000})
    for (int64_t n : {pl::MAX_N, pl::MAX_N - 1, (int64_t)1 << 31, ((int64_t)1 << 31) + 12345}) {
      const int64_t T = pl::frames_of(n, hop);
      CHECK((__int128)T * hop <= n && (__int128)(T + 1) * hop > n);
      for (int64_t t : {(int64_t)0, T / 2, T - 1}) {
        if (t < 0) continue;
        const __int128 c = (__int128)t * hop + hop / 2;
        CHECK((__int128)pl::centre(t, hop) == c && c < (__int128)n);
        CHECK((__int128)pl::first_sample(t, hop, 900) == c - 900);
      }
    }
  CHECK(pl::batch_check(1, pl::MAX_N, pl::MAX_N, 256, 16) == nullptr);    // 2^24 frames of 16 candidates
  CHECK(pl::batch_check(1, pl::MAX_N, pl::MAX_N, 128, 16) != nullptr);    // 2^25 frames
  CHECK(pl::batch_check(4096, (int64_t)1 << 20, (int64_t)1 << 20, 256, 602) != nullptr);   // 2^24 frames * 602 lags
  printf("OK\n");
  return 0;
}

static int checks() {
  pl::Geometry g;
  CHECK(pl::geometry(22050, 256, 80, 750, &g) == nullptr && g.W == 827 && g.tau_min == 30 && g.tau_max == 275);
  CHECK(pl::geometry(16000, 128, 80, 750, &g) == nullptr && g.W == 601 && g.tau_min == 22 && g.tau_max == 200);
  CHECK(pl::geometry(48000, 512, 80, 750, &g) == nullptr && g.W == 1801 && g.tau_min == 64 && g.tau_max == 600);
  const pl::Geometry keep = g;
  CHECK(pl::geometry(999, 256, 80, 750, &g) && pl::geometry(384001, 256, 80, 750, &g));
  CHECK(pl::geometry(22050, 0, 80, 750, &g) && pl::geometry(22050, 22051, 80, 750, &g));
  CHECK(pl::geometry(22050, 256, 0, 750, &g) && pl::geometry(22050, 256, -1, 750, &g) && pl::geometry(22050, 256, 80, 80, &g));
  CHECK(pl::geometry(22050, 256, 80, HUGE_VAL, &g));                                        // infinity
  CHECK(pl::geometry(22050, 256, 1e-9, 750, &g));                                          // a window of 10^13 samples: refused, not cast
  CHECK(pl::geometry(22050, 256, 80, 30000, &g) && strstr(pl::geometry(22050, 256, 80, 30000, &g), "tau_min"));
  CHECK(pl::geometry(48000, 512, 40, 750, &g) && strstr(pl::geometry(48000, 512, 40, 750, &g), "LDS"));
  CHECK(g.W == keep.W && g.F == keep.F);                                                   // a refusal leaves *g alone
  const size_t sz = 72;
  CHECK(pl::params_check(sz, sz, 0.5, 0.03, 0.01, 0.35, 0.14, 15) == nullptr);
  CHECK(pl::params_check(sz - 8, sz, 0.5, 0.03, 0.01, 0.35, 0.14, 15));
  CHECK(pl::params_check(sz, sz, -0.1, 0.03, 0.01, 0.35, 0.14, 15) && pl::params_check(sz, sz, 0.5, 0.0, 0.01, 0.35, 0.14, 15));
  CHECK(pl::params_check(sz, sz, 0.5, 0.03, -1, 0.35, 0.14, 15) && pl::params_check(sz, sz, 0.5, 0.03, 0.01, HUGE_VAL, 0.14, 15));
  CHECK(pl::params_check(sz, sz, 0.5, 0.03, 0.01, 0.35, -0.14, 15));
  CHECK(pl::params_check(sz, sz, 0.5, 0.03, 0.01, 0.35, 0.14, 1) && pl::params_check(sz, sz, 0.5, 0.03, 0.01, 0.35, 0.14, 17));
  CHECK(pl::params_check(sz, sz, 0.5, 0.03, 0.01, 0.35, 0.14, 2) == nullptr && pl::params_check(sz, sz, 0.5, 0.03, 0.01, 0.35, 0.14, 16) == nullptr);
  CHECK(pl::batch_check(3, 1000, 1000, 256, 277) == nullptr && pl::batch_check(0, 1000, 1000, 256, 277) && pl::batch_check(4097, 1000, 1000, 256, 277));
  CHECK(pl::batch_check(3, 0, 1000, 256, 277) && pl::batch_check(3, 1000, 999, 256, 277) && pl::batch_check(3, pl::MAX_N + 1, pl::MAX_N + 1, 256, 277));
  printf("OK\n");
  return 0;
}

static int tile(int sr, int hop, double fl, double ce) {
  pl::Geometry g;
  const char* m = pl::geometry(sr, hop, fl, ce, &g);
  if (m) {
    printf("ERR %s\n", m);
    return 0;
  }
  printf("W=%d tau=[%d,%d] lags=%d AL=%d F=%d stage=%d lds_bytes=%d\n", g.W, g.tau_min, g.tau_max, g.NL, g.AL, g.F, g.stage, g.lds_floats * 4);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "sweep") return sweep();
  if (mode == "big") return big();
  if (mode == "checks") return checks();
  if (mode == "tile" && argc == 6) return tile(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atof(argv[5]));
  fprintf(stderr, "usage: f0_plan_test sweep | big | checks | tile SR HOP FLOOR CEILING\n");
  return 1;
}
