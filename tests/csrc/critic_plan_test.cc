// Stand-alone program around e2e_tts_amd/csrc/critic/plan.h (the HIP-free half of libe2etts_critic.so), built by
// tests/test_critic_sanitizer.py with g++ -fsanitize=address,undefined and run on the CPU.
//   sweep          lengths 12 .. 700 and a few long ones through the default and the quarter tables: the rows every launch covers hold
//                  every sequence and what the next dense layer's fold reads; the folded convolution on buffers of exactly the planned
//                  sizes equals the strided one on integer data; the grouped kernel's staging and fragment reads stay inside the planned
//                  LDS image and every word read was written, for the planned tile and forced ones
//   lens N         the score lengths of the default tables for a row of N samples
//   checks         the argument checks and the refusals by name
//   cap            rows per pass under the workspace cap
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../e2e_tts_amd/csrc/critic/plan.h"

namespace pl = e2ecr_plan;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static std::vector<pl::Disc> tables(int div) {
  const int periods[5] = {2, 3, 5, 7, 11};
  const pl::LayerSpec mpd[5] = {{32 / div, 5, 3, 1, 2}, {128 / div, 5, 3, 1, 2}, {512 / div, 5, 3, 1, 2}, {1024 / div, 5, 3, 1, 2}, {1024 / div, 5, 1, 1, 2}};
  const int gd = div;
  auto gr = [&](int g) { return g / gd < 1 ? 1 : g / gd; };
  const pl::LayerSpec msd[7] = {{128 / div, 15, 1, 1, 7},         {128 / div, 41, 2, gr(4), 20},   {256 / div, 41, 2, gr(16), 20}, {512 / div, 41, 4, gr(16), 20},
                                {1024 / div, 41, 4, gr(16), 20}, {1024 / div, 41, 1, gr(16), 20}, {1024 / div, 5, 1, 1, 2}};
  const pl::LayerSpec post = {1, 3, 1, 1, 1};
  std::vector<pl::Disc> out;
  for (int i = 0; i < 5 + 3; ++i) {
    pl::Disc d;
    const bool per = i < 5;
    if (per) d.period = periods[i];
    else d.scale = i - 5;
    d.n_layers = per ? 5 : 7;
    int cin = 1;
    for (int l = 0; l <= d.n_layers; ++l) {
      const pl::LayerSpec& s = l < d.n_layers ? (per ? mpd[l] : msd[l]) : post;
      const char* m = pl::layer_plan(s, cin, l == 0, l == d.n_layers, &d.layer[l]);
      if (m) {
        fprintf(stderr, "layer_plan: %s\n", m);
        exit(1);
      }
      cin = s.cout;
    }
    out.push_back(d);
  }
  return out;
}

// the folded convolution against the strided one, one channel in, integer data, on buffers of exactly the planned row counts
static void fold_case(int k, int s, int pad, int n, int64_t rows_in, int64_t rows_out) {
  const pl::Fold f = pl::fold_of(k, s, pad);
  CHECK(f.q <= f.kf - 1 || k <= pad);
  std::vector<long> x((size_t)rows_in, 0), w((size_t)k);
  for (int i = 0; i < n; ++i) x.at(i) = (i * 7 + 3) % 11 - 5;
  for (int j = 0; j < k; ++j) w.at(j) = (j * 5 + 1) % 7 - 3;
  const int64_t to = pl::out_len(n, k, s, pad);
  CHECK(rows_out >= to && rows_in >= s * rows_out);
  for (int64_t t = 0; t < rows_out; ++t) {
    long direct = 0, folded = 0;
    for (int j = 0; j < k; ++j) {
      const int64_t i = t * s - pad + j;
      if (i >= 0 && i < n) direct += w.at(j) * x.at(i);
    }
    for (int jf = 0; jf < f.kf; ++jf) {
      const int64_t r = t - f.q + jf;   // folded row; rows outside [0, rows_out) read as zero, as conv_gemm reads them
      if (r < 0 || r >= rows_out) continue;
      for (int ph = 0; ph < s; ++ph) {
        const int j = pl::fold_tap(f, s, jf, ph);
        if (j >= 0 && j < k) folded += w.at(j) * x.at(r * s + ph);
      }
    }
    if (t < to) CHECK(direct == folded);
  }
}

static void group_case(const pl::Layer& L, int tm_forced) {
  pl::GroupPlan g;
  const char* m = pl::group_plan(L.cin, L.cout, L.k, L.stride, L.groups, tm_forced, &g);
  if (m) {
    CHECK(tm_forced > 0);   // a forced tile may not fit; the planned one must
    return;
  }
  CHECK((int64_t)g.lds_floats * 4 <= pl::LDS_BYTES && g.tm % 64 == 0 && g.waves >= 1 && g.waves <= 4);
  std::vector<char> written((size_t)g.lds_floats, 0);
  const int wr = (g.tm - 1) * L.stride + L.k;
  for (int r = 0; r < wr; ++r)
    for (int c = 0; c < g.cin_g; ++c) {
      char& slot = written.at((size_t)pl::group_lds_index(g, L.stride, r, c));
      CHECK(!slot);   // no two window elements share a word
      slot = 1;
    }
  for (int mp = 0; mp < g.tm / 64; ++mp)
    for (int j = 0; j < L.k; ++j)
      for (int c2 = 0; c2 < g.cin_g / 2; ++c2)
        for (int lane = 0; lane < 64; ++lane)
          for (int half = 0; half < 2; ++half) {
            const int li = lane & 31, lh = lane >> 5;
            const int idx = 2 * c2 * g.cstride + (j % L.stride) * g.prow + j / L.stride + mp * 64 + li + lh * g.cstride + 32 * half;   // the kernel's expression
            CHECK(written.at((size_t)idx));
            CHECK(idx == pl::group_lds_index(g, L.stride, (mp * 64 + 32 * half + li) * L.stride + j, 2 * c2 + lh));
          }
  CHECK(pl::group_frag_floats(L.cin, L.cout, L.k, L.groups) == (int64_t)L.groups * g.ntp * L.k * (g.cin_g / 2) * 64);
}

static int sweep() {
  long cases = 0;
  for (int div : {1, 4}) {
    const std::vector<pl::Disc> discs = tables(div);
    std::vector<int> ns;
    for (int n = 12; n <= 700; ++n) ns.push_back(n);
    for (int n : {1500, 2049, 2050, 3001, 22050, 196608, 1 << 24}) ns.push_back(n);
    for (const pl::Disc& d : discs) {
      for (int n : ns) {
        int64_t len[pl::MAX_MAPS + 1], rows[pl::MAX_MAPS];
        pl::disc_lens(d, n, len);
        pl::launch_rows(d, len, rows);
        for (int l = 0; l <= d.n_layers; ++l) {
          const pl::Layer& L = d.layer[l];
          CHECK(len[1 + l] >= 1 && rows[l] >= len[1 + l]);
          CHECK(len[1 + l] == (len[l] + 2 * L.pad - L.k) / L.stride + 1);
          if (L.kind == pl::DENSE) {
            CHECK(rows[l] >= pl::ceil_div(len[l], L.stride) && rows[l - 1] >= L.stride * rows[l]);
            if (n <= 700 || n == 3001) fold_case(L.k, L.stride, L.pad, (int)len[l], rows[l - 1], rows[l]);
          }
        }
        CHECK(pl::disc_buffer_floats(d, n) >= rows[0] * d.layer[0].cout * pl::disc_cols(d));
        for (int l = 0; l <= d.n_layers; ++l)
          if (d.layer[l].kind == pl::DENSE && d.layer[l].splits > 1)
            CHECK(pl::disc_partial_floats(d, n) >= rows[l] * d.layer[l].cout * pl::disc_cols(d) * d.layer[l].splits);
        ++cases;
      }
      for (int l = 0; l <= d.n_layers; ++l)
        if (d.layer[l].kind == pl::GROUPED)
          for (int tm : {0, 64, 128, 256, 512}) group_case(d.layer[l], tm);
    }
  }
  // folds the tables do not hold
  const int extra[][3] = {{7, 4, 1}, {3, 5, 0}, {5, 3, 2}, {5, 1, 2}, {4, 2, 3}, {9, 8, 4}};
  for (const auto& e : extra)
    for (int n = 1; n <= 64; ++n) {
      const pl::Fold f = pl::fold_of(e[0], e[1], e[2]);
      const int64_t to = pl::out_len(n, e[0], e[1], e[2]);
      int64_t r = pl::ceil_div(n, e[1]);
      if (to > r) r = to;
      if (r < 1) r = 1;
      if (f.q <= f.kf - 1) fold_case(e[0], e[1], e[2], n, r * e[1], r);
    }
  // the reflect extension stays inside the row for every accepted length
  for (int p = 1; p <= pl::MAX_PERIOD; ++p)
    for (int n = p + 1; n <= 4 * p + 3; ++n)
      for (int64_t i = 0; i < pl::period_rows(n, p) * p; ++i) {
        const int64_t j = pl::reflect_index(i, n);
        CHECK(j >= 0 && j < n);
      }
  printf("OK %ld\n", cases);
  return 0;
}

static int lens(int n) {
  const std::vector<pl::Disc> discs = tables(1);
  std::string out;
  for (const pl::Disc& d : discs) {
    int64_t len[pl::MAX_MAPS + 1];
    pl::disc_lens(d, n, len);
    out += std::to_string((long long)(len[1 + d.n_layers] * pl::disc_cols(d))) + " ";
  }
  printf("%s\n", out.c_str());
  return 0;
}

static int checks() {
  CHECK(pl::batch_check(1, 12, 0) == nullptr && pl::batch_check(0, 12, 0) && pl::batch_check(4097, 12, 0) && pl::batch_check(1, 0, 0) && pl::batch_check(1, 12, 2));
  CHECK(pl::batch_check(1, (1 << 24) + 1, 0) && pl::batch_check(pl::MAX_B, pl::MAX_LEN, 1) == nullptr);
  CHECK(pl::len_check(12, 12, 12) == nullptr && pl::len_check(11, 12, 12) && pl::len_check(13, 12, 12));
  pl::Layer L;
  auto refused = [&](pl::LayerSpec s, int cin, bool first, bool post, const char* word) {
    const char* m = pl::layer_plan(s, cin, first, post, &L);
    return m && strstr(m, word);
  };
  CHECK(refused({128, 41, 2, 4, 20}, 24, false, false, "Cin / groups must be a multiple of 8"));
  CHECK(refused({40, 41, 2, 4, 20}, 128, false, false, "Cout / groups must be a multiple of 16"));
  CHECK(refused({128, 41, 2, 3, 20}, 128, false, false, "groups must divide"));
  CHECK(refused({1024, 41, 8, 2, 20}, 1024, false, false, "does not fit 64 KiB"));
  CHECK(refused({30, 5, 3, 1, 2}, 32, false, false, "multiples of 4"));
  CHECK(refused({2, 3, 1, 1, 1}, 32, false, true, "post layer"));
  CHECK(refused({32, 5, 3, 2, 2}, 1, true, false, "first layer"));
  CHECK(refused({32, 65, 1, 1, 2}, 32, false, false, "k in [1, 64]"));
  CHECK(refused({32, 5, 1, 1, 5}, 32, false, false, "pad < k"));
  CHECK(pl::layer_plan({256, 41, 2, 16, 20}, 128, false, false, &L) == nullptr && L.kind == pl::GROUPED && L.gp.cin_g == 8 && L.gp.cout_g == 16 && L.gp.ntp == 1);
  CHECK(pl::layer_plan({128, 5, 3, 1, 2}, 32, false, false, &L) == nullptr && L.kind == pl::DENSE && L.fold.q == 1 && L.fold.o == 1 && L.fold.kf == 2);
  pl::GroupPlan g;
  CHECK(pl::group_plan(128, 128, 41, 2, 4, 96, &g) && pl::group_plan(128, 128, 41, 2, 4, 2048, &g));
  printf("OK\n");
  return 0;
}

static int cap() {
  CHECK(pl::rows_per_pass(1000, 0, 0, 2) == pl::DEFAULT_CAP / 8000 / 2 * 2);
  CHECK(pl::rows_per_pass((int64_t)1 << 40, 0, 1 << 20, 2) == 2 && pl::rows_per_pass((int64_t)1 << 40, 0, 1 << 20, 1) == 1);
  CHECK(pl::rows_per_pass(1 << 20, 0, (int64_t)24 << 20, 2) == 2 && pl::rows_per_pass(1 << 20, 0, (int64_t)40 << 20, 2) == 4);
  CHECK(pl::rows_per_pass(1 << 20, 2 << 20, (int64_t)40 << 20, 2) == 2);   // the partial sums count against the cap
  // the K split: whole 32-channel chunks, chains of at least 128 terms, at most 8 ranges
  CHECK(pl::dense_splits(96, 2) == 1 && pl::dense_splits(384, 2) == 4 && pl::dense_splits(1536, 2) == 8 && pl::dense_splits(1024, 5) == 8);
  CHECK(pl::dense_splits(24, 2) == 1 && pl::dense_splits(64, 1) == 1 && pl::dense_splits(256, 1) == 2 && pl::dense_splits(4096 * 8, 64) == 8);
  for (int c = 4; c <= 4096; c += 4)
    for (int kf = 1; kf <= 8; ++kf) {
      const int n = pl::dense_splits(c, kf);
      CHECK(n >= 1 && n <= pl::MAX_SPLITS && (n & (n - 1)) == 0 && (n == 1 || (c % (32 * n) == 0 && (int64_t)c * kf / n >= 128)));
    }
  printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc >= 3 && !strcmp(argv[1], "lens")) return lens(atoi(argv[2]));
  if (argc >= 2 && !strcmp(argv[1], "checks")) return checks();
  if (argc >= 2 && !strcmp(argv[1], "cap")) return cap();
  fprintf(stderr, "usage: critic_plan_test sweep | lens N | checks | cap\n");
  return 2;
}
