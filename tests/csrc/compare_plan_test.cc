// e2e_tts_amd/csrc/compare/plan.h as a stand-alone CPU program, built by tests/test_compare_sanitizer.py with g++ -fsanitize=address,undefined.
// Every buffer is a heap allocation of exactly the size plan.h promises, so an index outside it is a sanitizer report.
// Modes: sweep | caps | checks | lds N_MEL N_CEP
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../../e2e_tts_amd/csrc/compare/plan.h"

namespace pl = e2ecmp_plan;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(2);                                                              \
    }                                                                       \
  } while (0)

// the search kernel's walk over one pair on heap buffers of the planned sizes: the chunks of thread rows, the diagonals of a chunk, the
// two exchange rows and the handed-on row in an LDS image of exactly search_lds_doubles(L), the back-pointer words; then the walk
// kernel's back-track over those words into a path buffer of path_cells().  The recurrence runs on an integer cost so that the result
// can be compared with a plain row-by-row DP.
static long walk_pair(int Ta, int Tb, long long band, int NT) {
  const bool sw = pl::swapped(Ta, Tb);
  const int S = sw ? Tb : Ta, L = sw ? Ta : Tb;
  const double INF = std::numeric_limits<double>::infinity();
  auto cost = [&](int i, int j) { return (double)((i * 7 + j * 13 + (i ^ j)) % 5); };   // ties abound
  std::vector<uint32_t> words((size_t)pl::bp_words(Ta, Tb), 0xdeadbeefu);
  std::vector<unsigned char> written((size_t)pl::bp_words(Ta, Tb) * pl::BP_CELLS, 0);
  std::vector<double> lds((size_t)pl::search_lds_doubles(L, NT));
  CHECK((int64_t)lds.size() * 8 <= pl::LDS_BYTES);
  double* ex = lds.data();
  double* bound = lds.data() + 2 * NT;
  double total = std::numeric_limits<double>::quiet_NaN();
  for (int c0 = 0; c0 < S; c0 += NT) {
    std::vector<double> own_prev(NT, INF), diag(NT, INF);
    for (int tid = 0; tid < NT; ++tid) ex[NT + tid] = INF;
    const bool hand_on = c0 + NT < S;
    const int rows = S - c0 < NT ? S - c0 : NT;
    const int nd = rows + L - 1;
    for (int dd = 0; dd < nd; ++dd) {
      std::vector<double> vals(NT, INF);
      std::vector<int> codes(NT, 0), acts(NT, 0);
      for (int tid = 0; tid < NT; ++tid) {
        const int s = c0 + tid, l = dd - tid;
        const bool act = s < S && l >= 0 && l < L;
        double nb;
        if (tid > 0) nb = ex[((dd & 1) ^ 1) * NT + tid - 1];
        else nb = (c0 > 0 && l < L) ? bound[l] : INF;
        double val = INF;
        int code = 0;
        if (act) {
          const int i = sw ? l : s, j = sw ? s : l;
          if (pl::band_allows(i, j, Ta, Tb, band)) {
            const double up = sw ? own_prev[tid] : nb, left = sw ? nb : own_prev[tid];
            double best = diag[tid];
            if (up < best) best = up, code = 1;
            if (left < best) best = left, code = 2;
            val = (s == 0 && l == 0) ? cost(i, j) : cost(i, j) + best;
          }
        }
        diag[tid] = nb;
        own_prev[tid] = val;
        vals[tid] = val, codes[tid] = code, acts[tid] = act;
      }
      for (int tid = 0; tid < NT; ++tid) {   // after every thread has read: the kernel's barrier
        const int s = c0 + tid, l = dd - tid;
        ex[(dd & 1) * NT + tid] = vals[tid];
        if (hand_on && tid == NT - 1 && acts[tid]) {
          CHECK(l >= 0 && l < pl::round_up(L, 2) && l + NT - 1 == dd);   // thread 0 reads bound[dd]: THREADS - 1 ahead
          bound[l] = vals[tid];
        }
        if (acts[tid]) {
          const int64_t w = pl::bp_word(c0 + dd, s, S);
          CHECK(w >= 0 && w < (int64_t)words.size() && c0 + dd == s + l);
          const size_t cell = (size_t)w * pl::BP_CELLS + (size_t)pl::bp_shift(s) / 2;
          CHECK(!written[cell]);   // no two cells share their two bits
          written[cell] = 1;
          if (words[(size_t)w] == 0xdeadbeefu) words[(size_t)w] = 0;
          words[(size_t)w] |= (uint32_t)codes[tid] << pl::bp_shift(s);
          if (s == S - 1 && l == L - 1) total = vals[tid];
        }
      }
    }
  }
  // the plain DP
  std::vector<double> D((size_t)Ta * Tb, INF);
  for (int i = 0; i < Ta; ++i)
    for (int j = 0; j < Tb; ++j) {
      if (!pl::band_allows(i, j, Ta, Tb, band)) continue;
      double best = (i && j) ? D[(size_t)(i - 1) * Tb + j - 1] : INF;
      if (i && D[(size_t)(i - 1) * Tb + j] < best) best = D[(size_t)(i - 1) * Tb + j];
      if (j && D[(size_t)i * Tb + j - 1] < best) best = D[(size_t)i * Tb + j - 1];
      D[(size_t)i * Tb + j] = (i == 0 && j == 0) ? cost(0, 0) : cost(i, j) + best;
    }
  CHECK(total == D.back());
  if (!(total < INF)) return 0;
  // the walk kernel's back-track
  std::vector<uint32_t> cells((size_t)pl::path_cells(Ta, Tb));
  CHECK(cells.size() <= (size_t)(2 * pl::MAX_T - 1));
  int i = Ta - 1, j = Tb - 1;
  size_t N = 0;
  double sum = 0;
  for (;;) {
    CHECK(N < cells.size());
    cells[N++] = pl::pack_cell(i, j);
    CHECK(pl::cell_i(cells[N - 1]) == i && pl::cell_j(cells[N - 1]) == j);
    sum += cost(i, j);
    if (i == 0 && j == 0) break;
    int code;
    if (i == 0) code = 2;
    else if (j == 0) code = 1;
    else {
      const int s = sw ? j : i;
      const int64_t w = pl::bp_word(i + j, s, S);
      CHECK(w >= 0 && w < (int64_t)words.size());
      code = (int)((words[(size_t)w] >> pl::bp_shift(s)) & 3u);
    }
    if (code == 1) --i;
    else if (code == 2) --j;
    else --i, --j;
    CHECK(i >= 0 && j >= 0);
  }
  CHECK(sum == total);   // integer costs: exact
  return (long)N;
}

static int sweep() {
  long cells = 0;
  int pairs = 0;
  const int lens[] = {1, 2, 3, 15, 16, 17, 40, 63, 64, 65, 255, 256, 257, 300, 511, 513, 600, 1100};
  for (int Ta : lens)
    for (int Tb : lens) {
      if ((long)Ta * Tb > 160000 && !(Ta == 1100 && Tb == 1100)) continue;
      for (long long band : {-1LL, 0LL, 1LL, 2LL, 8LL}) {
        // the workgroup the library launches for this pair alone with D <= 16 and with wider rows, and smaller ones (a batch's longest
        // pair decides): every size gives the plain DP's total
        const int S = Ta < Tb ? Ta : Tb;
        const int nt = pl::search_threads(16, S), nt_wide = pl::search_threads(64, S);
        CHECK(nt % 64 == 0 && nt <= 1024 && nt_wide % 64 == 0 && nt_wide <= 256 && (nt >= S || nt == 1024) && (nt_wide >= S || nt_wide == 256));
        CHECK(pl::search_threads(32, S) <= 512 && pl::search_threads(32, S) >= nt_wide && pl::search_threads(20, 4096) == 512);
        const long n = walk_pair(Ta, Tb, band, nt);
        if (band == -1 || band == 2) {
          CHECK(walk_pair(Ta, Tb, band, 64) == n);
          if (nt_wide != nt) CHECK(walk_pair(Ta, Tb, band, nt_wide) == n);
        }
        if (band != 0) CHECK(n >= (Ta > Tb ? Ta : Tb));   // every band >= 1 holds a path
        cells += n;
        ++pairs;
      }
    }
  // the cepstra kernel's LDS image: basis rows, then the tile's rows
  int plans = 0;
  for (int n_mel = 1; n_mel <= pl::MAX_MEL; n_mel += (n_mel < 140 ? 1 : 37))
    for (int n_cep : {1, 13, 64}) {
      pl::CepPlan p;
      if (pl::cep_plan(n_mel, n_cep, &p)) continue;
      CHECK(p.stride % 4 == 0 && (p.stride / 4) % 2 == 1 && p.stride >= pl::round_up(n_mel, 4) + 4);
      CHECK((int64_t)p.lds_floats * 4 <= pl::LDS_BYTES && p.tile >= 4);
      std::vector<float> lds((size_t)p.lds_floats);
      float* sb = lds.data();
      float* sm = lds.data() + n_cep * p.stride;
      for (int idx = 0; idx < n_cep * p.stride; ++idx) sb[idx] = 1.f;
      const int M4 = pl::round_up(n_mel, 4);
      for (int f = 0; f < p.tile; ++f)
        for (int m = 0; m < M4; ++m) sm[f * p.stride + m] = 2.f;
      float acc = 0;
      for (int m = 0; m < M4; m += 4) acc += sb[(n_cep - 1) * p.stride + m + 3] * sm[(p.tile - 1) * p.stride + m + 3];   // the last word of the last rows
      CHECK(acc > 0);
      ++plans;
    }
  printf("OK %d pairs, %ld path cells, %d cepstra plans\n", pairs, cells, plans);
  return 0;
}

static int caps() {
  typedef __int128 i128;
  const int64_t T = pl::MAX_T;
  // the band at the caps
  for (int64_t i : {(int64_t)0, T / 2, T - 1})
    for (int64_t j : {(int64_t)0, T / 3, T - 1})
      for (int64_t Ta : {(int64_t)1, T - 1, T})
        for (int64_t Tb : {(int64_t)1, T / 2 + 1, T})
          for (int64_t band : {(int64_t)0, (int64_t)1, (int64_t)4095, pl::MAX_BAND}) {
            if (i >= Ta || j >= Tb) continue;
            i128 dev = (i128)i * Tb - (i128)j * Ta;
            if (dev < 0) dev = -dev;
            const bool want = dev <= (i128)band * (Ta > Tb ? Ta : Tb);
            CHECK(pl::band_allows(i, j, Ta, Tb, band) == want);
            CHECK(pl::band_allows(i, j, Ta, Tb, -1));
            CHECK(pl::band_allows(i, j, Ta, Tb, band) == pl::band_allows(j, i, Tb, Ta, band));   // symmetric
          }
  CHECK((i128)pl::MAX_BAND * T < ((i128)1 << 62));
  // the back-pointer index at the caps
  for (int64_t Ta : {(int64_t)1, T - 1, T})
    for (int64_t Tb : {(int64_t)1, T - 1, T}) {
      const int64_t S = Ta < Tb ? Ta : Tb;
      const i128 words = (i128)(Ta + Tb - 1) * ((S + 15) / 16);
      CHECK((i128)pl::bp_words(Ta, Tb) == words);
      const int64_t dg = Ta + Tb - 2, s = S - 1;
      CHECK((i128)pl::bp_word(dg, s, S) == (i128)dg * ((S + 15) / 16) + s / 16 && pl::bp_word(dg, s, S) < pl::bp_words(Ta, Tb));
      CHECK(pl::bp_shift(s) == (int)(s % 16) * 2 && pl::bp_shift(s) <= 30);
    }
  // a whole batch at the caps: offsets stay in int64
  CHECK((i128)pl::MAX_B * pl::bp_words(T, T) < ((i128)1 << 62) && (i128)pl::MAX_B * pl::path_cells(T, T) * 8 < ((i128)1 << 62));
  CHECK(pl::cell_i(pl::pack_cell(4095, 4095)) == 4095 && pl::cell_j(pl::pack_cell(4095, 4095)) == 4095 && pl::cell_j(pl::pack_cell(4095, 0)) == 0);
  CHECK(pl::path_cells(T, T) == 2 * T - 1 && pl::search_lds_doubles((int)T, pl::MAX_SEARCH_THREADS) * 8 <= pl::LDS_BYTES && pl::search_lds_doubles(1, 64) == 2 * 64 + 2);
  printf("OK\n");
  return 0;
}

static int checks() {
  CHECK(!pl::side_check(0, 1, 1, 1) && !pl::side_check(1, pl::MAX_B, pl::MAX_T, pl::MAX_D));
  CHECK(pl::side_check(2, 1, 1, 1) && pl::side_check(-1, 1, 1, 1) && pl::side_check(0, 0, 1, 1) && pl::side_check(0, pl::MAX_B + 1, 1, 1));
  CHECK(pl::side_check(0, 1, 0, 1) && pl::side_check(0, 1, pl::MAX_T + 1, 1) && pl::side_check(0, 1, 1, 0) && pl::side_check(0, 1, 1, pl::MAX_D + 1));
  CHECK(pl::side_check(0, (int64_t)1 << 40, 1, 1) && pl::side_check(0, 1, (int64_t)1 << 40, 1));
  CHECK(!pl::len_check(1, 1) && !pl::len_check(7, 7) && pl::len_check(0, 7) && pl::len_check(8, 7) && pl::len_check(-3, 7));
  CHECK(!pl::run_check(0, -1, false) && !pl::run_check(1, 5, false) && !pl::run_check(0, pl::MAX_BAND, false) && !pl::run_check(0, 0, true));
  CHECK(pl::run_check(0, 0, false) && pl::run_check(2, -1, false) && pl::run_check(-1, -1, false) && pl::run_check(0, pl::MAX_BAND + 1, false));
  pl::CepPlan p;
  CHECK(!pl::cep_plan(80, 13, &p) && !pl::cep_plan(1, 1, &p) && pl::cep_plan(0, 1, &p) && pl::cep_plan(80, 0, &p) && pl::cep_plan(80, 65, &p) && pl::cep_plan(1025, 1, &p));
  CHECK(pl::cep_plan(1024, 64, &p));   // 64 rows of 1028 floats alone are 257 KiB
  CHECK(pl::padded_d(1) == 4 && pl::padded_d(4) == 4 && pl::padded_d(13) == 16 && pl::padded_d(64) == 64);
  printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc >= 2 && !strcmp(argv[1], "caps")) return caps();
  if (argc >= 2 && !strcmp(argv[1], "checks")) return checks();
  if (argc >= 4 && !strcmp(argv[1], "lds")) {
    pl::CepPlan p;
    if (const char* m = pl::cep_plan(atoi(argv[2]), atoi(argv[3]), &p)) {
      printf("ERR %s\n", m);
      return 0;
    }
    printf("stride=%d tile=%d cepstra_lds_bytes=%d search_lds_bytes=%d walk_lds_bytes=%d\n", p.stride, p.tile, p.lds_floats * 4, pl::search_lds_doubles(pl::MAX_T, pl::MAX_SEARCH_THREADS) * 8,
           (2 * pl::MAX_T - 1) * 4);
    return 0;
  }
  fprintf(stderr, "usage: compare_plan_test sweep | caps | checks | lds N_MEL N_CEP\n");
  return 1;
}
