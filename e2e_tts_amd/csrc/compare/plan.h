// The HIP-free half of libe2etts_compare.so (include/e2etts_compare.h): the argument checks, the caps, the band predicate, the
// back-pointer word and bit index in int64, the workspace sizes, and the tile and LDS plans of the cepstra and the search kernels.
// compare.hip includes it on both its host and its device side; tests/csrc/compare_plan_test.cc builds it with g++ under
// AddressSanitizer + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define E2ECMP_HD __host__ __device__
#else
#define E2ECMP_HD
#endif

namespace e2ecmp_plan {

constexpr int MAX_B = 4096;
constexpr int MAX_T = 4096;        // frames per utterance: a path cell (i, j) packs into 2 x 12 bits, a row of D is 32 KiB of doubles
constexpr int MAX_D = 64;
constexpr int MAX_MEL = 1024;
constexpr int LDS_BYTES = 65536;   // what one workgroup may take
constexpr int THREADS = 256;       // of the cepstra kernel
constexpr int BP_CELLS = 16;       // 2-bit back-pointers per 32-bit word
constexpr int MODE_DTW = 0, MODE_SYNC = 1;

E2ECMP_HD inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }   // a >= 0, b > 0
E2ECMP_HD constexpr int round_up(int a, int m) { return (a + m - 1) / m * m; }
E2ECMP_HD inline int padded_d(int D) { return round_up(D, 4); }   // a feature row in memory: 16-byte words, zeros behind D

// ---- the band: cell (i, j) of a Ta x Tb pair is allowed iff |i * Tb - j * Ta| <= band * max(Ta, Tb); band < 0: every cell is.
// i < Ta, j < Tb <= MAX_T and band <= MAX_BAND keep every product below 2^63.
constexpr int64_t MAX_BAND = (int64_t)1 << 40;
E2ECMP_HD inline bool band_allows(int64_t i, int64_t j, int64_t Ta, int64_t Tb, int64_t band) {
  if (band < 0) return true;
  const int64_t dev = i * Tb - j * Ta;
  return (dev < 0 ? -dev : dev) <= band * (Ta > Tb ? Ta : Tb);
}

// ---- the search: the shorter sequence (S frames) lies on the threads, in chunks of NT rows; the longer one (L frames) is swept.
// NT, the workgroup's size, is a multiple of 64 that covers the batch's longest shorter sequence when the register budget allows:
// a thread holds its own feature row and two rows of the other side, so 1024 threads serve D <= 16, 512 serve D <= 32 and 256 the rest.
// No result depends on NT.
// B is on the threads iff Tb < Ta.  The cells of anti-diagonal dg = i + j lie side by side: cell (i, j) with thread row s (= j when
// swapped, else i) is 2 bits at bit bp_shift(s) of word bp_word(i + j, s, S) of the pair's words.
E2ECMP_HD inline bool swapped(int64_t Ta, int64_t Tb) { return Tb < Ta; }
E2ECMP_HD inline int64_t bp_row_words(int64_t S) { return ceil_div(S, BP_CELLS); }
E2ECMP_HD inline int64_t bp_words(int64_t Ta, int64_t Tb) { return (Ta + Tb - 1) * bp_row_words(Ta < Tb ? Ta : Tb); }
E2ECMP_HD inline int64_t bp_word(int64_t dg, int64_t s, int64_t S) { return dg * bp_row_words(S) + s / BP_CELLS; }
E2ECMP_HD inline int bp_shift(int64_t s) { return (int)(s % BP_CELLS) * 2; }
E2ECMP_HD inline int64_t path_cells(int64_t Ta, int64_t Tb) { return Ta + Tb - 1; }   // a path has at most this many cells
E2ECMP_HD inline uint32_t pack_cell(int i, int j) { return ((uint32_t)i << 12) | (uint32_t)j; }   // i, j < MAX_T = 2^12
E2ECMP_HD inline int cell_i(uint32_t c) { return (int)(c >> 12); }
E2ECMP_HD inline int cell_j(uint32_t c) { return (int)(c & 4095u); }

constexpr int MAX_SEARCH_THREADS = 1024;
E2ECMP_HD constexpr int search_threads_cap(int D4) { return D4 <= 16 ? MAX_SEARCH_THREADS : D4 <= 32 ? MAX_SEARCH_THREADS / 2 : MAX_SEARCH_THREADS / 4; }
E2ECMP_HD inline int search_threads(int D4, int S_max) {
  const int want = round_up(S_max < 1 ? 1 : S_max, 64), cap = search_threads_cap(D4);
  return want < cap ? want : cap;
}
// the search kernel's LDS, in doubles: two rows of NT values the neighbours exchange, then the row of D a chunk hands to the next
// (L values, rounded up to 2)
E2ECMP_HD inline int search_lds_doubles(int L, int NT) { return 2 * NT + round_up(L, 2); }
static_assert((2 * MAX_SEARCH_THREADS + MAX_T) * 8 <= LDS_BYTES, "the search kernel's LDS plan");
static_assert(MAX_T <= 4096 && (2 * MAX_T - 1) * 4 <= LDS_BYTES, "the walk kernel keeps a path of packed cells in LDS");

// ---- the cepstra kernel: a workgroup holds the basis [n_cep rows] and a tile of frames [tile rows] in LDS, every row `stride` floats:
// n_mel rounded up to 4 plus one 16-byte word, and one more when that makes an even number of words (rows a word apart in the banks)
struct CepPlan {
  int stride = 0, tile = 0, lds_floats = 0;
};
E2ECMP_HD inline int cep_stride(int n_mel) {
  int s = round_up(n_mel, 4) + 4;
  if ((s / 4) % 2 == 0) s += 4;
  return s;
}
inline const char* cep_plan(int64_t n_mel, int64_t n_cep, CepPlan* p) {
  if (n_mel < 1 || n_mel > MAX_MEL) return "n_mel must lie in [1, 1024]";
  if (n_cep < 1 || n_cep > MAX_D) return "n_cep must lie in [1, 64]";
  CepPlan q;
  q.stride = cep_stride((int)n_mel);
  for (int tile = 64; tile >= 4; tile /= 2)
    if (((int64_t)n_cep + tile) * q.stride * 4 <= LDS_BYTES) {
      q.tile = tile;
      break;
    }
  if (!q.tile) return "the basis and four frames do not fit the cepstra kernel's LDS plan (64 KiB): fewer mel bins or fewer cepstra";
  q.lds_floats = ((int)n_cep + q.tile) * q.stride;
  *p = q;
  return nullptr;
}

// ---- the argument checks: NULL, or the message
inline const char* side_check(int64_t side, int64_t B, int64_t T, int64_t D) {
  if (side != 0 && side != 1) return "side must be E2ECMP_A or E2ECMP_B";
  if (B < 1 || B > MAX_B) return "B must lie in [1, 4096]";
  if (T < 1 || T > MAX_T) return "T must lie in [1, 4096]";
  if (D < 1 || D > MAX_D) return "D must lie in [1, 64]";
  return nullptr;
}
inline const char* len_check(int64_t len, int64_t T) { return (len < 1 || len > T) ? "every length must lie in [1, T]" : nullptr; }
inline const char* run_check(int64_t mode, int64_t band, bool zero_band_ok) {
  if (mode != MODE_DTW && mode != MODE_SYNC) return "mode must be E2ECMP_DTW or E2ECMP_SYNC";
  if (band == 0 && !zero_band_ok) return "band must be at least 1, or negative for no band";
  if (band > MAX_BAND) return "band must not exceed 2^40";
  return nullptr;
}

}  // namespace e2ecmp_plan
