// The HIP-free half of libe2etts_resample.so (include/e2etts_resample.h): the argument checks, the index formulas of a conversion by L / M,
// the phase-major coefficient table, the bookkeeping of a stream and the tile choice.  resample.hip includes it on both its host and its
// device side; tests/csrc/resample_plan_test.cc builds it with g++ under AddressSanitizer + UBSan.  Everything is int64: the centre
// c(m) = m * M + half of an output passes 2^31 after about five minutes of audio.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define E2ERS_HD __host__ __device__
#else
#define E2ERS_HD
#endif

namespace e2ers_plan {

constexpr int MAX_RATIO = 1024;              // 1 <= L, M <= MAX_RATIO
constexpr int MAX_PHASE_TAPS = 1024;         // P = ceil(n_taps / L), the taps one output sample sums
constexpr int MAX_B = 4096;
constexpr int64_t MAX_N = (int64_t)1 << 40;  // samples per row (of a call, or of a stream in total): n * L and m * M stay far below 2^63
constexpr int THREADS = 256;
constexpr int LDS_FLOATS = 16384;            // 64 KiB: what a kernel gets without opting in; two workgroups fit a CU
constexpr int TILE_MIN_OUTPUTS = 2048;       // small L: a tile is repeated until it holds at least this many outputs (if the LDS allows)

E2ERS_HD inline int64_t floor_div(int64_t a, int64_t b) {   // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
E2ERS_HD inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }   // b > 0

inline int64_t gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// e2ers_load's checks on (n_taps, L, M) -- the taps' finiteness is checked where they are read.  NULL, or the message.
inline const char* filter_check(int64_t n_taps, int64_t L, int64_t M) {
  if (L < 1 || L > MAX_RATIO || M < 1 || M > MAX_RATIO) return "L and M must lie in [1, 1024]";
  if (gcd(L, M) != 1) return "L and M must be coprime (reduce the ratio)";
  if (n_taps < 1 || n_taps % 2 == 0) return "n_taps must be odd (the filter is centred on tap (n_taps - 1) / 2)";
  if (ceil_div(n_taps, L) > MAX_PHASE_TAPS) return "too many taps: ceil(n_taps / L) must not exceed 1024";
  return nullptr;
}

struct Filter {
  int L = 0, M = 0, half = 0, P = 0;   // half = (n_taps - 1) / 2, P = ceil(n_taps / L)
};

inline Filter make_filter(int64_t n_taps, int64_t L, int64_t M) {   // after filter_check
  Filter f;
  f.L = (int)L;
  f.M = (int)M;
  f.half = (int)((n_taps - 1) / 2);
  f.P = (int)ceil_div(n_taps, L);
  return f;
}

// ---- one conversion: y[m] = sum_k x[k] h[c(m) - k L], c(m) = m M + half
E2ERS_HD inline int64_t n_out(int64_t n, int64_t L, int64_t M) { return ceil_div(n * L, M); }
E2ERS_HD inline int64_t centre(int64_t m, const Filter& f) { return m * f.M + f.half; }
E2ERS_HD inline int64_t phase(int64_t m, const Filter& f) { return centre(m, f) % f.L; }       // r: row of the table
E2ERS_HD inline int64_t k_hi(int64_t m, const Filter& f) { return centre(m, f) / f.L; }        // last input with a tap index >= 0
E2ERS_HD inline int64_t k_lo(int64_t m, const Filter& f) { return ceil_div(centre(m, f) - 2 * (int64_t)f.half, f.L); }   // first with one <= 2 half

// The table G[r][i] = h[r + i L] (0 past the last tap), r < L, i < P: output m reads x[k_hi(m) - i] * G[phase(m)][i].
inline int64_t table_floats(const Filter& f) { return (int64_t)f.L * f.P; }
inline int64_t table_tap(int64_t r, int64_t i, const Filter& f) {   // index into h, or -1: the entry is a zero
  const int64_t j = r + i * f.L;
  return j <= 2 * (int64_t)f.half ? j : -1;
}
inline void build_table(const float* taps, const Filter& f, float* G) {
  for (int64_t r = 0; r < f.L; ++r)
    for (int64_t i = 0; i < f.P; ++i) {
      const int64_t j = table_tap(r, i, f);
      G[r * f.P + i] = j < 0 ? 0.f : taps[j];
    }
}

// ---- a stream: after N samples in total the outputs m < emitted(N) exist; the history kept starts at history_start(emitted)
inline int64_t emitted(int64_t N, int last, const Filter& f) {
  if (last) return n_out(N, f.L, f.M);
  const int64_t e = floor_div(N * f.L - 1 - f.half, f.M) + 1;   // k_hi(m) <= N - 1
  return e < 0 ? 0 : e;
}
inline int64_t history_start(int64_t E, const Filter& f) {   // = max(0, k_lo(E)): the first sample output E will read
  const int64_t k = ceil_div(E * f.M - f.half, f.L);
  return k < 0 ? 0 : k;
}
// what a stream that holds N samples keeps: [history_keep, N).  (A very short filter can put history_start past N: nothing is kept then.)
inline int64_t history_keep(int64_t E, int64_t N, const Filter& f) {
  const int64_t k = history_start(E, f);
  return k < N ? k : N;
}

// ---- the tile of one workgroup
// A tile is S * L * nrep consecutive outputs.  They are taken in groups of S lanes that share a phase: group q (q < L * nrep) has
// p = q mod L, rep = q div L, and its lane s computes the output at offset p + L * (S * rep + s) of the tile.  Outputs L apart share the
// row of G and read inputs exactly M apart.  The tile's input window, S * nrep * M + P samples, lies in LDS.
// LDS image: sample t of the window sits at pad(t) = t + (t >> shift), shift = the number of trailing zero bits of M (M odd: pad(t) = t).
// Lanes of a group read addresses l * M apart; l * M is a multiple of 2^shift, so pad() turns that into l * (M + (M >> shift)), an odd
// stride: the 32 lanes that one ds_read_b32 group serves fall into 32 different banks for every M.
struct Tile {
  int S = 0, nrep = 0, shift = 0;
  int window = 0, lds_floats = 0;
  int64_t outputs = 0;
};

E2ERS_HD inline int pad_index(int t, int shift) { return shift ? t + (t >> shift) : t; }

inline int tile_window(int S, int nrep, const Filter& f) { return S * nrep * f.M + f.P; }

inline Tile choose_tile(const Filter& f) {
  Tile t;
  for (int m = f.M; !(m & 1); m >>= 1) ++t.shift;
  const auto lds = [&](int S, int nrep) { return pad_index(tile_window(S, nrep, f) - 1, t.shift) + 1; };
  t.S = 64;
  while (t.S > 1 && lds(t.S, 1) > LDS_FLOATS) t.S >>= 1;   // S = 1 always fits: (M + P) * 1.5 <= 3072
  t.nrep = (int)ceil_div(TILE_MIN_OUTPUTS, (int64_t)t.S * f.L);
  while (t.nrep > 1 && lds(t.S, t.nrep) > LDS_FLOATS) --t.nrep;
  t.window = tile_window(t.S, t.nrep, f);
  t.lds_floats = lds(t.S, t.nrep);
  t.outputs = (int64_t)t.S * f.L * t.nrep;
  return t;
}

// offset inside the tile of the output that item o (o < tile.outputs, item = group * S + lane) computes
E2ERS_HD inline int64_t tile_offset(int64_t o, int S, int L) {
  const int64_t q = o / S, s = o % S;
  return q % L + (int64_t)L * (S * (q / L) + s);
}
// first sample of the window of the tile that starts at output m0 (may be negative: samples before the row are zeros)
E2ERS_HD inline int64_t window_start(int64_t m0, const Filter& f) { return k_hi(m0, f) - (f.P - 1); }

// ---- e2ers_forward's checks on its scalars (those that need no filter; out_stride is checked against n_out once one is loaded).
// NULL, or the message.
inline const char* forward_check(int dtype, int64_t audio_stride, int64_t B, int64_t n) {
  if (dtype != 0 && dtype != 1) return "dtype must be E2ERS_F32 or E2ERS_I16";
  if (B < 1 || B > MAX_B) return "B must lie in [1, 4096]";
  if (n < 1 || n > MAX_N) return "n must lie in [1, 2^40]";
  if (audio_stride < n) return "audio_stride must be at least n";
  return nullptr;
}

}  // namespace e2ers_plan
