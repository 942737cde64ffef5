// The HIP-free half of libe2etts_stats.so (include/e2etts_stats.h): the argument checks, the caps, the power-of-two image of a row, the
// virtual indices of the two percentiles, the workgroup and elements-per-thread choice, the LDS bytes, the bitonic stage schedule and the
// record sizes.  stats.hip includes it on both its host and its device side; tests/csrc/stats_plan_test.cc builds it with g++ under
// AddressSanitizer + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define E2EST_HD __host__ __device__
#else
#define E2EST_HD
#endif

namespace e2est_plan {

constexpr int MAX_B = 4096;          // rows of one add
constexpr int MAX_ROW = 16384;       // frames of one row: its power-of-two image of 32-bit keys is at most LDS_BYTES
constexpr int LDS_BYTES = 65536;     // what one workgroup may take
constexpr int WAVE = 64;
constexpr int MIN_IMAGE = 64;        // the smallest image: one key per lane of one wavefront
constexpr int MAX_THREADS = 1024;
constexpr int MAX_E = 16;            // keys a thread holds at most
constexpr int KIND_F0 = 0, KIND_ENERGY = 1, KIND_PITCH = 2, KINDS = 3;
constexpr int ROW_BYTES = 72, ACC_BYTES = 56;   // e2est_row; the resident accumulator of one kind (stats.hip: Acc)
static_assert(MAX_ROW * 4 == LDS_BYTES && MAX_THREADS * MAX_E == MAX_ROW, "the cap is the LDS image and the largest workgroup's keys");

// ---- argument checks: NULL when fine, else what is wrong (the caller adds the values)
E2EST_HD inline const char* kind_check(int kind) { return kind >= 0 && kind < KINDS ? nullptr : "kind must be E2EST_F0, E2EST_ENERGY or E2EST_PITCH"; }
E2EST_HD inline const char* shape_check(int64_t B, int64_t T, int64_t row_stride) {
  if (B < 1 || B > MAX_B) return "B must lie in [1, E2EST_MAX_B]";
  if (T < 1 || T > INT32_MAX) return "T must lie in [1, 2^31 - 1]";
  if (row_stride < T || row_stride > INT32_MAX) return "row_stride must lie in [T, 2^31 - 1]";
  return nullptr;
}
// one row's length: a row has a frame, lies inside T, and its image fits the LDS plan (there is no multi-pass select)
E2EST_HD inline const char* len_check(int64_t len, int64_t T) {
  if (len < 1) return "a row must have at least 1 frame";
  if (len > T) return "a row is longer than T";
  if (len > MAX_ROW) return "a row is longer than E2EST_MAX_ROW frames (the LDS plan's cap)";
  return nullptr;
}
// normalize takes any length in [0, T]: nothing is sorted
E2EST_HD inline const char* norm_len_check(int64_t len, int64_t T) { return len >= 0 && len <= T ? nullptr : "a length must lie in [0, T]"; }

// ---- the image: the row's n keys, then +inf up to the next power of two (at least MIN_IMAGE)
E2EST_HD inline int image(int n) {   // 1 <= n <= MAX_ROW
  int P = MIN_IMAGE;
  while (P < n) P <<= 1;
  return P;
}
// keys a thread holds and the workgroup's threads for an image of P keys: E * NT == P, NT a multiple of 64
E2EST_HD inline int elems(int P) { return P <= 64 ? 1 : P <= 128 ? 2 : P <= 1024 ? 4 : P <= 8192 ? 8 : 16; }
E2EST_HD inline int threads(int P) { return P / elems(P); }
E2EST_HD inline int lds_bytes(int P) { return P * 4; }   // the reductions' 16 doubles reuse the image once it is dead (MIN_IMAGE * 4 >= 128)
static_assert(MIN_IMAGE * 4 >= (MAX_THREADS / WAVE) * 8, "the reduction scratch fits the smallest image");

// ---- the percentiles: numpy's "linear" method.  v = (n - 1) * q / 100 is exact in double for q = 25, 75 (a multiple of 1/4), so it is
// integer arithmetic here: lo = floor(v), hi = min(lo + 1, n - 1), gamma = v - lo in {0, .25, .5, .75}, exact in float32.
struct VIndex {
  int lo, hi;
  float gamma;
};
E2EST_HD inline VIndex vindex(int64_t n, int q) {   // n >= 1; q is 25 or 75
  const int64_t num = (n - 1) * (q / 25);           // v = num / 4
  VIndex r;
  r.lo = (int)(num / 4);
  r.hi = r.lo + 1 < n ? r.lo + 1 : (int)(n - 1);
  r.gamma = (float)(num % 4) * 0.25f;
  return r;
}

// ---- the bitonic network over an image of P keys held E to a thread: key r of thread t is element i = r * NT + t.
// Merge sizes k = 2, 4 .. P; inside each the distances j = k / 2 .. 1; element i is compared with i ^ j, the pair ascending iff (i & k) == 0.
// The partner of a stage is, by its distance: another key of the same thread (j >= NT), the same key of another wavefront's thread
// (64 <= j < NT: through LDS, with a barrier), or the same key of lane t ^ j of the same wavefront (j < 64: a shuffle).
constexpr int STAGE_REG = 0, STAGE_LDS = 1, STAGE_SHFL = 2;
E2EST_HD inline int stage_class(int j, int NT) { return j >= NT ? STAGE_REG : j >= WAVE ? STAGE_LDS : STAGE_SHFL; }
E2EST_HD inline int partner(int i, int j) { return i ^ j; }
// element i keeps the smaller key of its pair (else the larger)
E2EST_HD inline bool keeps_min(int i, int j, int k) { return ((i & j) == 0) == ((i & k) == 0); }
E2EST_HD inline int stage_count(int P) {   // log2(P) * (log2(P) + 1) / 2
  int l = 0;
  while ((1 << l) < P) ++l;
  return l * (l + 1) / 2;
}

// ---- a float32 as a 32-bit key whose unsigned order is the total order -inf < .. < -0 < +0 < .. < +inf, and back
E2EST_HD inline uint32_t key_of(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
E2EST_HD inline uint32_t bits_of(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }
E2EST_HD inline bool non_finite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }
constexpr uint32_t KEY_PAD = 0xff800000u;       // key_of(+inf): the keys at and above it are +inf and the positive NaNs
constexpr uint32_t KEY_NEG_INF = 0x007fffffu;   // key_of(-inf): the keys at and below it are -inf and the negative NaNs

}  // namespace e2est_plan
