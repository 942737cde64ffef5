// The HIP-free half of libe2etts_critic.so (include/e2etts_critic.h): the argument checks, the per-layer length formulas, the stride
// fold of the dense layers, the rows every layer's launch covers, the workspace sizes with the cap above which a batch is processed in
// groups of pairs, the grouped kernel's shape support and tile choice, and the index order of the reductions.  critic.hip includes it on
// both its host and its device side; tests/csrc/critic_plan_test.cc builds it with g++ under AddressSanitizer + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define E2ECR_HD __host__ __device__
#else
#define E2ECR_HD
#endif

namespace e2ecr_plan {

constexpr int MAX_B = 4096;
constexpr int MAX_LEN = 1 << 24;
constexpr int MAX_PERIODS = 8, MAX_SCALES = 4, MAX_LAYERS = 8, MAX_DISC = MAX_PERIODS + MAX_SCALES, MAX_MAPS = MAX_LAYERS + 1;
constexpr int MAX_PERIOD = 64, MAX_K = 64, MAX_STRIDE = 8, MAX_CH = 4096;
constexpr int LDS_BYTES = 65536;   // what one workgroup of the grouped kernel may take
constexpr int RED_THREADS = 256, RED_PER_LANE = 16, RED_CHUNK = RED_THREADS * RED_PER_LANE;   // the reduction's chunk: see the header
constexpr int64_t DEFAULT_CAP = (int64_t)2 << 30;
constexpr int POOL_K = 4, POOL_S = 2, POOL_PAD = 2;

enum Kind { FIRST = 0, DENSE = 1, GROUPED = 2, POST = 3 };

E2ECR_HD inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }   // a >= 0, b > 0
E2ECR_HD inline int64_t round_up(int64_t a, int64_t m) { return ceil_div(a, m) * m; }

// floor((n + 2 pad - k) / stride) + 1, 0 when the padded row is shorter than the kernel
E2ECR_HD inline int64_t out_len(int64_t n, int k, int stride, int pad) {
  const int64_t v = n + 2 * (int64_t)pad - k;
  return v < 0 ? 0 : v / stride + 1;
}
E2ECR_HD inline int64_t pool_len(int64_t n) { return out_len(n, POOL_K, POOL_S, POOL_PAD); }   // n / 2 + 1
// the period fold: rows of the folded signal, and the sample the extended signal holds at index i < H * p (i >= n: reflected)
E2ECR_HD inline int64_t period_rows(int64_t n, int p) { return ceil_div(n, p); }
E2ECR_HD inline int64_t reflect_index(int64_t i, int64_t n) { return i < n ? i : 2 * (n - 1) - i; }

// ---- the stride fold of a dense layer (k, s, pad) into a stride-1 layer on the input viewed as [T / s, s * Cin]:
// q = ceil(pad / s) rows of padding, o = s q - pad, K' = ceil((o + k) / s) taps; folded tap j', phase f holds tap s j' + f - o where it exists
struct Fold {
  int q = 0, o = 0, kf = 1;
};
E2ECR_HD inline Fold fold_of(int k, int s, int pad) {
  Fold f;
  f.q = (int)ceil_div(pad, s);
  f.o = s * f.q - pad;
  f.kf = (int)ceil_div(f.o + k, s);
  return f;
}
E2ECR_HD inline int fold_tap(const Fold& f, int s, int jf, int phase) { return s * jf + phase - f.o; }   // valid iff in [0, k)

// ---- the K split of a dense layer.  conv_gemm adds one chain of K = K' * s * Cin fused multiply-adds per element, whose rounding error
// grows like K; the folded channel axis is therefore cut into n equal ranges (whole 32-channel chunks each, chains of at least 128 terms),
// every range is one conv_gemm launch into a partial buffer of its own, and the partials are merged by the fixed tree
// ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)) before the bias: about 1 / sqrt(n) of the unsplit error.
constexpr int MAX_SPLITS = 8;
E2ECR_HD inline int dense_splits(int cin_f, int kf) {
  int n = MAX_SPLITS;
  while (n > 1 && (cin_f % (32 * n) != 0 || (int64_t)cin_f * kf / n < 128)) n /= 2;
  return n;
}

// ---- the grouped kernel: a workgroup takes TM output positions of one group of one sequence; its input window, (TM - 1) s + k rows of
// cin_g channels, lies in LDS channel-major and de-interleaved by phase, [c][r % s][r / s], every phase row `prow` floats (odd).  A
// wavefront computes units of 64 positions x 32 output channels; cout_g = 16 runs as one 32-column tile whose upper half is zero weights.
struct GroupPlan {
  int cin_g = 0, cout_g = 0, ntp = 0, tm = 0, prow = 0, cstride = 0, lds_floats = 0, waves = 0;
};
E2ECR_HD inline int group_prow(int tm, int k, int s) { return (tm + (k - 1) / s) | 1; }
E2ECR_HD inline int64_t group_lds_floats(int cin_g, int tm, int k, int s) { return (int64_t)cin_g * s * group_prow(tm, k, s); }
inline const char* group_plan(int cin, int cout, int k, int s, int groups, int tm_forced, GroupPlan* out) {
  if (groups < 1 || cin % groups || cout % groups) return "groups must divide Cin and Cout";
  GroupPlan g;
  g.cin_g = cin / groups, g.cout_g = cout / groups;
  if (g.cin_g % 8) return "grouped layer: Cin / groups must be a multiple of 8";
  if (g.cout_g % 16) return "grouped layer: Cout / groups must be a multiple of 16";
  g.ntp = (int)ceil_div(g.cout_g, 32);
  int tm = tm_forced > 0 ? tm_forced : 64 * (g.ntp >= 4 ? 1 : 4 / g.ntp);
  if (tm % 64 || tm > 1024) return "grouped layer: the tile must be a multiple of 64, at most 1024";
  while (tm > 64 && tm_forced <= 0 && group_lds_floats(g.cin_g, tm, k, s) * 4 > LDS_BYTES) tm -= 64;
  if (group_lds_floats(g.cin_g, tm, k, s) * 4 > LDS_BYTES) return "grouped layer: the input window of a 64-position tile does not fit 64 KiB of LDS";
  g.tm = tm;
  g.prow = group_prow(tm, k, s);
  g.cstride = s * g.prow;
  g.lds_floats = (int)group_lds_floats(g.cin_g, tm, k, s);
  const int units = tm / 64 * g.ntp;
  g.waves = units < 4 ? units : 4;
  if (out) *out = g;
  return nullptr;
}
// where row r of the window, channel c lies in LDS
E2ECR_HD inline int group_lds_index(const GroupPlan& g, int s, int r, int c) { return c * g.cstride + (r % s) * g.prow + r / s; }
// fragment-order weights of a grouped layer: [group][32-column tile][tap][channel pair][lane 0..63], lane l holds
// w[group * cout_g + tile * 32 + l % 32][2 * pair + l / 32][tap] (0 where the column is >= cout_g)
E2ECR_HD inline int64_t group_frag_floats(int cin, int cout, int k, int groups) {
  return (int64_t)groups * ceil_div(cout / groups, 32) * k * (cin / groups / 2) * 64;
}

// ---- one layer and one discriminator as the library runs them
struct Layer {
  int cin = 0, cout = 0, k = 0, stride = 1, groups = 1, pad = 0;
  int kind = FIRST;
  Fold fold;
  int splits = 1;   // dense: dense_splits
  GroupPlan gp;
};
struct LayerSpec {
  int cout, k, stride, groups, pad;
};

// nullptr or what is wrong with layer i of a table (cin: its input channels; post: the Cout = 1 layer)
inline const char* layer_plan(const LayerSpec& s, int cin, bool first, bool post, Layer* out) {
  if (s.cout < 1 || s.cout > MAX_CH || s.k < 1 || s.k > MAX_K || s.stride < 1 || s.stride > MAX_STRIDE || s.groups < 1 || s.pad < 0 || s.pad >= s.k)
    return "layer: cout in [1, 4096], k in [1, 64], stride in [1, 8], groups >= 1, 0 <= pad < k";
  Layer L;
  L.cin = cin, L.cout = s.cout, L.k = s.k, L.stride = s.stride, L.groups = s.groups, L.pad = s.pad;
  if (post) {
    if (s.cout != 1 || s.stride != 1 || s.groups != 1) return "post layer: cout, stride and groups must be 1";
    if (first) return "a discriminator needs at least one layer before its post layer";
    L.kind = POST;
  } else if (first) {
    if (s.groups != 1) return "first layer: groups must be 1 (Cin is 1)";
    if (s.cout % 4) return "first layer: Cout must be a multiple of 4";
    L.kind = FIRST;
  } else if (s.groups == 1) {
    if (cin % 4 || s.cout % 4) return "dense layer: Cin and Cout must be multiples of 4";
    L.kind = DENSE;
    L.fold = fold_of(s.k, s.stride, s.pad);
    if (L.fold.q > L.fold.kf - 1) return "dense layer: the folded padding exceeds the folded kernel";
    L.splits = dense_splits(s.stride * cin, L.fold.kf);
  } else {
    L.kind = GROUPED;
    if (const char* m = group_plan(cin, s.cout, s.k, s.stride, s.groups, 0, &L.gp)) return m;
  }
  if (out) *out = L;
  return nullptr;
}

struct Disc {
  int period = 0;   // 0: a scale discriminator
  int scale = 0;    // pool applications before it
  int n_layers = 0; // before the post layer; layer[n_layers] is the post layer
  Layer layer[MAX_MAPS];
};

// the lengths a row of n samples has at the input of discriminator d (len[0]) and after each of its layers (len[1 + l])
inline void disc_lens(const Disc& d, int64_t n, int64_t* len /* [n_layers + 2] */) {
  int64_t v = n;
  if (d.period) v = period_rows(n, d.period);
  for (int i = 0; i < d.scale; ++i) v = pool_len(v);
  len[0] = v;
  for (int l = 0; l <= d.n_layers; ++l) {
    const Layer& L = d.layer[l];
    v = out_len(v, L.k, L.stride, L.pad);
    len[1 + l] = v;
  }
}
inline int disc_cols(const Disc& d) { return d.period ? d.period : 1; }

// The rows layer l's launch covers (its output buffer holds that many rows per sequence, zeros past a sequence's length), from the longest
// row's lengths `len` (disc_lens): at least the longest output; a dense layer's launch also covers its folded input, ceil(len_in / s) rows,
// and the layer before a dense layer writes s rows for every row of that launch.  rows[l] >= stride[l + 1] * rows[l + 1] for a dense l + 1.
inline void launch_rows(const Disc& d, const int64_t* len, int64_t* rows /* [n_layers + 1] */) {
  int64_t need = 0;
  for (int l = d.n_layers; l >= 0; --l) {
    const Layer& L = d.layer[l];
    int64_t r = len[1 + l] > need ? len[1 + l] : need;
    if (r < 1) r = 1;
    if (L.kind == DENSE) {
      const int64_t fin = ceil_div(len[l], L.stride);
      if (fin > r) r = fin;
      need = r * L.stride;
    } else {
      need = 0;
    }
    rows[l] = r;
  }
}

// floats of one of the two alternating buffers per ROW of the batch, for a longest row of n samples
inline int64_t disc_buffer_floats(const Disc& d, int64_t n) {
  int64_t len[MAX_MAPS + 1], rows[MAX_MAPS];
  disc_lens(d, n, len);
  launch_rows(d, len, rows);
  int64_t m = 0;
  for (int l = 0; l <= d.n_layers; ++l) {
    const int64_t f = rows[l] * d.layer[l].cout * disc_cols(d);
    if (f > m) m = f;
  }
  return m;
}

// floats of the partial-sum buffer per ROW of the batch: the largest split dense layer's output, once per split
inline int64_t disc_partial_floats(const Disc& d, int64_t n) {
  int64_t len[MAX_MAPS + 1], rows[MAX_MAPS];
  disc_lens(d, n, len);
  launch_rows(d, len, rows);
  int64_t m = 0;
  for (int l = 0; l <= d.n_layers; ++l) {
    if (d.layer[l].kind != DENSE || d.layer[l].splits < 2) continue;
    const int64_t f = rows[l] * d.layer[l].cout * disc_cols(d) * d.layer[l].splits;
    if (f > m) m = f;
  }
  return m;
}

// rows of the batch one pass may hold under the cap (both alternating buffers of floats_per_row each and the partial sums), at least
// `unit` (2 for the fused call: a pair is never split)
inline int64_t rows_per_pass(int64_t floats_per_row, int64_t partial_floats_per_row, int64_t cap_bytes, int unit) {
  if (cap_bytes <= 0) cap_bytes = DEFAULT_CAP;
  const int64_t per = 2 * floats_per_row + partial_floats_per_row;
  int64_t r = cap_bytes / (4 * (per > 0 ? per : 1));
  r = r / unit * unit;
  return r < unit ? unit : r;
}

// ---- argument checks (nullptr = fine)
inline const char* batch_check(int B, long long ld, int dtype) {
  if (B < 1 || B > MAX_B) return "B must lie in [1, 4096]";
  if (ld < 1 || ld > MAX_LEN) return "ld must lie in [1, 2^24]";
  if (dtype != 0 && dtype != 1) return "dtype must be E2ECR_F32 or E2ECR_PCM16";
  return nullptr;
}
inline const char* len_check(int64_t n, long long ld, int min_len) {
  if (n < min_len) return "a row is shorter than the smallest accepted length (the largest period + 1)";
  if (n > ld) return "a row is longer than ld";
  return nullptr;
}

// the reduction's order: element e of a mean goes to lane e % RED_THREADS of chunk e / RED_CHUNK
E2ECR_HD inline int64_t red_chunks(int64_t n) { return ceil_div(n > 0 ? n : 1, RED_CHUNK); }

}  // namespace e2ecr_plan
