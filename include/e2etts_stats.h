/* e2etts_stats.h -- C ABI of the corpus-statistics companion library (libe2etts_stats.so).
 *
 * What the reference's TextMelLoader.build_stats (src/tools/dataloader.py:106-151) writes into stats.json, from arrays that already lie
 * on the device (the mel front-end's e2emel_energy_dev, the pitch library's e2ef0_f0_dev, a caller's tensor), and the data loader's
 * energy target (get_prosody, dataloader.py:179-183).  THE DEFINITION BELOW IS THE CONTRACT.
 *
 * Definition.
 *   rows      one add takes a ragged batch of B rows of fp32 frame values, row b holding n = lens[b] frames, 1 <= n <= min(T,
 *             E2EST_MAX_ROW).  A row never shares arithmetic with another: every row's record equals the record of a B = 1 call on it,
 *             bit for bit.
 *   scaled    kinds E2EST_ENERGY and E2EST_PITCH, the reference's remove_outlier (src/tools/utils.py:142-150) per row.  s is the row
 *             sorted ascending.  For q = 25 and 75: v = (n - 1) q / 100 (exact: a multiple of 1/4), lo = floor(v), hi = min(lo + 1, n - 1),
 *             g = float32(v - lo); the percentile, as np.percentile computes it on a float32 row, in float32 with every operation
 *             rounded separately (no fused multiply-add):
 *                 g <  0.5:  s[lo] + (s[hi] - s[lo]) * g
 *                 g >= 0.5:  s[hi] - (s[hi] - s[lo]) * (1 - g)
 *             The fences, in float32, each operation rounded: lower = p25 - 1.5 * (p75 - p25), upper = p75 + 1.5 * (p75 - p25).
 *             A value is KEPT iff lower < v < upper, both comparisons strict.  min = s[0], max = s[n - 1].
 *             sum = the sum of double(v) over the kept values, mean = sum / n_kept, m2 = the sum of (double(v) - mean)^2 over them, the
 *             product and the sum rounded separately; mean = m2 = 0 when nothing is kept.  The order of the two sums is fixed by the row's
 *             length alone; any order is within (N - 1) 2^-53 sum|x| of the exact sum.
 *   f0        kind E2EST_F0: the frames with v != 0 are voiced (so -0.0 is unvoiced); n_kept counts them, sum / mean / m2 as above over
 *             them.  No sort; the float fields of the record are 0.
 *   merge     the handle keeps (n, mean, M2) per kind, and for the scaled kinds the running raw min and max over ALL values, outliers
 *             included.  The rows of an add are folded in row order by Chan's pairwise update in double:
 *                 n = na + nb;  d = mean_b - mean_a;  mean = mean_a + d * nb / n;  M2 = M2a + M2b + d * d * na * nb / n
 *             (a row that kept nothing is skipped; the first row that kept something is taken as it is).  The result of a sequence of
 *             rows therefore does not depend on how they were split into add calls.  This is NOT sklearn's bit pattern -- its
 *             partial_fit result depends on the order the loader visited the files in -- it agrees with it within the rounding of a
 *             double sum in any order.
 *   result    mean as kept, std = sqrt(M2 / n) (population), 1 when M2 == 0 for the scaled kinds (sklearn's scale of a constant
 *             feature); min = (double(raw min) - mean) / std and max likewise: subtraction and division by a positive number are
 *             monotone, so this is the reference's second pass over the normalised values, bit for bit for the same mean and std.
 *   normalize out[b, t] = (v - float32(mean)) / float32(std) in float32, the division correctly rounded, for t < lens[b]; 0 beyond.
 *
 * Stated deviations from the reference.
 *  - A row that contains a non-finite value is REFUSED: its record has status 1, no row of that add is merged, and every later
 *    e2est_fetch_rows / e2est_result returns E2EST_EINVAL naming the add and the row until e2est_reset.  (numpy would propagate NaN.)
 *  - A row longer than E2EST_MAX_ROW frames is refused by e2est_add before anything is enqueued, the error naming the row: the sort
 *    works on one LDS image, there is no multi-pass select.
 *  - The f0 track is fp32 here; the reference's np.mean / np.std run in float64 on float64 tracks, so do the sums here.
 *
 * Conventions (those of e2etts_compare.h)
 *  - plain C; every function returns 0 or a negative E2EST_E* code, e2est_last_error() gives the message;
 *  - `values` and `out` are DEVICE memory; lens may be host or device memory and are READ DURING VALIDATION, by a blocking copy when they
 *    lie in device memory;
 *  - the handle works on its own non-blocking stream.  e2est_add and e2est_normalize ENQUEUE and return: they do not wait for the device.
 *    e2est_fetch_rows, e2est_result and e2est_sync drain the stream.  Work the caller still has queued on a stream of its own is ordered
 *    with e2est_order_after;
 *  - every argument is validated BEFORE anything is enqueued: such a call has enqueued nothing and the handle stays usable;
 *  - e2est_create with bad arguments opens no device;
 *  - workspaces grow with the largest call seen and are never shrunk; steady state allocates nothing;
 *  - one handle is used by one thread at a time (calls are serialised by a mutex inside).
 *
 * Exports: 16 entry points, and 2 more in the test build.
 */
#ifndef E2ETTS_STATS_H
#define E2ETTS_STATS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2EST_API __attribute__((visibility("default")))
#else
#define E2EST_API
#endif

#define E2EST_ABI_VERSION 1

#define E2EST_OK 0
#define E2EST_EINVAL (-1)   /* bad argument / shape / length; a refused row */
#define E2EST_EHIP (-2)     /* HIP runtime error */
#define E2EST_ESTATE (-3)   /* call order (fetch_rows before an add), an accumulator without a kept value */
#define E2EST_ENOMEM (-4)

#define E2EST_MAX_B 4096
#define E2EST_MAX_ROW 16384   /* frames per row: the power-of-two image of a row is at most 64 KiB of LDS (190 s at hop 256, 22.05 kHz) */

/* kinds */
#define E2EST_F0 0
#define E2EST_ENERGY 1
#define E2EST_PITCH 2

typedef struct e2est_handle e2est_handle;

/* One row's record, 72 bytes. */
typedef struct e2est_row {
  int64_t n;        /* frames of the row */
  int64_t n_kept;   /* scaled kinds: values inside the fences; E2EST_F0: voiced frames */
  double sum;       /* of the kept values */
  double mean;      /* sum / n_kept, 0 when n_kept == 0 */
  double m2;        /* sum of squared deviations from mean */
  float p25, p75, lower, upper, min, max;   /* scaled kinds; 0 for E2EST_F0 */
  int32_t status;   /* 0 ok, 1 the row holds a non-finite value (the other fields are then unspecified) */
  int32_t reserved;
} e2est_row;

/* One kind's block of stats.json and the accumulator behind it, 88 bytes. */
typedef struct e2est_block {
  int64_t present;    /* 1 when a row of this kind was added since the last reset; the other fields are 0 otherwise */
  int64_t rows;       /* rows added */
  int64_t n_frames;   /* frames added */
  int64_t n_kept;     /* values behind mean and std (scaled: inside the fences; E2EST_F0: voiced) */
  double mean, std;
  double m2;          /* with n_kept and mean: what merges with another accumulator by the formula above */
  double min, max;    /* scaled kinds: of the normalised values, over all frames */
  double raw_min, raw_max;   /* scaled kinds: of the values themselves (exact float32 values) */
} e2est_block;

typedef struct e2est_stats {
  e2est_block kind[3];   /* by E2EST_F0, E2EST_ENERGY, E2EST_PITCH */
} e2est_stats;

E2EST_API const char* e2est_version(void);
E2EST_API int e2est_abi_version(void);
/* Last error message of this handle (or of a failed e2est_create when handle == NULL). */
E2EST_API const char* e2est_last_error(const e2est_handle* handle);

E2EST_API int e2est_create(int device_id, e2est_handle** out);
E2EST_API void e2est_destroy(e2est_handle* handle);

E2EST_API void* e2est_stream(e2est_handle* handle);   /* the handle's hipStream_t (opens the device) */
E2EST_API int e2est_order_after(e2est_handle* handle, void* caller_stream);
E2EST_API int e2est_sync(e2est_handle* handle);
E2EST_API size_t e2est_device_bytes(const e2est_handle* handle);

/* Empties the three accumulators and forgets a refused row. */
E2EST_API int e2est_reset(e2est_handle* handle);
/* Accumulates B rows of one kind: values fp32 on the device, row b at values + b * row_stride (elements; row_stride >= T), lens [B]
 * int64, each in [1, min(T, E2EST_MAX_ROW)].  Nothing beyond a row's length is read. */
E2EST_API int e2est_add(e2est_handle* handle, int kind, const float* values, int64_t row_stride, const int64_t* lens, int B, int T);
/* The records of the last add's rows into out [B] (host or device memory).  E2EST_EINVAL, naming the row, when one was refused (the
 * records are written all the same). */
E2EST_API int e2est_fetch_rows(e2est_handle* handle, e2est_row* out);
/* The three blocks.  A kind with no row added is absent (present = 0).  E2EST_ESTATE, naming the kind, for an E2EST_F0 accumulator
 * without a voiced frame or a scaled one with nothing kept: the reference ends in NaN, or in an unfitted scaler, there. */
E2EST_API int e2est_result(e2est_handle* handle, e2est_stats* out);
/* The data loader's target: out [B, T] fp32 on the device (dense rows) from values as for e2est_add; lens each in [0, T]; std > 0. */
E2EST_API int e2est_normalize(e2est_handle* handle, const float* values, int64_t row_stride, const int64_t* lens, int B, int T, double mean, double std,
                              float* out);

/* Measurement aid: with profiling on, the calls record HIP events around their kernels; after the stream has drained (e2est_sync,
 * e2est_fetch_rows, e2est_result) e2est_profile_read gives the last calls' milliseconds as {rows, merge, normalize}. */
E2EST_API int e2est_profile_enable(e2est_handle* handle, int on);
E2EST_API int e2est_profile_read(e2est_handle* handle, double ms_out[3]);

#ifdef E2EST_TEST_HOOKS
/* Test build only (libe2etts_stats_test.so; the product library does not export these). */
/* Fills every workspace of the handle (the accumulators included) with NaN bit patterns, then resets. */
E2EST_API int e2est_debug_poison_workspace(e2est_handle* handle);
/* The row kernel's sorted rows: out [B, T] fp32 (host or device), row b's first lens[b] values ascending, the rest untouched.  Arguments as for
 * e2est_add with a scaled kind; nothing is accumulated. */
E2EST_API int e2est_debug_sorted(e2est_handle* handle, const float* values, int64_t row_stride, const int64_t* lens, int B, int T, float* out);
#endif

#ifdef __cplusplus
}
#endif
#endif
