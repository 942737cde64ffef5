/* e2etts_compare.h -- C ABI of the comparison companion library (libe2etts_compare.so).
 *
 * How close two recordings are, on the GPU: dynamic time warping over cepstra of the log-mel both already have on the device (the mel
 * front-end's e2emel_mel_dev, the pitch library's e2ef0_f0_dev), and along the path the mel-cepstral distortion, the mel L1, the f0 error
 * and the voiced/unvoiced error.  The reference's only evaluation tool (modules/metrics/mos_test.py) loads a learned metric that is not
 * available; nothing here restates it.  THE DEFINITION BELOW IS THE CONTRACT.  The distortion is computed on DCT cepstra of THIS
 * PROJECT'S log-mel (natural log of a Slaney filterbank's magnitudes): it is NOT comparable with the SPTK / WORLD mel-cepstrum MCD figures
 * of the literature, only with other figures made by this library.
 *
 * Definition.
 *   sides    the handle holds two sides, E2ECMP_A and E2ECMP_B: each a ragged batch of B utterances with lens[b] frames, 1 <= lens[b] <=
 *            min(T, E2ECMP_MAX_T).  A side is set from log-mel [B, T, n_mel] fp32 channels-last (the layout of e2emel_mel_dev) with an
 *            optional f0 track [B, T] in Hz, 0 = unvoiced (the layout of e2ef0_f0_dev), or from ready features [B, T, D] fp32, D <=
 *            E2ECMP_MAX_D (a general DTW).  A side is copied into the handle and stays RESIDENT until it is set again: the recordings
 *            can stay as side A while side B changes.  Pair b is utterance b of A against utterance b of B; every pair is computed
 *            over its own lengths and equals a B = 1 call on it bit for bit.
 *   cepstra  c[t, k] = sum_m basis[k, m] * logmel[t, m], k < n_cep <= 64, basis [n_cep, n_mel] given by the caller (e2ecmp_load; the
 *            Python binding's default is rows 1 .. 13 of the orthonormal DCT-II, so c0 is left out).  One fp32 fused-multiply-add chain
 *            per value over m ascending from 0: the result does not depend on the batch, the grid or the tile.
 *   cost     in double: d(i, j) = sqrt(sum_k (double(a[i, k]) - double(b[j, k]))^2), k ascending, the product and the sum rounded
 *            separately (no fused multiply-add), the square root correctly rounded.  The cost matrix never reaches HBM.
 *   search   D(0, 0) = d(0, 0); D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), in double.  Ties go to the diagonal
 *            first, then to (i-1, j), then to (i, j-1).  Back-pointers take 2 bits per cell.  band >= 1: a Sakoe-Chiba band, cell (i, j)
 *            is allowed iff |i * Tb - j * Ta| <= band * max(Ta, Tb) in int64 (csrc/compare/plan.h: band_allows); band < 0: no band;
 *            band == 0 is refused.  A pair without a path of finite cost inside the band gets status 1 and NaN figures (n_path 0); the
 *            other pairs of the batch are unaffected.  (Every band >= 1 holds a path: the cells nearest the line i / Ta = j / Tb are
 *            connected.  Status 1 is reached by infinite or NaN features.)
 *            mode E2ECMP_SYNC skips the search: the path is (i, i), i < min(Ta, Tb) -- the frame-synchronous comparison of a
 *            teacher-forced output with its recording -- and dist_total is the sum of d along it.
 *   figures  accumulated in double along the path, N cells: see e2ecmp_result.  A frame is voiced iff its f0 > 0.
 *   path     int32 pairs (i, j) in path order, N <= Ta + Tb - 1 of them per pair, resident until the next run (e2ecmp_fetch_path).
 *
 * Conventions (those of e2etts_mel.h)
 *  - plain C; every function returns 0 or a negative E2ECMP_E* code, e2ecmp_last_error() gives the message;
 *  - data pointers may be host OR device memory; the lengths are READ DURING VALIDATION, by a blocking copy when they lie in device memory;
 *  - the handle works on its own non-blocking stream; every computing entry point returns after that stream has drained; work the
 *    caller still has queued on a stream of its own is ordered with e2ecmp_order_after;
 *  - every argument is validated BEFORE anything is enqueued: such a call has enqueued nothing and the handle stays usable;
 *  - e2ecmp_create with bad arguments opens no device;
 *  - workspaces grow with the largest call seen and are never shrunk; steady state allocates nothing;
 *  - one handle is used by one thread at a time (calls are serialised by a mutex inside).
 *
 * Exports: 17 entry points, and 2 more in the test build.
 */
#ifndef E2ETTS_COMPARE_H
#define E2ETTS_COMPARE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2ECMP_API __attribute__((visibility("default")))
#else
#define E2ECMP_API
#endif

#define E2ECMP_ABI_VERSION 1

#define E2ECMP_OK 0
#define E2ECMP_EINVAL (-1)   /* bad argument / shape / length */
#define E2ECMP_EHIP (-2)     /* HIP runtime error */
#define E2ECMP_ESTATE (-3)   /* call order (set_mels before load, run before both sides are set) */
#define E2ECMP_ENOMEM (-4)

#define E2ECMP_MAX_B 4096
#define E2ECMP_MAX_T 4096    /* frames per utterance: one row of D in double stays in LDS */
#define E2ECMP_MAX_D 64      /* features per frame; n_cep <= this */
#define E2ECMP_MAX_MEL 1024  /* e2ecmp_create refuses (n_mel, n_cep) whose basis and a tile of frames do not fit 64 KiB of LDS */

#define E2ECMP_A 0
#define E2ECMP_B 1

/* e2ecmp_run mode */
#define E2ECMP_DTW 0
#define E2ECMP_SYNC 1

typedef struct e2ecmp_handle e2ecmp_handle;

/* One pair's figures: int64 and double only, 72 bytes. */
typedef struct e2ecmp_result {
  int64_t n_path;          /* N, the number of path cells (0 with status 1) */
  int64_t n_voiced_both;   /* path cells voiced on both sides (0 without f0) */
  int64_t n_vuv_mismatch;  /* path cells voiced on exactly one side (0 without f0) */
  int64_t status;          /* 0 ok, 1 no path of finite cost inside the band */
  double dist_total;       /* D at the end cell (E2ECMP_SYNC: the sum of d along the path) */
  double mcd_db;           /* (10 sqrt(2) / ln 10) * the mean of d over the path */
  double mel_l1;           /* mean over path cells and mel bins of |logmel_a - logmel_b|; NaN unless both sides were set from mels */
  double f0_rmse_hz;       /* over the path cells voiced on both sides; NaN when there is none or a side has no f0 */
  double f0_rmse_cents;    /* the same of 1200 log2(f0_b / f0_a) */
} e2ecmp_result;

E2ECMP_API const char* e2ecmp_version(void);
E2ECMP_API int e2ecmp_abi_version(void);
/* Last error message of this handle (or of a failed e2ecmp_create when handle == NULL). */
E2ECMP_API const char* e2ecmp_last_error(const e2ecmp_handle* handle);

/* n_mel in [1, E2ECMP_MAX_MEL], n_cep in [1, E2ECMP_MAX_D]. */
E2ECMP_API int e2ecmp_create(int device_id, int n_mel, int n_cep, e2ecmp_handle** out);
E2ECMP_API void e2ecmp_destroy(e2ecmp_handle* handle);
/* The cepstral basis [n_cep, n_mel], a fp32 HOST array of finite values.  Sides set from mels before stay as they are. */
E2ECMP_API int e2ecmp_load(e2ecmp_handle* handle, const float* basis);

E2ECMP_API void* e2ecmp_stream(e2ecmp_handle* handle);   /* the handle's hipStream_t (opens the device) */
E2ECMP_API int e2ecmp_order_after(e2ecmp_handle* handle, void* caller_stream);
E2ECMP_API int e2ecmp_sync(e2ecmp_handle* handle);
E2ECMP_API size_t e2ecmp_device_bytes(const e2ecmp_handle* handle);

/* Sets a side from log-mel [B, T, n_mel] fp32 and, when f0 is not NULL, its track [B, T] fp32 Hz; lens [B] int64, each in [1, T].
 * The cepstra are computed now. */
E2ECMP_API int e2ecmp_set_mels(e2ecmp_handle* handle, int side, const float* mel, const float* f0, const int64_t* lens, int B, int T);
/* Sets a side from features [B, T, D] fp32, 1 <= D <= E2ECMP_MAX_D: no mel (mel_l1 is NaN) and no f0. */
E2ECMP_API int e2ecmp_set_features(e2ecmp_handle* handle, int side, const float* features, const int64_t* lens, int B, int T, int D);
/* The features the search reads of a side, [B, T, D] fp32 (the cepstra of a side set from mels; rows >= lens[b] are 0). */
E2ECMP_API int e2ecmp_fetch_features(e2ecmp_handle* handle, int side, float* out);

/* Compares the sides pair by pair: both must be set, with the same B and the same D.  results_out [B] (may be NULL). */
E2ECMP_API int e2ecmp_run(e2ecmp_handle* handle, int mode, long long band, e2ecmp_result* results_out);
/* The path of pair b of the last run: n_path (i, j) int32 pairs into out (capacity in pairs; host or device), n_out receives n_path. */
E2ECMP_API int e2ecmp_fetch_path(e2ecmp_handle* handle, int b, int32_t* out, long long capacity, long long* n_out);

/* Measurement aid: with profiling on, the calls record HIP events around their kernels; e2ecmp_profile_read gives the last calls'
 * milliseconds as {cepstra, search, walk} (a set_mels writes the first, a run the other two). */
E2ECMP_API int e2ecmp_profile_enable(e2ecmp_handle* handle, int on);
E2ECMP_API int e2ecmp_profile_read(e2ecmp_handle* handle, double ms_out[3]);

#ifdef E2ECMP_TEST_HOOKS
/* Test build only (libe2etts_compare_test.so; the product library does not export these). */
/* Fills every workspace of the handle (both sides included, the basis not) with NaN bit patterns; no side is set afterwards. */
E2ECMP_API int e2ecmp_debug_poison_workspace(e2ecmp_handle* handle);
/* e2ecmp_run that also takes band == 0 (cells exactly on the line i * Tb == j * Ta): the one band without a path for most pairs. */
E2ECMP_API int e2ecmp_debug_run(e2ecmp_handle* handle, int mode, long long band, e2ecmp_result* results_out);
#endif

#ifdef __cplusplus
}
#endif
#endif
