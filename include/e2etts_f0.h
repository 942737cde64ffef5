/* e2etts_f0.h -- C ABI of the pitch-tracking companion library (libe2etts_f0.so).
 *
 * The f0 track of a recording on the mel front-end's frame grid, and the data loader's pitch targets made from it, on the GPU.  The
 * reference gets its track from parselmouth (src/tools/utils.py: extract_f0, Sound.to_pitch_ac(time_step = hop / sr, voicing_threshold
 * 0.5, pitch_floor 80, pitch_ceiling 750)) and then forces it onto the mel length by truncation and zero padding.  This library is
 * Boersma's autocorrelation method as Praat documents it, restated, and is UNPINNED AGAINST PARSELMOUTH (which is not a dependency and
 * was never run beside it): the definition here is the contract.  Stated deviations: frames lie on the mel grid, so the track has
 * exactly mel_len frames and the reference's truncation / padding (utils.py:57-70) is NOT reproduced; the autocorrelation is the direct
 * sum (Praat evaluates it through an FFT and resamples it with a sinc; here the maxima are interpolated with a parabola).
 *
 * Definition.  Per row with n valid samples at `sr` Hz and hop `hop`; x is fp32 in [-1, 1], or int16 / 32768.
 *   grid     T = floor(n / hop); frame t is centred on sample c = t * hop + hop / 2 (integer division), the centre of mel frame t of
 *            e2emel_forward.  Samples outside [0, n) are 0.  Every row is analysed over its own length: row b equals a B = 1 call on it.
 *            Frames >= T_b are written as 0 and not computed.
 *   window   W = floor(3 sr / floor), plus 1 if that is even; h = (W - 1) / 2; the window is x[c - h .. c + h].  m = the mean of its W
 *            samples; a[i] = (x[i] - m) * w[i], w[i] = 0.5 - 0.5 cos(2 pi (i + 0.5) / W).  w and the window's own normalised
 *            autocorrelation r_w[tau] = sum_i w[i] w[i + tau] / sum_i w[i]^2 (tau = 0 .. tau_max + 1) are built by the caller in float64,
 *            rounded once to fp32 and loaded with the parameters (e2ef0_configure).
 *   acf      r_a[tau] = sum_{i = 0}^{W - 1 - tau} a[i] a[i + tau], tau = 0 .. tau_max + 1; tau_max = floor(sr / floor), tau_min =
 *            ceil(sr / ceiling) >= 2.  r[tau] = r_a[tau] / (r_a[0] * r_w[tau]).  r_a[0] == 0: the frame has no voiced candidate.
 *            fp32 (m is the fp32 rounding of a float64 sum) in a fixed order: one fused multiply-add per term in ascending i within
 *            chunks of 32 terms, the chunk sums added in ascending order.  The result does not depend on the batch, the grid or the tile.
 *   peaks    p_t = max_i |x[i] - m| over the window; g = max_t p_t over the row's frames.
 *   voiced   every tau in [tau_min, tau_max] with r[tau] > r[tau - 1], r[tau] >= r[tau + 1] and r[tau] > 0 is a candidate:
 *            d = 0.5 (r[tau-1] - r[tau+1]) / (r[tau-1] - 2 r[tau] + r[tau+1]); v = min(1, r[tau] - 0.25 (r[tau-1] - r[tau+1]) d);
 *            f = sr / (tau + d); strength s = v - octave_cost * log2(floor * (tau + d) / sr).  The K - 1 strongest are kept (a tie goes
 *            to the smaller tau), stored in descending strength at indices 1 .. K - 1; an empty slot has f = 0 and s = -infinity.
 *   unvoiced candidate index 0, f = 0: s_u = voicing_threshold + max(0, 2 - (p_t / g) / (silence_threshold / (1 + voicing_threshold)))
 *            (in double on the fp32 p_t and g, rounded once).  g == 0: s_u = voicing_threshold + 2, and the row has no voiced candidate.
 *   path     maximise the sum of strengths minus transition costs over the row's frames; c = 0.01 sr / hop; both ends unvoiced: 0; one
 *            end voiced: voiced_unvoiced_cost * c; both voiced: octave_jump_cost * c * |log2 f1 - log2 f2|.  Double arithmetic on the
 *            fp32 candidates: delta[t][j] = max_i (delta[t-1][i] - cost(i, j)) + s[t][j]; ties go to the lower candidate index (among
 *            predecessors and at the end of the path); one back-pointer per cell.  f0[t] is the chosen f (0 = unvoiced).
 *   targets  the data loader's get_f0 (src/tools/dataloader.py:185-196) on the resident track: uv = f0 == 0; y = (f0 - mean) / std, or
 *            log2(f0 + eps); unvoiced frames filled as np.interp does -- slope = (y1 - y0) / (x1 - x0), slope * (x - x0) + y0, constant
 *            beyond the first and the last voiced frame; an all-unvoiced row becomes 0.  In double without contraction, rounded once
 *            to fp32.  Frames >= T_b are 0 in both outputs.
 *
 * Limits.  The analysis kernel keeps, per workgroup, four frames' windows (each W + tau_max + 2 floats, padded), four rows of lags and
 * the samples of a tile of at least four frames in 64 KiB of LDS; e2ef0_configure refuses a geometry that does not fit
 * (csrc/f0/plan.h: geometry).  48 kHz with floor 80 (W = 1801, 602 lags) at hop 512 is served.
 *
 * Conventions (those of e2etts_mel.h)
 *  - plain C; every function returns 0 or a negative E2EF0_E* code, e2ef0_last_error() gives the message;
 *  - data pointers may be host OR device memory; every output pointer may be NULL;
 *  - the handle works on its own non-blocking stream; every computing entry point returns after that stream has drained; work the
 *    caller still has queued on a stream of its own is ordered with e2ef0_order_after;
 *  - every argument, the length array included, is validated BEFORE anything is enqueued: such a call has enqueued nothing and the
 *    handle stays usable;  n_valid is READ DURING VALIDATION, by a blocking copy when it lies in device memory;
 *  - e2ef0_create and e2ef0_configure with bad arguments open no device;
 *  - workspaces grow with the largest call seen and are never shrunk; steady state allocates nothing;
 *  - one handle is used by one thread at a time (calls are serialised by a mutex inside).
 */
#ifndef E2ETTS_F0_H
#define E2ETTS_F0_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2EF0_API __attribute__((visibility("default")))
#else
#define E2EF0_API
#endif

#define E2EF0_ABI_VERSION 1

#define E2EF0_OK 0
#define E2EF0_EINVAL (-1)   /* bad argument / geometry / length */
#define E2EF0_EHIP (-2)     /* HIP runtime error */
#define E2EF0_ESTATE (-3)   /* call order (forward before configure, targets without a resident track) */
#define E2EF0_ENOMEM (-4)

#define E2EF0_MAX_B 4096
#define E2EF0_MAX_K 16      /* candidates per frame, the unvoiced one included */
#define E2EF0_MIN_RATE 1000
#define E2EF0_MAX_RATE 384000

/* e2ef0_forward dtype */
#define E2EF0_F32 0         /* float samples in [-1, 1] */
#define E2EF0_I16 1         /* int16 PCM, divided by 32768 (exact in fp32) */

/* e2ef0_targets mode */
#define E2EF0_LINEAR 0      /* (f0 - mean) / std */
#define E2EF0_LOG 1         /* log2(f0 + eps) */

typedef struct e2ef0_handle e2ef0_handle;

typedef struct e2ef0_params {
  size_t struct_size;          /* sizeof(e2ef0_params) */
  double floor;                /* 80: what the reference passes */
  double ceiling;              /* 750 */
  double voicing_threshold;    /* 0.5 */
  double silence_threshold;    /* 0.03: Praat's defaults from here on */
  double octave_cost;          /* 0.01 */
  double octave_jump_cost;     /* 0.35 */
  double voiced_unvoiced_cost; /* 0.14 */
  int max_candidates;          /* K = 15, 2 <= K <= E2EF0_MAX_K */
} e2ef0_params;

E2EF0_API const char* e2ef0_version(void);
E2EF0_API int e2ef0_abi_version(void);
/* Last error message of this handle (or of a failed e2ef0_create when handle == NULL). */
E2EF0_API const char* e2ef0_last_error(const e2ef0_handle* handle);

/* sample_rate in [E2EF0_MIN_RATE, E2EF0_MAX_RATE], hop >= 1: the mel front-end's. */
E2EF0_API int e2ef0_create(int device_id, int sample_rate, int hop, e2ef0_handle** out);
E2EF0_API void e2ef0_destroy(e2ef0_handle* handle);

/* The parameters and the two tables: w [W] and r_w [tau_max + 2] fp32 HOST arrays for this geometry (see the definition; W =
 * e2ef0_window(), tau_max + 2 = e2ef0_lags()).  The tables are validated (finite, w in [0, 1], r_w[0] == 1, 0 < r_w <= 1), uploaded to
 * staging buffers and swapped in only when everything succeeded: a failed call leaves the configuration held before in place.
 * Forgets a resident track. */
E2EF0_API int e2ef0_configure(e2ef0_handle* handle, const e2ef0_params* params, const float* w, const float* r_w);
/* W, tau_max + 2 and tau_min of (sample_rate, floor, ceiling): what the tables of e2ef0_configure are sized with.  Negative (E2EF0_EINVAL) for
 * a geometry e2ef0_configure would refuse. */
E2EF0_API int e2ef0_window(int sample_rate, int hop, double floor, double ceiling);
E2EF0_API int e2ef0_lags(int sample_rate, int hop, double floor, double ceiling);
E2EF0_API int e2ef0_tau_min(int sample_rate, int hop, double floor, double ceiling);
/* Frames one workgroup of the analysis kernel takes for the configured geometry (0 before e2ef0_configure). */
E2EF0_API int e2ef0_tile_frames(const e2ef0_handle* handle);

E2EF0_API void* e2ef0_stream(e2ef0_handle* handle);   /* the handle's hipStream_t (opens the device) */
E2EF0_API int e2ef0_order_after(e2ef0_handle* handle, void* caller_stream);
E2EF0_API int e2ef0_sync(e2ef0_handle* handle);
E2EF0_API size_t e2ef0_device_bytes(const e2ef0_handle* handle);

/* The f0 track of a batch of recordings.
 *   audio      B rows of n samples, row b at audio + b * audio_stride ELEMENTS (audio_stride >= n); dtype E2EF0_F32 or E2EF0_I16.
 *   n_valid    [B] int64 samples of each row, each in [0, n], or NULL (every row has n).  At least one row needs a frame (n_valid >= hop).
 *   T_out      receives T = max_b floor(n_valid[b] / hop), the frame count the outputs are laid out with.
 *   f0_out     [B, T] fp32 Hz, 0 = unvoiced; frames >= lens[b] are 0.
 *   lens_out   [B] int64 = floor(n_valid[b] / hop): the mel_lens of e2emel_forward.
 * The track stays RESIDENT in the handle (e2ef0_f0_dev) until the next forward. */
E2EF0_API int e2ef0_forward(e2ef0_handle* handle, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n,
                            float* f0_out, int64_t* lens_out, int* T_out);

/* The data loader's targets from the resident track: f0_t_out and uv_out [B, T] fp32 of the last forward (uv = 1 where f0 == 0; both 0
 * in frames >= lens[b]).  mode E2EF0_LINEAR uses (mean, std), std finite and not 0; E2EF0_LOG uses eps >= 0.  Both stay resident
 * (e2ef0_target_f0_dev, e2ef0_target_uv_dev) until the next forward or targets. */
E2EF0_API int e2ef0_targets(e2ef0_handle* handle, double mean, double std, int mode, double eps, float* f0_t_out, float* uv_out);

/* Device pointers of the resident results, NULL when not resident. */
E2EF0_API const float* e2ef0_f0_dev(e2ef0_handle* handle);
E2EF0_API const float* e2ef0_target_f0_dev(e2ef0_handle* handle);
E2EF0_API const float* e2ef0_target_uv_dev(e2ef0_handle* handle);

/* Measurement aid: with profiling on, forward and targets record HIP events around their phases; e2ef0_profile_read gives the last
 * calls' milliseconds as {analyse, path, targets} (a forward writes the first two, e2ef0_targets the third). */
E2EF0_API int e2ef0_profile_enable(e2ef0_handle* handle, int on);
E2EF0_API int e2ef0_profile_read(e2ef0_handle* handle, double ms_out[3]);

#ifdef E2EF0_TEST_HOOKS
/* Test build only (libe2etts_f0_test.so; the product library does not export these). */
/* Fills every workspace of the handle (the resident results included, the tables not) with NaN bit patterns; nothing is resident afterwards. */
E2EF0_API int e2ef0_debug_poison_workspace(e2ef0_handle* handle);
/* The analysis kernel with r written out: arguments as e2ef0_forward; r_out [B, T, tau_max + 2] fp32 (rows of frames >= lens[b] are 0; a
 * frame with r_a[0] == 0 has r = 0 throughout). */
E2EF0_API int e2ef0_debug_acf(e2ef0_handle* handle, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n,
                              float* r_out, int* T_out);
/* The analysis and the row-peak kernels: freq_out, strength_out [B, T, K] fp32 as the path search reads them (index 0 the unvoiced
 * candidate; empty slots f = 0, s = -infinity; frames >= lens[b] all 0). */
E2EF0_API int e2ef0_debug_candidates(e2ef0_handle* handle, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n,
                                     float* freq_out, float* strength_out, int* T_out);
/* The path kernel alone on the caller's candidates: freq, strength [B, T, K] fp32 (host or device; a slot with strength == -infinity is
 * empty, index 0 must not be), frames [B] int32 in [0, T], f0_out [B, T].  The track stays resident as a forward's does, with `frames` as
 * the rows' lengths: e2ef0_targets can be run on it. */
E2EF0_API int e2ef0_debug_path(e2ef0_handle* handle, const float* freq, const float* strength, const int32_t* frames, int B, int T, float* f0_out);
#endif

#ifdef __cplusplus
}
#endif
#endif
