/* e2etts_condition.h -- C ABI of the recording-conditioning companion library (libe2etts_condition.so).
 *
 * What the reference does to a recording before anything else (modules/metrics/audio_processing.py: normalize_signal): set_channels,
 * remove_silent (pydub detect_silence) and set_loudness, on int16 PCM on the GPU.  (set_frame_rate is libe2etts_resample.so.)  pydub does
 * all of this in integers through the standard library's audioop (rms, mul, tomono); the arithmetic below reproduces audioop bit for
 * bit.  The pydub layer itself -- millisecond positions, window stepping, range merging, the zero padding of a short slice -- is restated
 * from its source and is UNPINNED AGAINST PYDUB: the definition here is the contract.
 *
 * Definition (all integers).  Rows of N int16 frames at `rate` Hz.
 *   pos(p)   = p * rate / 1000 (floor): the sample index of millisecond p
 *   len_ms   = round(1000 * (N / rate)) in double, half to even.  pos(len_ms) may exceed N by up to rate / 2000 samples: samples in
 *              [N, pos(len_ms)) count as zeros.
 *   downmix  mono = floor((l + r) / 2)                                                     (audioop.tomono(.., 0.5, 0.5))
 *   rms      isqrt(S / n), S the sum of squares of n samples                               (audioop.rms)
 *   silence  with W = min_silence_len and k = floor(10 ^ (thresh_dB / 20) * 32768): no ranges when len_ms < W; else window start i in
 *            [0, len_ms - W] is silent iff S(pos(i) .. pos(i + W)) < (k + 1)^2 * (pos(i + W) - pos(i))   (rms <= k).  Walk the silent
 *            starts in order: a start b whose silent predecessor a has b > a + W opens a new range; a range is [first start, last start + W].
 *   span     E2ECOND_TRIM_REFERENCE (remove_silent as the reference has it): s = ranges[0][1] if ranges[0][0] == 0 else 0; e = len_ms
 *            ALWAYS (the reference tests `silent[-1][-1] == 0`, which no range satisfies: it never trims the tail).
 *            E2ECOND_TRIM_BOTH (what its docstring says; a stated deviation): additionally e = ranges[-1][0] when ranges[-1][1] == len_ms.
 *            A row without ranges, and every row under E2ECOND_TRIM_NONE, is kept unsliced: s = 0, e = len_ms, n_out = N.
 *            Otherwise n_out = max(0, pos(e) - pos(s)), the samples from pos(s) on, zeros past N.
 *   gain     out = floor(min(max(v * gain, -32768.0), 32767.0)) in double                  (audioop.mul)
 *            The caller computes gain (set_loudness: 10 ^ ((target - dBFS) / 20), dBFS = 20 * log(rms / 32768, 10), rms over the kept
 *            span, padding included) from the span's sum of squares that e2econd_analyze returns.
 *   fp32     out / 32768 (exact).
 * No float reductions: sums are uint64, so nothing depends on the order of summation.
 *
 * Conventions (those of e2etts_resample.h)
 *  - plain C; every function returns 0 or a negative E2ECOND_E* code, e2econd_last_error() gives the message;
 *  - data pointers may be host OR device memory; every output pointer may be NULL;
 *  - the handle works on its own non-blocking stream; every computing entry point returns after that stream has drained; work the
 *    caller still has queued on a stream of its own is ordered with e2econd_order_after;
 *  - every argument, the length array included, is validated BEFORE anything is enqueued: such a call has enqueued nothing and the
 *    handle stays usable.  The one E2ECOND_EINVAL that is found afterwards is a row with more ranges than `cap` (see e2econd_analyze);
 *  - lens and gain are READ DURING VALIDATION, by a blocking copy when they lie in device memory;
 *  - e2econd_create and e2econd_configure open no device: the GPU is first touched by a computing call;
 *  - workspaces grow with the largest call seen and are never shrunk; steady state allocates nothing;
 *  - one handle is used by one thread at a time (calls are serialised by a mutex inside).
 */
#ifndef E2ETTS_CONDITION_H
#define E2ETTS_CONDITION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2ECOND_API __attribute__((visibility("default")))
#else
#define E2ECOND_API
#endif

#define E2ECOND_ABI_VERSION 1

#define E2ECOND_OK 0
#define E2ECOND_EINVAL (-1)   /* bad argument / length; more ranges than cap */
#define E2ECOND_EHIP (-2)     /* HIP runtime error */
#define E2ECOND_ESTATE (-3)   /* call order (not configured, apply without a completed analyze) */
#define E2ECOND_ENOMEM (-4)

#define E2ECOND_MAX_B 4096
#define E2ECOND_MIN_RATE 1000
#define E2ECOND_MAX_RATE 384000
#define E2ECOND_MAX_W 4096

#define E2ECOND_TRIM_NONE 0
#define E2ECOND_TRIM_REFERENCE 1
#define E2ECOND_TRIM_BOTH 2

#define E2ECOND_WANT_PCM 1
#define E2ECOND_WANT_WAV 2

typedef struct e2econd_handle e2econd_handle;

/* one row's record of e2econd_analyze (32 bytes) */
typedef struct e2econd_row {
  int32_t len_ms;
  int32_t n_ranges;   /* the true count, also when it exceeds cap */
  int32_t s_ms, e_ms; /* the kept span in ms */
  int64_t n_out;      /* its samples */
  uint64_t sumsq;     /* its sum of squares (zero padding included) */
} e2econd_row;

E2ECOND_API const char* e2econd_version(void);
E2ECOND_API int e2econd_abi_version(void);
/* Last error message of this handle (or of a failed e2econd_create when handle == NULL). */
E2ECOND_API const char* e2econd_last_error(const e2econd_handle* handle);

E2ECOND_API int e2econd_create(int device_id, e2econd_handle** out);
E2ECOND_API void e2econd_destroy(e2econd_handle* handle);

/* rate in [E2ECOND_MIN_RATE, E2ECOND_MAX_RATE] Hz, min_silence_len W in [1, E2ECOND_MAX_W] ms, the threshold k in [0, 32767] int16
 * units.  Forgets a completed analysis. */
E2ECOND_API int e2econd_configure(e2econd_handle* handle, int rate, int min_silence_len, int k);

E2ECOND_API void* e2econd_stream(e2econd_handle* handle);   /* the handle's hipStream_t (opens the device) */
E2ECOND_API int e2econd_order_after(e2econd_handle* handle, void* caller_stream);
E2ECOND_API int e2econd_sync(e2econd_handle* handle);
E2ECOND_API size_t e2econd_device_bytes(const e2econd_handle* handle);

/* Stereo to mono.  stereo: B rows of n interleaved (l, r) frames, row b at stereo + b * stride ELEMENTS (stride >= 2 n).  The result
 * [B, n] int16 stays RESIDENT (e2econd_mono_dev, rows n elements apart) until the next downmix and is copied to mono_out (rows out_stride >= n
 * elements apart) when that is given.  Every row is converted over all n frames. */
E2ECOND_API int e2econd_downmix(e2econd_handle* handle, const int16_t* stereo, long long stride, int B, long long n, int16_t* mono_out, long long out_stride);
E2ECOND_API const int16_t* e2econd_mono_dev(e2econd_handle* handle);

/* Silence ranges and the kept span of every row.
 *   pcm       B rows of mono int16, row b at pcm + b * stride elements (stride >= n).  A row in DEVICE memory is read again by
 *             e2econd_apply and must stay valid until then; host rows are staged in the handle.
 *   lens      [B] int64 frames of each row, each in [0, n], or NULL (every row has n).
 *   trim      E2ECOND_TRIM_*.
 *   cap       ranges per row that ranges_out holds.
 *   rows_out  [B] records (host or device memory).
 *   ranges_out [B][cap][2] int32 (start, end) in ms, zeros past a row's count.
 * When a row has more ranges than cap, rows_out and ranges_out are still written -- n_ranges is the true count, the first cap ranges are
 * listed -- and the call returns E2ECOND_EINVAL; e2econd_apply then has nothing to work on. */
E2ECOND_API int e2econd_analyze(e2econd_handle* handle, const int16_t* pcm, long long stride, const int64_t* lens, int B, long long n, int trim, int cap,
                                e2econd_row* rows_out, int32_t* ranges_out);

/* Gather, gain and store of the last analysis: row b becomes its kept span times gain[b] ([B] double, finite, not negative).
 *   want      E2ECOND_WANT_PCM | E2ECOND_WANT_WAV: what is computed and kept RESIDENT.
 *   width     receives max_b n_out[b]; every row is written over `width` samples, zeros at and past its n_out.
 *   pcm_out, wav_out  [B] rows out_stride >= width elements apart; each needs its E2ECOND_WANT_* bit.
 * The resident outputs are laid out with rows e2econd_out_stride() elements apart (width rounded up to 8; the padding is zero) until the next
 * analyze or apply.  width == 0 computes nothing. */
E2ECOND_API int e2econd_apply(e2econd_handle* handle, const double* gain, int want, int16_t* pcm_out, float* wav_out, long long out_stride, long long* width);
E2ECOND_API const int16_t* e2econd_pcm_dev(e2econd_handle* handle);   /* NULL when not resident */
E2ECOND_API const float* e2econd_wav_dev(e2econd_handle* handle);
E2ECOND_API long long e2econd_out_stride(const e2econd_handle* handle);

/* Starts per workgroup of the window test for the configured W (0 before e2econd_configure). */
E2ECOND_API long long e2econd_tile_starts(const e2econd_handle* handle);

/* Measurement aid: with profiling on, downmix, analyze and apply record HIP events around their phases; e2econd_profile_read gives the last
 * call's milliseconds as {upload, compute, fetch}. */
E2ECOND_API int e2econd_profile_enable(e2econd_handle* handle, int on);
E2ECOND_API int e2econd_profile_read(e2econd_handle* handle, double ms_out[3]);

#ifdef E2ECOND_TEST_HOOKS
/* Test build only (libe2etts_condition_test.so): fills every workspace of the handle with NaN bit patterns; nothing is resident and no
 * analysis is held afterwards. */
E2ECOND_API int e2econd_debug_poison_workspace(e2econd_handle* handle);
#endif

#ifdef __cplusplus
}
#endif
#endif
