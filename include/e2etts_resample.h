/* e2etts_resample.h -- C ABI of the sample-rate conversion companion library (libe2etts_resample.so).
 *
 * A batched, streaming, rational-ratio polyphase FIR resampler on the GPU.  The reference changes rates through pydub.set_frame_rate
 * (modules/metrics/audio_processing.py:26), which is audioop.ratecv: linear interpolation without an anti-aliasing filter.  That is NOT
 * reproduced; this library defines its own arithmetic, which equals scipy.signal.resample_poly(x, L, M, window = taps / L).
 *
 * Arithmetic.  Conversion by L / M, gcd(L, M) = 1, output rate = input rate * L / M, odd-length taps h[0 .. 2 half] centred at half:
 *
 *   n_out = ceil(n_valid * L / M)
 *   c(m)  = m * M + half                                  (int64)
 *   y[m]  = sum_k x[k] * h[c(m) - k * L]                  over all k with 0 <= k < n_valid and 0 <= c(m) - k * L <= 2 half
 *
 * The sum is ONE fp32 FMA chain, acc = fmaf(x[k], h[..], acc) from acc = +0.0f with k ascending: no atomics, no split sums, no
 * reassociation.  Every output sample is therefore a pure function of (row, m): it does not depend on the tile, the grid, the batch or
 * the chunking of a stream.  Samples outside [0, n_valid) are zeros (multiplied or skipped: the bits are the same for finite taps, and
 * e2ers_load refuses others).  Input is fp32, or int16 PCM divided by 32768 (exact).  Output is fp32 and / or int16 PCM =
 * trunc(y * 32768) saturated to [-32768, 32767], computed from the fp32 y (e2etts_denoise's rule).
 *
 * The library only ever sees taps, L and M; e2e_tts_amd.resample.design builds the default Kaiser-windowed sinc in float64.
 *
 * A library of its own next to libe2etts_hip.so, libe2etts_align.so and libe2etts_mel.so, whose ABIs it leaves untouched.
 *
 * Conventions (those of e2etts_mel.h)
 *  - plain C; every function returns 0 or a negative E2ERS_E* code, e2ers_last_error() gives the message;
 *  - data pointers may be host OR device memory; every output pointer may be NULL;
 *  - the handle works on its own non-blocking stream.  Every entry point but e2ers_stream_push returns after that stream has drained;
 *    work the caller still has queued on a stream of its own that writes an input (or reads an output) is ordered with e2ers_order_after;
 *  - every argument, the length array included, is validated BEFORE anything is enqueued: a call that returns E2ERS_EINVAL has enqueued
 *    nothing, the resident outputs are what they were and the handle stays usable;
 *  - n_valid is READ DURING VALIDATION, by a blocking copy when it lies in device memory;
 *  - e2ers_create opens no device: the GPU is first touched by e2ers_load;
 *  - workspaces grow with the largest call seen and are never shrunk; steady state allocates nothing;
 *  - one handle is used by one thread at a time (calls are serialised by a mutex inside).
 */
#ifndef E2ETTS_RESAMPLE_H
#define E2ETTS_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2ERS_API __attribute__((visibility("default")))
#else
#define E2ERS_API
#endif

#define E2ERS_ABI_VERSION 1

#define E2ERS_OK 0
#define E2ERS_EINVAL (-1)   /* bad argument / filter / length */
#define E2ERS_EHIP (-2)     /* HIP runtime error */
#define E2ERS_ESTATE (-3)   /* call order (no filter loaded, no stream open, nothing to fetch, two pushes already unfetched) */
#define E2ERS_ENOMEM (-4)

#define E2ERS_MAX_B 4096
#define E2ERS_MAX_RATIO 1024        /* L and M */
#define E2ERS_MAX_PHASE_TAPS 1024   /* P = ceil(n_taps / L): the taps one output sample sums */

/* dtype of the input samples */
#define E2ERS_F32 0         /* float samples */
#define E2ERS_I16 1         /* int16 PCM, divided by 32768 (exact in fp32) */

typedef struct e2ers_handle e2ers_handle;

E2ERS_API const char* e2ers_version(void);
E2ERS_API int e2ers_abi_version(void);
/* Last error message of this handle (or of a failed e2ers_create when handle == NULL). */
E2ERS_API const char* e2ers_last_error(const e2ers_handle* handle);

E2ERS_API int e2ers_create(int device_id, e2ers_handle** out);
E2ERS_API void e2ers_destroy(e2ers_handle* handle);

/* The filter: n_taps fp32 taps (host or device memory), odd in number, and the ratio L / M.  Refused (E2ERS_EINVAL): an even n_taps,
 * gcd(L, M) != 1, L or M outside [1, E2ERS_MAX_RATIO], a tap that is not finite, P = ceil(n_taps / L) > E2ERS_MAX_PHASE_TAPS.
 * Builds the phase-major table G[r][i] = h[r + i * L] (zero past the last tap; r < L, i < P) in handle-owned HBM: output m with
 * r = c(m) mod L and k_hi = c(m) div L sums x[k_hi - i] * G[r][i].  The table is staged in a buffer of its own and swapped in when it has
 * arrived: a load that fails, with whatever code, leaves the filter loaded before in place.  A successful load closes an open stream and
 * forgets the resident outputs. */
E2ERS_API int e2ers_load(e2ers_handle* handle, const float* taps, int n_taps, int L, int M);

E2ERS_API void* e2ers_stream(e2ers_handle* handle);   /* the handle's hipStream_t (opens the device) */
E2ERS_API int e2ers_order_after(e2ers_handle* handle, void* caller_stream);
E2ERS_API int e2ers_sync(e2ers_handle* handle);
E2ERS_API size_t e2ers_device_bytes(const e2ers_handle* handle);   /* HBM the handle holds now (table + workspaces) */

/* One conversion of a batch.
 *   audio       B rows of n samples, row b at audio + b * audio_stride ELEMENTS (audio_stride >= n); dtype E2ERS_F32 or E2ERS_I16.
 *   n_valid     [B] int64 samples of each row, each in [0, n], or NULL (every row has n).  A row of 0 samples yields 0 outputs.
 *   n_out_max   receives ceil(n * L / M), the width the outputs are laid out with; the caller sizes them with the same formula.
 *   wav_out     [B] rows of fp32, row b at wav_out + b * out_stride elements (out_stride >= n_out_max); n_out_max samples of a row are
 *               written, those at or past the row's own n_out = ceil(n_valid[b] * L / M) as 0.
 *   pcm_out     the same layout in int16 PCM.
 *   n_out_lens  [B] int64 = ceil(n_valid[b] * L / M).
 * Row b equals a B = 1 call on that row, bit for bit.  Both outputs stay RESIDENT in the handle ([B, n_out_max], dense) until the next
 * e2ers_forward; a stream does not touch them. */
E2ERS_API int e2ers_forward(e2ers_handle* handle, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n,
                            float* wav_out, int16_t* pcm_out, long long out_stride, int64_t* n_out_lens, long long* n_out_max);

/* Device pointers of the resident outputs of the last forward ([B, n_out_max] dense), NULL when nothing is resident. */
E2ERS_API const float* e2ers_wav_dev(e2ers_handle* handle);
E2ERS_API const int16_t* e2ers_pcm_dev(e2ers_handle* handle);

/* Streaming: B parallel rows of equal length, fed in chunks of any size.
 *   _begin(B, dtype)  opens a stream (abandoning an open one).
 *   _push(chunk, chunk_stride, n, last, &n_ready)  appends n samples per row (row b at chunk + b * chunk_stride elements; n may be 0, chunk
 *         then NULL) and enqueues the outputs that became final.  After N samples in total the outputs m < E' exist, E' =
 *         floor((N * L - 1 - half) / M) + 1 (0 if that is negative); with last != 0 every m < ceil(N * L / M) exists and the stream is
 *         closed to further pushes.  A push with n = 0 and last = 1 flushes.  *n_ready receives the outputs per row THIS push made
 *         (possibly 0).  The handle keeps the input history from sample max(0, ceil((E' * M - half) / L)) on, nothing older.
 *         _push RETURNS ONCE ENQUEUED.  A chunk in host memory has been consumed when it returns; one in device memory must stay valid
 *         until the fetch of that push (or e2ers_sync) returns.  At most two pushes with outputs may be unfetched: a third is E2ERS_ESTATE.
 *   _fetch(wav_out, pcm_out, out_stride, capacity)  drains the stream and hands out the outputs of the OLDEST unfetched push that made
 *         any: [B] rows of its n_ready samples, out_stride elements apart (out_stride >= n_ready; capacity, in elements, must hold
 *         (B - 1) * out_stride + n_ready).  E2ERS_ESTATE when nothing is unfetched.
 * The concatenated pieces are bit-identical to e2ers_forward of the concatenated input, for any chunking. */
E2ERS_API int e2ers_stream_begin(e2ers_handle* handle, int B, int dtype);
E2ERS_API int e2ers_stream_push(e2ers_handle* handle, const void* chunk, long long chunk_stride, long long n, int last, long long* n_ready);
E2ERS_API int e2ers_stream_fetch(e2ers_handle* handle, float* wav_out, int16_t* pcm_out, long long out_stride, size_t capacity);

/* Output samples one workgroup produces for the loaded filter (0 before a load). */
E2ERS_API long long e2ers_tile_outputs(const e2ers_handle* handle);

/* Measurement aid: with profiling on, every forward records HIP events around its phases; e2ers_profile_read gives the last call's
 * milliseconds as {upload, filter, fetch}. */
E2ERS_API int e2ers_profile_enable(e2ers_handle* handle, int on);
E2ERS_API int e2ers_profile_read(e2ers_handle* handle, double ms_out[3]);

#ifdef E2ERS_TEST_HOOKS
/* Test build only (libe2etts_resample_test.so; the product library does not export it): fills every workspace of the handle (the resident
 * outputs and an open stream's state included, the table not) with NaN bit patterns; nothing is resident and no stream is open afterwards. */
E2ERS_API int e2ers_debug_poison_workspace(e2ers_handle* handle);
#endif

#ifdef __cplusplus
}
#endif
#endif
