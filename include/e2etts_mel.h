/* e2etts_mel.h -- C ABI of the mel front-end companion library (libe2etts_mel.so).
 *
 * Serves the analysis side of the reference, TorchSTFT.mel_spectrogram / generate_melspecs (e2e_tts/src/tools/stft.py:11-89, :107-135,
 * with dynamic_range_compression of src/tools/utils.py:22-28), on the GPU: a recording -> log-mel frames and frame energies, the inputs of
 * forced alignment (include/e2etts_align.h) and of the energy controls.  Per row:
 *
 *   F.pad(reflect, (n_fft - hop) / 2)  ->  framed DFT, periodic Hann window, center=False, onesided
 *   mag = sqrt((re^2 + im^2) + 1e-9)   ->  mel = basis @ mag  ->  log(max(mel, clip_val));   energy = sqrt(sum_k mag_k^2)
 *
 * A library of its own next to libe2etts_hip.so and libe2etts_align.so, whose ABIs it leaves untouched; it shares their kernel objects
 * (the transform is the exact-fp32 convolution the denoiser's forward STFT runs on).
 *
 * Conventions (those of e2etts_align.h)
 *  - plain C; every function returns 0 or a negative E2EMEL_E* code, e2emel_last_error() gives the message;
 *  - data pointers may be host OR device memory (hipMemcpyDefault); every output pointer may be NULL;
 *  - the handle works on its own non-blocking stream and every entry point returns after that stream has drained; work the caller still
 *    has queued on a stream of its own that writes an input (or reads an output) is ordered with e2emel_order_after;
 *  - every argument, the length array included, is validated BEFORE anything is enqueued: a call that returns E2EMEL_EINVAL has enqueued
 *    nothing, the resident outputs are what they were and the handle stays usable (a failure after validation is E2EMEL_EHIP or
 *    E2EMEL_ENOMEM; the resident outputs are then gone);
 *  - n_valid is READ DURING VALIDATION, by a blocking copy when it lies in device memory: it must be complete when the call is made;
 *  - e2emel_create opens no device: the GPU is first touched by e2emel_load;
 *  - arithmetic is exact fp32 throughout (the mel feeds a discrete decision, the durations: no split-precision or bf16 path);
 *  - workspaces grow with the largest (B, n) seen and are never shrunk; steady state allocates nothing.  Device memory is
 *    O(B * R * (hop + Cpad)) with R = T + n_overlap - 1 rows and Cpad = 2 * bins rounded up to 32: the padded rows and one spectrum;
 *    magnitudes never reach HBM;
 *  - one handle is used by one thread at a time (calls are serialised by a mutex inside).
 *
 * NOT reproduced: the reference's two asserts on fp32 input (min >= -1, max <= 1, stft.py:56-57).  Checking them needs a pass over the
 * samples and a device round trip before anything is enqueued; samples outside [-1, 1] are transformed as they are.  (The Python mirror
 * models.TorchSTFT checks them, as the reference does.)
 */
#ifndef E2ETTS_MEL_H
#define E2ETTS_MEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2EMEL_API __attribute__((visibility("default")))
#else
#define E2EMEL_API
#endif

#define E2EMEL_ABI_VERSION 1

#define E2EMEL_OK 0
#define E2EMEL_EINVAL (-1)   /* bad argument / geometry / length */
#define E2EMEL_EHIP (-2)     /* HIP runtime error, or a kernel launcher's refusal after validation (a defect, not an argument error) */
#define E2EMEL_ESTATE (-3)   /* call order (forward before the bases are loaded) */
#define E2EMEL_ENOMEM (-4)

#define E2EMEL_MAX_B 4096
#define E2EMEL_MAX_MEL 1024  /* n_mel */

/* e2emel_forward dtype */
#define E2EMEL_F32 0         /* float samples in [-1, 1] */
#define E2EMEL_I16 1         /* int16 PCM, divided by 32768 (exact in fp32): audio / max_wav_value of the reference's data preparation */

typedef struct e2emel_handle e2emel_handle;

E2EMEL_API const char* e2emel_version(void);
E2EMEL_API int e2emel_abi_version(void);
/* Last error message of this handle (or of a failed e2emel_create when handle == NULL). */
E2EMEL_API const char* e2emel_last_error(const e2emel_handle* handle);

/* TorchSTFT(filter_length = n_fft, hop_length = hop, n_mel_channels = n_mel) on GPU `device_id`.  Geometry served is what the exact-fp32
 * framing serves: n_fft = hop * n_overlap with n_overlap in {2, 4, 8}, hop % 32 == 0, hop <= 1024; n_mel % 4 == 0 (the row alignment of
 * e2ealign_forward, which reads the result), n_mel <= E2EMEL_MAX_MEL.  Anything else is E2EMEL_EINVAL: there is no other path. */
E2EMEL_API int e2emel_create(int device_id, int n_fft, int hop, int n_mel, e2emel_handle** out);
E2EMEL_API void e2emel_destroy(e2emel_handle* handle);

/* The two matrices, host (or device) memory, copied into handle-owned HBM; bins = n_fft / 2 + 1.
 *   dft_basis [2 * bins, n_fft] fp32: rows 0 .. bins - 1 = window[n] * cos(2 pi k n / n_fft), rows bins .. = window[n] * sin(...) (the
 *             sign of the imaginary part does not matter: only re^2 + im^2 is used), built in float64 and rounded once; a window shorter
 *             than n_fft is centre-padded with zeros, as torch.stft does (e2e_tts_amd.mel.dft_basis).
 *   mel_basis [n_mel, bins] fp32, any matrix (librosa.filters.mel's in the reference).  The first and last non-zero bin of every row are
 *             recorded here and the projection sums each row over that band only, in ascending bin order: skipped terms are exact zeros.
 *   clip_val  dynamic_range_compression's clamp (1e-5 in the reference); must be a positive finite number.  A clamped element is written as
 *             log(clip_val) computed in float64 and rounded once (what a correctly rounded fp32 log gives), the others go through logf.
 * The new bases are staged in buffers of their own and swapped in when all of them have arrived: a load that fails, with whatever code,
 * leaves the bases loaded before in place and the handle as usable as it was. */
E2EMEL_API int e2emel_load(e2emel_handle* handle, const float* dft_basis, const float* mel_basis, float clip_val);

E2EMEL_API void* e2emel_stream(e2emel_handle* handle);   /* the handle's hipStream_t (opens the device) */
E2EMEL_API int e2emel_order_after(e2emel_handle* handle, void* caller_stream);
E2EMEL_API int e2emel_sync(e2emel_handle* handle);
E2EMEL_API size_t e2emel_device_bytes(const e2emel_handle* handle);   /* HBM the handle holds now (bases + workspaces) */

/* mel_spectrogram(audio, return_energy=True) of a batch of recordings.
 *   audio        B rows of n samples, row b at audio + b * audio_stride ELEMENTS (audio_stride >= n); dtype E2EMEL_F32 or E2EMEL_I16.
 *   n_valid      [B] int64 samples of each row, or NULL (every row has n).  Needs (n_fft - hop) / 2 < n_valid[b] <= n (a shorter row
 *                cannot be reflected: torch raises there) and n_valid[b] >= hop (at least one frame).
 *   T_out        receives T = max_b floor(n_valid[b] / hop), the frame count the outputs are laid out with.  The caller sizes the
 *                outputs with the same formula before the call.
 *   mel_out      [B, T, n_mel] fp32, CHANNELS-LAST: the layout e2ealign_forward and e2etts_vocoder_btc take (the reference returns its
 *                transpose [B, n_mel, T]).
 *   energy_out   [B, T] fp32.
 *   mel_lens_out [B] int64 = floor(n_valid[b] / hop).
 * Every row is padded, reflected and framed OVER ITS OWN LENGTH: row b equals a B = 1 call on that row.  (The reference, given one
 * zero-padded batch, reflects at the batch's end; the denoiser makes the same choice as this library.)  Frames >= mel_lens[b] are written
 * as 0 in both outputs and are not computed.  The energy is reduced in a fixed order without atomics: the result does not depend on
 * the batch or the grid.  Both outputs stay RESIDENT in the handle until the next forward. */
E2EMEL_API int e2emel_forward(e2emel_handle* handle, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n,
                              float* mel_out, float* energy_out, int64_t* mel_lens_out, int* T_out);

/* Device pointers of the resident outputs of the last forward ([B, T, n_mel] / [B, T] of that call), NULL when nothing is resident:
 * what e2ealign_align reads without a copy through the host (order it with e2ealign_order_after(e2emel_stream())). */
E2EMEL_API const float* e2emel_mel_dev(e2emel_handle* handle);
E2EMEL_API const float* e2emel_energy_dev(e2emel_handle* handle);

/* Frames one workgroup of the fused tail kernel takes for this geometry (a power of two <= 16, by the LDS one tile of magnitudes needs). */
E2EMEL_API int e2emel_tile_frames(const e2emel_handle* handle);

/* Measurement aid: with profiling on, every forward records HIP events around its phases; e2emel_profile_read gives the last call's
 * milliseconds as {pad, transform, tail}. */
E2EMEL_API int e2emel_profile_enable(e2emel_handle* handle, int on);
E2EMEL_API int e2emel_profile_read(e2emel_handle* handle, double ms_out[3]);

#ifdef E2EMEL_TEST_HOOKS
/* Test build only (libe2etts_mel_test.so; the product library does not export it): fills every workspace of the handle (the resident
 * outputs included, the bases not) with NaN bit patterns. */
E2EMEL_API int e2emel_debug_poison_workspace(e2emel_handle* handle);
/* Test build only: on != 0 replaces the band table recorded by the last e2emel_load with the degenerate band [0, bins - 1] of every row
 * (the tail kernel then walks all bins, explicit zeros included, as it does for a dense matrix); 0 puts the recorded bands back. */
E2EMEL_API int e2emel_debug_force_dense(e2emel_handle* handle, int on);
/* Test build only: the tail kernel alone.  The caller's spectrum spec [B, T + n_overlap - 1, Cpad] fp32 (host or device; row f of an
 * utterance holds re[0 .. bins) | im[0 .. bins) of frame f, Cpad = 2 * bins rounded up to a multiple of 32; the last n_overlap - 1 rows
 * are never read) goes straight into mel_tail_kernel, through the function e2emel_forward launches it through, with frames [B] int32
 * (host or device, 0 <= frames[b] <= T) as the rows' frame counts.  mel_out [B, T, n_mel] and energy_out [B, T] as e2emel_forward writes
 * them.  The transform's basis is not used: the handle may have been loaded with any dft_basis. */
E2EMEL_API int e2emel_debug_tail(e2emel_handle* handle, const float* spec, const int32_t* frames, int B, int T, float* mel_out, float* energy_out);
#endif

#ifdef __cplusplus
}
#endif
#endif
