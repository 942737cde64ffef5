/* e2etts_align.h -- C ABI of the forced-alignment companion library (libe2etts_align.so).
 *
 * Serves the reference's AlignmentEncoder (U/layers.py:275-369) and its monotonic alignment search (binarize_attention_parallel,
 * U/layers.py:124-134; mas_width1 / b_mas, U/function.py:96-137) on the GPU: given a recording's mel, the phoneme embeddings and the
 * speaker vector, which frames belong to which phoneme.  U/ = e2e_tts/models/acoustic/unsupervised_fastspeech2/.
 *
 * A library of its own next to libe2etts_hip.so (include/e2etts.h), whose ABI it leaves untouched: the aligner does not use the encoder
 * stack -- its keys are the embedding rows src_word_emb(ids), the second value every Encoder.forward returns -- and its weights travel in
 * a blob of their own (e2e_tts_amd.packer.pack_aligner; the container of e2etts_load_weights).
 *
 * Conventions (those of e2etts.h)
 *  - plain C; every function returns 0 or a negative E2EALIGN_E* code, e2ealign_last_error() gives the message;
 *  - data pointers may be host OR device memory (hipMemcpyDefault); every output pointer may be NULL;
 *  - the handle works on its own non-blocking stream and every entry point returns after that stream has drained; work the caller still
 *    has queued on a stream of its own that writes an input (or reads an output) is ordered with e2ealign_order_after;
 *  - every argument, the length arrays included, is validated BEFORE anything is enqueued: a call that returns E2EALIGN_EINVAL has
 *    enqueued nothing, the resident maps are what they were and the handle stays usable (a failure after validation is E2EALIGN_EHIP or
 *    E2EALIGN_ENOMEM; the resident maps are then gone);
 *  - the length arrays are READ DURING VALIDATION, by a blocking copy when they lie in device memory: such an array must be complete when
 *    the call is made (synchronise the stream that wrote it -- e2ealign_order_after orders the data tensors, not this read);
 *  - e2ealign_create opens no device: the GPU is first touched by e2ealign_load_weights or by the first call that computes;
 *  - arithmetic is exact fp32 throughout (durations are a discrete decision: no split-precision or bf16 path);
 *  - workspaces grow with the largest (B, T, L) seen and are never shrunk; steady state allocates nothing.  Device memory is
 *    O(B * T * L): three [B, T, L] maps (attn, attn_logprob, attn_hard), one back-pointer BIT per cell, and O(B * (T + L) * channels)
 *    for the projections.  The reference's [B, n_att, T, L] difference tensor is never formed.  A prior given in host memory is staged
 *    in one more [B, T, L] buffer; a generated one (e2ealign_forward_bb / e2ealign_align_bb) holds nothing of its own.
 *  - one handle is used by one thread at a time (calls are serialised by a mutex inside).
 */
#ifndef E2ETTS_ALIGN_H
#define E2ETTS_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2EALIGN_API __attribute__((visibility("default")))
#else
#define E2EALIGN_API
#endif

#define E2EALIGN_ABI_VERSION 2

#define E2EALIGN_OK 0
#define E2EALIGN_EINVAL (-1)   /* bad argument / shape / length, a weight blob without one of the aligner's tensors */
#define E2EALIGN_EHIP (-2)     /* HIP runtime error, or a kernel launcher's refusal after validation (a defect, not an argument error) */
#define E2EALIGN_ESTATE (-3)   /* call order (forward before weights are loaded) */
#define E2EALIGN_ENOMEM (-4)

/* limits of the kernels (E2EALIGN_EINVAL beyond them) */
#define E2EALIGN_MAX_ATT 128   /* n_att_channels */
#define E2EALIGN_MAX_L 2048    /* phonemes per row */
#define E2EALIGN_MAX_B 4096
#define E2EALIGN_MAX_PRIOR_SCALING 1048576.0   /* 2^20: the largest `scaling` of a generated prior (every log-gamma argument stays finite) */

/* e2ealign_mas / e2ealign_align flags */
#define E2EALIGN_LOG_MAP 1     /* `map` already holds log-probabilities: the search does not take the logarithm */

typedef struct e2ealign_handle e2ealign_handle;

E2EALIGN_API const char* e2ealign_version(void);
E2EALIGN_API int e2ealign_abi_version(void);
/* Last error message of this handle (or of a failed e2ealign_create when handle == NULL). */
E2EALIGN_API const char* e2ealign_last_error(const e2ealign_handle* handle);

/* AlignmentEncoder(n_mel_channels, n_att_channels, n_text_channels, temperature) (U/layers.py:278-330) on GPU `device_id`.
 * n_mel and n_text must be multiples of 4 (the exact-fp32 convolution's row alignment), n_att <= E2EALIGN_MAX_ATT. */
E2EALIGN_API int e2ealign_create(int device_id, int n_mel, int n_att, int n_text, float temperature, e2ealign_handle** out);
E2EALIGN_API void e2ealign_destroy(e2ealign_handle* handle);

/* load_state_dict: `blob` is packer.pack_aligner's image (host or device memory), copied into handle-owned HBM.  The directory is
 * checked on the host first: a missing tensor or one of the wrong size is E2EALIGN_EINVAL and the weights loaded before stay. */
E2EALIGN_API int e2ealign_load_weights(e2ealign_handle* handle, const void* blob, size_t nbytes);

E2EALIGN_API void* e2ealign_stream(e2ealign_handle* handle);   /* the handle's hipStream_t (opens the device) */
E2EALIGN_API int e2ealign_order_after(e2ealign_handle* handle, void* caller_stream);
E2EALIGN_API int e2ealign_sync(e2ealign_handle* handle);
E2EALIGN_API size_t e2ealign_device_bytes(const e2ealign_handle* handle);   /* HBM the handle holds now (weights + workspaces) */

/* AlignmentEncoder.forward (U/layers.py:332-369).
 *   mel      [B, T, n_mel] fp32, CHANNELS-LAST (the engine's native layout, what e2etts_fetch_mel returns; the reference's `queries` is
 *            its transpose [B, n_mel, T]).  Padded frames carry data like every other frame (the reference's convolutions see them).
 *   keys     [B, L, n_text] fp32: the embedding rows of the phoneme ids (the reference's `keys` transposed), pad rows included.
 *   speaker  [B, n_text] fp32 speaker vectors, or NULL (speaker_embed=None): key_spk_proj / query_spk_proj of them are added to every
 *            position before the projections.
 *   txt_lens [B] int64 (1 <= txt_lens[b] <= L): keys >= txt_lens[b] are masked (the reference's prefix mask), or NULL (mask=None).
 *   prior    [B, T, L] fp32 or NULL (attn_prior=None).  With a prior the log-softmax runs over ALL L columns, padded keys included,
 *            because the mask comes after it.
 * Outputs (each may be NULL): attn [B, T, L] (exactly 0 at masked keys), attn_logprob [B, T, L] (before the mask).  Both stay RESIDENT
 * in the handle until the next forward / align. */
E2EALIGN_API int e2ealign_forward(e2ealign_handle* handle, const float* mel, const float* keys, const float* speaker, const int64_t* txt_lens,
                                  const float* prior, int B, int T, int L, float* attn_out, float* attn_logprob_out);

/* b_mas(attn, in_lens, out_lens, width=1) (U/function.py:96-137), index for index on the slice [:out_lens[b], :in_lens[b]] of each row:
 * log in fp32 (log 0 = -inf), row 0 columns >= 1 set to -inf, log_p[i, j] = a[i, j] + max(prev[j], prev[j - 1]) with the diagonal taken
 * on >= (ties and -inf ties go diagonal), backtracking from column in_lens[b] - 1, and the reference's closing opt[0, 0] = 1.
 *   map      [B, T, L] fp32 probabilities -- or log-probabilities with E2EALIGN_LOG_MAP -- or NULL: the resident attn of the last forward
 *            (B, T, L must then be that call's; E2EALIGN_EINVAL if nothing is resident).
 *   in_lens  [B] int64, 1 <= in_lens[b] <= L;  out_lens [B] int64, 1 <= out_lens[b] <= T.
 * Outputs (each may be NULL): attn_hard [B, T, L] fp32 (0 / 1, zero outside the slice), dur [B, L] fp32 = attn_hard.sum over frames. */
E2EALIGN_API int e2ealign_mas(e2ealign_handle* handle, const float* map, int flags, const int64_t* in_lens, const int64_t* out_lens, int B, int T,
                              int L, float* attn_hard_out, float* dur_out);

/* Both in one call (the attn_out of VarianceAdaptor.forward, U/layers.py:203-212): forward with the mask of txt_lens, then the search on
 * its attn with in_lens = txt_lens, out_lens = mel_lens.  Only what is asked for leaves the device. */
E2EALIGN_API int e2ealign_align(e2ealign_handle* handle, const float* mel, const float* keys, const float* speaker, const int64_t* txt_lens,
                                const int64_t* mel_lens, const float* prior, int B, int T, int L, float* dur_out, float* attn_hard_out,
                                float* attn_out, float* attn_logprob_out);

/* The beta-binomial attention prior of the reference's data preparation (beta_binomial_prior_distribution, TOOLS/utils.py:129-139, padded
 * by the collate function, dataloader.py:274-281; TOOLS/ = e2e_tts/src/tools/), generated on the device.  For row b with
 * P = txt_lens[b] phonemes, M = mel_lens[b] frames and a scaling factor s = `scaling`:
 *
 *     prior[b, t, k] = fp32( C(n, k) * B(k + alpha, n - k + beta) / B(alpha, beta) )
 *                      with n = P, alpha = s * (t + 1), beta = s * (M - t),   for 0 <= t < M, 0 <= k < P
 *     prior[b, t, k] = 0 everywhere else in the padded [T, L]
 *
 *  - the reference's quirk is kept: n = P trials, but only the outcomes 0 .. P - 1 are stored, so a row does not sum to 1;
 *  - the value is evaluated in float64 through log-gamma terms and rounded to fp32 once; a result below fp32's normal range may come out
 *    as the subnormal or as 0;
 *  - 1 <= txt_lens[b] <= L, 1 <= mel_lens[b] <= T, both arrays required; `scaling` finite, > 0 and <= E2EALIGN_MAX_PRIOR_SCALING.
 * `prior_out` [B, T, L] fp32, host or device memory, must not be NULL (it is the call's only result).  Needs no weights and leaves the
 * resident maps alone. */
E2EALIGN_API int e2ealign_prior(e2ealign_handle* handle, const int64_t* txt_lens, const int64_t* mel_lens, int B, int T, int L, double scaling,
                                float* prior_out);

/* e2ealign_forward / e2ealign_align with the prior of e2ealign_prior(txt_lens, mel_lens, scaling) GENERATED inside the attention pass: the
 * same bits as the call that is handed e2ealign_prior's tensor, without a [B, T, L] prior in memory (nothing is uploaded, no staging
 * buffer is held).  Both length arrays are required; txt_lens is also the mask. */
E2EALIGN_API int e2ealign_forward_bb(e2ealign_handle* handle, const float* mel, const float* keys, const float* speaker, const int64_t* txt_lens,
                                     const int64_t* mel_lens, double scaling, int B, int T, int L, float* attn_out, float* attn_logprob_out);
E2EALIGN_API int e2ealign_align_bb(e2ealign_handle* handle, const float* mel, const float* keys, const float* speaker, const int64_t* txt_lens,
                                   const int64_t* mel_lens, double scaling, int B, int T, int L, float* dur_out, float* attn_hard_out,
                                   float* attn_out, float* attn_logprob_out);

/* Measurement aid: with profiling on, every forward / mas / align records HIP events around its phases; e2ealign_profile_read gives the
 * last call's milliseconds as {projections, attention pass, search} (0 for a phase the call did not run). */
E2EALIGN_API int e2ealign_profile_enable(e2ealign_handle* handle, int on);
E2EALIGN_API int e2ealign_profile_read(e2ealign_handle* handle, double ms_out[3]);

#ifdef E2EALIGN_TEST_HOOKS
/* Test build only (libe2etts_align_test.so; the product library does not export it): fills every workspace of the handle (the resident
 * maps included, the weights not) with NaN bit patterns. */
E2EALIGN_API int e2ealign_debug_poison_workspace(e2ealign_handle* handle);
/* Test build only: the attention pass of e2ealign_forward ALONE, on projections given by the caller instead of computed from weights (none
 * need be loaded): q [B, T, n_att], k [B, L, n_att] fp32, prior [B, T, L] | NULL, txt_lens [B] int64 | NULL, host or device memory.  Same
 * validation of B, T, L and txt_lens as e2ealign_forward, same choice of the frame tile (one function launches both), same outputs. */
E2EALIGN_API int e2ealign_debug_attention(e2ealign_handle* handle, const float* q, const float* k, const float* prior, const int64_t* txt_lens,
                                          int B, int T, int L, float* attn_out, float* attn_logprob_out);
/* Test build only: the same with the generated prior that e2ealign_forward_bb takes: txt_lens and mel_lens are required. */
E2EALIGN_API int e2ealign_debug_attention_bb(e2ealign_handle* handle, const float* q, const float* k, const int64_t* txt_lens,
                                             const int64_t* mel_lens, double scaling, int B, int T, int L, float* attn_out,
                                             float* attn_logprob_out);
#endif

#ifdef __cplusplus
}
#endif
#endif
