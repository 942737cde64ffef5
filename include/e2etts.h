/*
 * e2etts.h -- C ABI of the MI355X-native FastSpeech2 + HiFi-GAN inference engine.
 *
 * The reference (InterlinkLabs/e2e-tts) has no FFI / plugin interface: its hot path is a stack of
 * Python classes calling torch.  This header is the boundary this project puts
 * underneath Python mirrors of those classes; every entry point names the reference call it serves.
 * Paths are relative to the reference root; U/ = e2e_tts/models/acoustic/unsupervised_fastspeech2/,
 * V/ = e2e_tts/models/vocoder/, API/ = e2e_tts/src/api/.
 *
 * Conventions
 *  - plain C, no torch types; every function returns 0 on success or a negative E2ETTS_E* code, and
 *    e2etts_last_error() gives the message (no exceptions cross the boundary);
 *  - data pointers may be host OR device memory: copies use hipMemcpyDefault, so a caller that keeps
 *    its buffers in HBM (bench.py, the torch-tensor mirrors) pays no PCIe transfer;
 *  - STREAM ORDERING of device buffers: the engine works on its own non-blocking stream and every entry point
 *    returns only after that stream has drained, so results are complete on return.  What the engine cannot
 *    see is work the CALLER still has queued on a stream of its own that writes an input buffer (or still reads
 *    a buffer handed in as an output): call e2etts_order_after(engine, that_stream) first -- the engine's stream
 *    then waits for everything queued on that stream so far -- or synchronise that stream yourself.  The Python
 *    binding does this for every torch CUDA tensor argument (torch.cuda.current_stream());
 *  - one engine = one GPU + one HIP stream (at small batches the vocoder forks the ResBlocks of a stage onto internal side
 *    streams and joins them back into that stream before anything else reads their sum: invisible to the caller, same
 *    results bit for bit); calls on one engine are serialised by an internal mutex;
 *    distinct engines are independent (one process per GPU in multi-GPU runs);
 *  - activations are channels-last ([B, N, C]); what the vocoder keeps in HBM between layers, per vocoder precision (below):
 *      E2ETTS_PRECISION_FP32      fp32 activations, fp32 weights;
 *      E2ETTS_PRECISION_BF16X3    fp32 activations, weights as bf16 hi + lo pairs;
 *      E2ETTS_PRECISION_BF16      fp32 activations, residuals and stage sums (a bf16 copy of a conv's input where two launches hand one
 *                                 over), bf16 weight images;
 *      E2ETTS_PRECISION_BF16_ACT  bf16 activations, residuals and stage sums (2 bytes per element), bf16 weight images, bf16-rounded biases;
 *      E2ETTS_PRECISION_FP16_ACT  fp16 (IEEE binary16) activations, residuals and stage sums (2 bytes per element), fp16 weight images,
 *                                 fp16-rounded biases (both built when the mode is first selected);
 *    the acoustic model's activations are fp32 in every mode.  Weights come packed by e2e_tts_amd/packer.py (weight-norm and BatchNorm
 *    folded, conv weights tap-major).
 */
#ifndef E2ETTS_H
#define E2ETTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported. */
#if defined(__GNUC__) || defined(__clang__)
#define E2ETTS_API __attribute__((visibility("default")))
#else
#define E2ETTS_API
#endif

/* ABI revision of this header: bumped whenever a struct layout or a signature changes.  A host checks e2etts_abi_version() ==
 * E2ETTS_ABI_VERSION (the Python binding does at load) and fills e2etts_config.struct_size, which e2etts_create checks. */
#define E2ETTS_ABI_VERSION 4

#define E2ETTS_MAX_STAGES 8
#define E2ETTS_MAX_RB_KERNELS 4
#define E2ETTS_MAX_DILATIONS 4

#define E2ETTS_OK 0
#define E2ETTS_EINVAL (-1)   /* bad argument / shape (the Python mirror raises ValueError) */
#define E2ETTS_EHIP (-2)     /* HIP runtime error */
#define E2ETTS_ESTATE (-3)   /* call order (e.g. vocoder before weights are loaded) */
#define E2ETTS_ENOMEM (-4)
#define E2ETTS_EKEY (-5)     /* tensor missing from the weight blob (KeyError) */

/* Dimensions parsed from the reference's config.yaml (API/utils.py:34; e2e_tts/config/model_config.yaml). */
typedef struct e2etts_config {
  uint32_t struct_size;   /* = sizeof(e2etts_config) of the header the CALLER was compiled against.  e2etts_create reads nothing beyond
                             it and refuses (E2ETTS_EINVAL) a size it does not know: a host built against an older or newer header gets an
                             error instead of garbage fields.  This revision knows exactly one size, e2etts_config_size(). */
  int32_t n_symbols;      /* len(symbols) = 131; the embedding has n_symbols + 1 rows (U/blocks/transformer.py:25) */
  int32_t n_speakers;
  int32_t n_mel;          /* audio.mel.channels */
  int32_t hidden;         /* encoder_hidden == decoder_hidden */
  int32_t enc_layers, dec_layers;
  int32_t n_head;
  int32_t ffn_dim;        /* conv_filter_size */
  int32_t ffn_k1, ffn_k2; /* conv_kernel_size */
  int32_t max_seq_len;
  int32_t dur_layers, dur_kernel, dur_chans;
  int32_t var_layers, var_kernel, var_chans; /* pitch predictor (and the energy predictor unless energy_layers / energy_kernel say otherwise); filter_size */
  int32_t n_bins;
  int32_t postnet_layers, postnet_dim, postnet_kernel;
  int32_t voc_init_ch;
  int32_t voc_stages;
  int32_t voc_up_rate[E2ETTS_MAX_STAGES];
  int32_t voc_up_kernel[E2ETTS_MAX_STAGES];
  int32_t voc_n_kernels;
  int32_t voc_rb_kernel[E2ETTS_MAX_RB_KERNELS];
  int32_t voc_n_dil;
  int32_t voc_rb_dil[E2ETTS_MAX_RB_KERNELS][E2ETTS_MAX_DILATIONS];
  int32_t hop_length;
  int32_t sample_rate;
  int32_t pos_table_rows; /* rows of the regenerated sinusoid table shipped in the blob */
  float f0_mean, f0_std;  /* stats.json "f0" (U/layers.py:152) */
  int32_t voc_resblock;   /* 1: ResBlock1 (V/layers.py:11-40), voc_n_dil pairs; 2: ResBlock2 (V/layers.py:49-66), voc_n_dil = 2 single convs */
  int32_t voc_istft_nfft; /* 0: HiFi-GAN tail (conv_post -> tanh, V/generator.py:49-51); else the iSTFTNet tail (V/generator.py:107-113 +
                             src/tools/stft.py:138-148): conv_post to n_fft + 2 channels, exp / sin, inverse STFT */
  int32_t voc_istft_hop;  /* iSTFT hop; prod(voc_up_rate) * voc_istft_hop == hop_length */
  int32_t block_type;     /* encoder / decoder block: 0 = FFT block (U/blocks/transformer.py:178-189); 1 = Conformer block
                             (U/blocks/conformer.py:171-255): n_head relative-position heads, ffn_dim = hidden x ffn_expansion_factor,
                             ffn_k1 = depthwise kernel size; 2 = Fastformer block (U/blocks/fastformer.py:144-298): additive attention with
                             heads and head size SWAPPED -- FastAttention is built with dim_head = hidden / n_head and runs
                             hidden / n_head heads of size n_head (:152,190-191; hidden 384, n_head 2: 192 heads of size 2); n_head
                             (and dec_n_head) must be 1, 2, 4 or 8 with hidden / n_head <= 512 and hidden <= 1024; FFN conv ffn_k1 -> GELU -> 1 */
  int32_t energy_layers;  /* energy predictor depth / kernel (U/layers.py:92,96: ener_predictor_layers / ener_predictor_kernel); 0 = the pitch */
  int32_t energy_kernel;  /* predictor's (var_layers / var_kernel, U/layers.py:54,58), which is what the shipped model_config.yaml has */
  int32_t dec_n_head;     /* attention heads of the decoder's blocks (decoder_head, U/blocks/transformer.py:105, conformer.py:108); 0 = n_head, which then
                             is both encoder_head and decoder_head */
  int32_t pitch_no_uv;    /* variance_embedding.use_uv == False (U/layers.py:136,155-157): the pitch predictor has ONE output, the bucket is
                             torch.bucketize(prediction * p_control, pitch_bins) and the embedding table has pitch_emb_rows rows; 0 = use_uv */
  int32_t pitch_log2;     /* with use_uv: pitch_quantization == "log" (U/layers.py:148-149): f0 = 2 ** prediction instead of prediction * std + mean */
  int32_t pitch_emb_rows; /* rows of pitch_embedding (U/layers.py:60-63: n_bins with use_uv, f0_bins without); 0 = n_bins */
  int32_t pred_pad_left;  /* variance_predictor.ffn_padding != "SAME" (U/layers.py:400-402,479-481): the three predictors' convolutions are padded
                             (k - 1, 0) -- causal -- instead of ((k - 1) / 2, (k - 1) / 2); 0 = SAME */
  int32_t pitch_frame;    /* variance_embedding.pitch_feature == "frame_level" (U/layers.py:226-257): the pitch predictor and its embedding run on the */
  int32_t energy_frame;   /* length regulator's output ([B, T] rows) instead of on the phonemes; likewise energy_feature.  0 = phoneme_level.  The
                             frame-level feature's pitch_idx / pitch_pred / energy_idx / energy_pred then have T columns: e2etts_acoustic takes NULL
                             for them and e2etts_fetch_tap / e2etts_fetch_tap_i32 hand them out afterwards (T is only known then) */
} e2etts_config;

/* Threading: every entry point takes the engine's internal mutex, so single calls are safe from any thread and distinct engines are
 * independent.  Results that stay RESIDENT between calls (e2etts_acoustic -> e2etts_fetch_mel / e2etts_vocoder(NULL, ...),
 * e2etts_synthesize with pcm_out == NULL -> e2etts_fetch_pcm, taps, the vocoder stream) belong to the last such call: threads sharing one
 * engine serialise those SEQUENCES themselves (the Python binding holds Engine.lock around them). */
typedef struct e2etts_engine e2etts_engine;

/* Library / build identification. */
E2ETTS_API const char* e2etts_version(void);
/* E2ETTS_ABI_VERSION of the header the library was built from, and its sizeof(e2etts_config): what a binding compares its own mirror
 * of the struct with before it calls e2etts_create (e2e_tts_amd/_lib.py: load_library). */
E2ETTS_API int e2etts_abi_version(void);
E2ETTS_API size_t e2etts_config_size(void);

/* Last error message of this engine (or of a failed e2etts_create when engine == NULL). */
E2ETTS_API const char* e2etts_last_error(const e2etts_engine* engine);

/* Replaces: TTS.__init__ model construction + .to(device) (API/utils.py:41-56). */
E2ETTS_API int e2etts_create(int device_id, const e2etts_config* cfg, e2etts_engine** out);
E2ETTS_API void e2etts_destroy(e2etts_engine* engine);

/* Replaces: load_state_dict for both models (API/utils.py:48-49,54-55).  `blob` is the packed weight
 * image (host or device memory; a device image is what a RCCL broadcast from rank 0 leaves behind --
 * SURVEY.md 8(e)); it is copied into engine-owned HBM. */
E2ETTS_API int e2etts_load_weights(e2etts_engine* engine, const void* blob, size_t nbytes);

/* Multi-GPU start-up (no reference line: the reference is single-device): ONE RCCL broadcast of the packed
 * image from rank `root` of `rccl_comm` (an ncclComm_t of the RCCL copy the host process links or has loaded; every rank's
 * engine sits on that communicator's device), issued on the engine's stream straight into engine-owned HBM, then the same
 * binding as e2etts_load_weights.  Collective: every rank of the communicator calls it with the same nbytes; `blob_or_null`
 * (host or device memory) is read on the root only.  RCCL is resolved at the first call (process image, else librccl.so.1 or
 * $E2ETTS_RCCL_LIB); E2ETTS_ESTATE if it cannot be.  Hosts that drive RCCL through torch.distributed broadcast a tensor and
 * call e2etts_load_weights on it instead (e2e_tts_amd/dist.py) -- torch does not expose its ncclComm_t. */
E2ETTS_API int e2etts_load_weights_bcast(e2etts_engine* engine, const void* blob_or_null, size_t nbytes, void* rccl_comm, int root);

/* Replaces: UnsupervisedFastSpeech2.inference (U/model.py:155-194).
 *   ids  [B, L] int64, lens [B] int64 (1 <= lens[b] <= L), speaker [n_spk_ids] int64 with
 *   n_spk_ids == 1 (broadcast, as API/utils.py:133 does) or == B.
 * Outputs (each may be NULL): dur [B, L] fp32 (duration_rounded), mel_lens [B] int64, T_out = max mel
 * length, pitch_idx / energy_idx [B, L] int32 (the bucket indices of U/function.py:178-187 and
 * U/layers.py:169), log_dur [B, L], pitch_pred [B, L, 2] ([B, L] when pitch_no_uv), energy_pred [B, L].
 * mel / mel_post stay resident; read them with e2etts_fetch_mel.  One host sync (for T). */
E2ETTS_API int e2etts_acoustic(e2etts_engine* engine, const int64_t* ids, const int64_t* lens, int B, int L,
                    const int64_t* speaker, int n_spk_ids, float d_control, float p_control, float e_control,
                    float* dur_out, int64_t* mel_lens_out, int* T_out, int32_t* pitch_idx_out, int32_t* energy_idx_out,
                    float* log_dur_out, float* pitch_pred_out, float* energy_pred_out);

/* Same, with per-utterance or per-phoneme duration, pitch and energy controls.  The reference applies the controls by plain tensor
 * arithmetic, so its UnsupervisedFastSpeech2.inference accepts tensors for them and broadcasts:
 *   duration  torch.round(torch.exp(log_d) - 1) * d_control                     (U/layers.py:218-221)
 *   pitch     prediction * control  (use_uv: [B, L, 2] * [B, L, 1], :145; else :157)
 *   energy    prediction * control                                            (U/layers.py:168)
 * Each control is an fp32 array of n values (host or device memory, ordered like every other input: e2etts_order_after):
 *   n == 1      one value for the batch;
 *   n == B      one value per utterance (the reference's [B, 1], or [B, 1, 1] for pitch under use_uv);
 *   n == B * L  one value per phoneme, row-major [B, L] (the reference's [B, L], or [B, L, 1]).
 * A NULL pointer means 1.0 (its count is not read).  Any other count returns E2ETTS_EINVAL before anything is enqueued; the engine stays
 * usable.  The values are used exactly as the scalar entry's are (no validation of values).  Padded phoneme slots are read like any other
 * element, as the reference reads them.  Under use_uv one control scales both the f0 and the uv column, as a [B, L, 1] tensor does.
 * Frame-level features (pitch_frame / energy_frame; an EXTENSION: the reference would need a [B, T] control before T is known): a
 * per-utterance value applies to every frame of its row; a per-phoneme array is expanded along the rounded durations -- frame t of row b
 * takes the control of the phoneme whose repeat span covers it (the length regulator's mapping: int(dur) repeats, running sum), and frames
 * at or beyond mel_lens[b] take control[b, L - 1].  So an array that is uniform per row gives exactly the per-utterance bits.
 * Memory: the controls are copied into an engine-owned workspace of 3 * B * L floats that grows only with B * L; steady state allocates
 * nothing.  Outputs exactly as e2etts_acoustic. */
E2ETTS_API int e2etts_acoustic_ctl(e2etts_engine* engine, const int64_t* ids, const int64_t* lens, int B, int L,
                        const int64_t* speaker, int n_spk_ids, const float* d_control, int n_d, const float* p_control, int n_p,
                        const float* e_control, int n_e, float* dur_out, int64_t* mel_lens_out, int* T_out, int32_t* pitch_idx_out,
                        int32_t* energy_idx_out, float* log_dur_out, float* pitch_pred_out, float* energy_pred_out);

/* The TEACHER-FORCED pass (UnsupervisedFastSpeech2.forward in eval(), U/model.py:95-153: durations, pitch and energy given instead of
 * predicted) is e2etts_acoustic_forced of include/e2etts_forced.h, served by the companion library libe2etts_forced.so on an engine of
 * this library: this header and the symbols libe2etts_hip.so exports are unchanged by it. */

/* Copies of the resident results of the last e2etts_acoustic: mel, mel_post [B, T, n_mel] (either may be NULL). */
E2ETTS_API int e2etts_fetch_mel(e2etts_engine* engine, float* mel, float* mel_post);

/* Debug / parity taps of the last e2etts_acoustic: which = "enc_out" [B, L, H] | "dec_out" [B, T, H]. */
/* taps: "enc_out" [B, L, hidden], "dec_out" [B, T, hidden] (after e2etts_acoustic); "istft_spec_phase" [B, T * prod(voc_up_rate) + 1,
 * n_fft + 2] = exp / sin heads of the iSTFTNet generator (reference iSTFT.forward's return values), after a vocoder call. */
E2ETTS_API int e2etts_fetch_tap(e2etts_engine* engine, const char* which, float* out, size_t n_floats);
/* after e2etts_acoustic_forced (include/e2etts_forced.h) also "pitch_target", "energy_target", "dec_in" (see there; E2ETTS_ESTATE after any other
 * acoustic pass). */
/* more taps of the last e2etts_acoustic, at the level the feature lives at (N = L for phoneme_level, T for frame_level):
 * e2etts_fetch_tap: "pitch_pred" [B, N, 2] ([B, N] when pitch_no_uv), "energy_pred" [B, N]; e2etts_fetch_tap_i32: "pitch_idx", "energy_idx" [B, N]. */
E2ETTS_API int e2etts_fetch_tap_i32(e2etts_engine* engine, const char* which, int32_t* out, size_t n_values);

/* Replaces: HifiGan.forward (V/generator.py:37-53) on mel [B, n_mel, T] (the reference layout,
 * channels-first, as API/utils.py:144 passes it) or, when mel == NULL, on the resident mel_post of the
 * last e2etts_acoustic.  Outputs (each may be NULL): wav [B, T*hop] fp32 in (-1, 1);
 * pcm [B, T*hop] int16 = trunc(wav * 32768) as TTS.combine_audio computes it (API/utils.py:111-117). */
E2ETTS_API int e2etts_vocoder(e2etts_engine* engine, const float* mel_bct, int B, int T, float* wav_out, int16_t* pcm_out);

/* Same, mel given channels-last [B, T, n_mel] (the engine's native layout; no transpose). */
E2ETTS_API int e2etts_vocoder_btc(e2etts_engine* engine, const float* mel_btc, int B, int T, float* wav_out, int16_t* pcm_out);

/* Replaces one iteration of the TTS.inference batch loop (API/utils.py:130-148): acoustic -> vocoder.
 * pcm_out [B, T*hop] int16 (rows padded to the batch maximum; valid samples of row b = mel_lens[b]*hop),
 * mel_lens_out [B]. T_out receives T.  pcm_capacity = number of int16 the caller's buffer holds; if it is
 * too small E2ETTS_EINVAL is returned with T_out set, and the result can be fetched with e2etts_fetch_pcm. */
E2ETTS_API int e2etts_synthesize(e2etts_engine* engine, const int64_t* ids, const int64_t* lens, int B, int L,
                      const int64_t* speaker, int n_spk_ids, float d_control, float p_control, float e_control,
                      int16_t* pcm_out, size_t pcm_capacity, int64_t* mel_lens_out, int* T_out);
/* Same, with the array controls of e2etts_acoustic_ctl (same counts, memory and frame-level rule); a server batches requests that
 * carry different speakers (n_spk_ids == B) and different controls into one call. */
E2ETTS_API int e2etts_synthesize_ctl(e2etts_engine* engine, const int64_t* ids, const int64_t* lens, int B, int L,
                          const int64_t* speaker, int n_spk_ids, const float* d_control, int n_d, const float* p_control, int n_p,
                          const float* e_control, int n_e, int16_t* pcm_out, size_t pcm_capacity, int64_t* mel_lens_out, int* T_out);
E2ETTS_API int e2etts_fetch_pcm(e2etts_engine* engine, int16_t* pcm_out, size_t capacity);
E2ETTS_API int e2etts_fetch_wav(e2etts_engine* engine, float* wav_out, size_t capacity);

/* Long-form / streaming vocoder (BASELINE config 5).  The mel stream of B parallel utterances is pushed in chunks of any
 * size, channels-last [B, n, n_mel] (host or device memory); the engine keeps the receptive-field halo (returned by
 * _begin, in frames; 15 for the default HiFi-GAN V1) and the not-yet-emittable tail internally, so HBM use is bounded by
 * the chunk size, and the concatenated output is bit-identical to one e2etts_vocoder call on the whole mel.
 *   _begin(B)                      -> halo in frames (>= 0) or a negative error
 *   _push(mel, n, last, &n_emit)   -> enqueues the vocoder on [context | pending | new] and RETURNS; n_emit frames became final
 *   _fetch(wav, pcm, capacity)     -> waits for the OLDEST unfetched push that emitted frames and copies its n_emit * hop samples per
 *                                     utterance, [B, n_emit * hop] compact
 * Up to two emitting pushes may await their fetch (a third fails with E2ETTS_ESTATE), so a caller either alternates push / fetch
 * as before, or keeps the GPU busy across chunk boundaries: push(i + 1), then fetch(i) -- chunk i's samples travel to the host on a
 * copy stream while chunk i + 1 computes.  Each in-flight chunk has its own output buffers; the resident one-shot result
 * (e2etts_fetch_wav / _pcm) is not touched by the stream.  A chunk in pageable host memory has been consumed when _push returns; one in
 * device memory, or in host memory the caller pinned, must stay valid until the fetch of that push (or e2etts_sync) returns.  Errors of
 * the enqueued work surface at the fetch.
 *
 * _begin_denoised(B, strength, &delay) opens a DENOISED stream (vocoder-bias denoiser, below): the concatenated pieces are bit-identical to
 * e2etts_denoise(wav = e2etts_vocoder(whole mel), n_valid = T * hop_length for every row, strength), as fp32 and as saturated int16, in every
 * vocoder precision, for any chunking and with two chunks in flight.  The reference's reflect padding happens at the true start and the
 * true end of the stream only, never at a chunk border; a stream of at most filter_length / 2 samples in total is copied through unchanged
 * (e2etts_denoise's rule for a row that cannot be reflected); strength 0 is allowed and equals e2etts_denoise(..., 0).
 * It returns the vocoder's halo like _begin, and *delay = C = ceil((filter_length - hop) / hop_length) (3 for 1024 / 256 at hop_length 256):
 * the denoiser's frames reach filter_length - hop samples beyond a sample, so every window carries C more mel frames of context per side
 * and emitted frames lag pushed ones by halo + C.  The denoiser runs on the window's waveform, per slot, in a workspace of the slot's own
 * (bounded by the chunk): nothing of it is carried between chunks.  _push and _fetch are used as above; n_emit counts frames whose
 * DENOISED samples became final and _fetch hands those out.  One-shot calls (e2etts_denoise included) between the steps do not disturb it.
 * Errors: E2ETTS_ESTATE without bases or bias; E2ETTS_EINVAL for a negative strength, for a denoiser hop that does not divide hop_length and
 * for the iSTFT tail (voc_istft_nfft != 0: its tap buffers are engine-wide).  While a denoised stream is open and unfinished (until its last
 * chunk is fetched, or the next _begin / _begin_denoised, which abandons it) e2etts_denoiser_load, _set_bias and _calibrate return
 * E2ETTS_ESTATE: chunks in flight read the bases and the bias.  e2etts_load_weights closes it like any stream.  _begin itself is
 * unchanged: a stream opened with it is never denoised, whatever e2etts_set_denoise says. */
E2ETTS_API int e2etts_vocoder_stream_begin(e2etts_engine* engine, int B);
E2ETTS_API int e2etts_vocoder_stream_begin_denoised(e2etts_engine* engine, int B, float strength, int* delay_frames_out);
E2ETTS_API int e2etts_vocoder_stream_push(e2etts_engine* engine, const float* mel_btc, int n_frames, int last, int* n_frames_out);
E2ETTS_API int e2etts_vocoder_stream_fetch(e2etts_engine* engine, float* wav_out, int16_t* pcm_out, size_t capacity);

/* Replaces: audio_speed_change (API/utils.py:163-172), which shells out to ffmpeg's `atempo` filter: tempo change without pitch change
 * of an int16 PCM signal (host or device memory), on the GPU.  ffmpeg is not part of this build: the kernel is waveform-similarity
 * overlap-add (WSOLA), the algorithm family behind that filter, restated from the published method -- PARITY UNPINNED against the
 * reference; it mirrors e2e_tts_amd/api.py: time_stretch_wsola (40 ms frames, 50 % overlap, +-10 ms search, float64) step for step.
 * n_out receives round(n_in / speed); with pcm_out == NULL the call only reports that size.  speed in [0.25, 4].  (The Python mirror's
 * DEFAULT for speed != 1 is the model's own duration control -- no post-processing at all; this entry serves speed_mode="wsola".) */
/* `speed` is a double: n_out and the per-frame analysis positions are computed from it exactly as the Python mirror computes them from
 * its float (a C float 0.8f is 0.800000012, which rounds n_in / speed the other way at exact .5 ties).  sample_rate in [4000, 96000]: the
 * kernel keeps one analysis frame, its search region and three work frames in LDS (0.18 s of float64 samples <= 160 KB). */
E2ETTS_API int e2etts_tempo(e2etts_engine* engine, const int16_t* pcm_in, size_t n_in, double speed, int sample_rate, int16_t* pcm_out,
                 size_t capacity, size_t* n_out);

/* Replaces: Denoiser (V/denoiser.py:156-186) and the STFT it is built on (:55-153) -- the usual post-filter of a GAN vocoder: the
 * magnitude spectrum of what the vocoder makes of an all-zero mel (its "bias": a constant hum) is subtracted, scaled by `strength`, from
 * every STFT frame of an utterance, the result is clamped at 0 and inverted with the utterance's own phases.
 * Arithmetic: both transforms are convolutions with the reference's windowed bases, computed in EXACT fp32 in every precision mode
 * (csrc/denoiser.hip); mag_d * cos / sin(atan2(im, re)) is evaluated as (re, im) * mag_d / mag (0 where mag == 0).
 *
 * e2etts_denoiser_load: the two bases in the reference's own buffer layout, [filter_length + 2, filter_length] fp32
 *   (STFT.forward_basis / inverse_basis squeezed; e2e_tts_amd/denoiser.py: stft_bases builds them as the reference does), host or device
 *   memory, read with blocking copies (a device buffer must be complete: e2etts_order_after does not cover this call).  win_sq: the squared,
 *   centre-padded window [filter_length] fp32 of the sum-square envelope (:43-46), NULL = periodic Hann of filter_length points (in
 *   float64, as the reference's envelope takes it).  The bases are NOT part of the weight blob: they, and the bias, stay across
 *   e2etts_load_weights (load another vocoder: calibrate again); loading bases drops the bias.
 *   Served: filter_length = hop * n_overlap with n_overlap in {2, 4, 8}, hop a multiple of 32, hop <= 1024; anything else returns
 *   E2ETTS_EINVAL (numbers in the message) before any launch.
 * e2etts_denoiser_set_bias: an explicit bias spectrum [filter_length / 2 + 1] (n_bins must be that number).
 * e2etts_denoiser_calibrate: the reference's constructor (:165-179): the engine's own vocoder, in its current precision, on one utterance
 *   of T mel frames [T, n_mel] channels-last (NULL = zeros; T = 88 is the reference's mode = 'zeros', for mode = 'normal' pass a random
 *   mel); the magnitudes of frame 0 of its transform become the bias, and are copied to bias_out when given.  T * hop_length must be a
 *   multiple of the denoiser's hop above filter_length / 2.  Resident results (the wav / PCM of the last vocoder or synthesize call,
 *   taps) are left as they were.
 * e2etts_denoise: wav_in [B, n] fp32 (NULL = the resident wav of the last e2etts_vocoder / e2etts_synthesize call; B and n must then
 *   be its shape), n_valid [B] int64 valid samples per row (NULL = n for every row).  Each row is transformed ALONE: reflect-padded at its
 *   own end, as the reference run on that row trimmed to its length.  Every n_valid[b] must lie in [0, n] and be a multiple of the
 *   denoiser's hop (vocoder output always is), else E2ETTS_EINVAL.  Rows with n_valid[b] <= filter_length / 2 cannot be reflect-padded --
 *   the reference raises there -- and are COPIED THROUGH unchanged, so that one two-frame utterance does not fail a batch.  Samples at
 *   or past n_valid[b] come out 0.  Outputs (one may be NULL): wav_out [B, n] fp32; pcm_out [B, n] int16 = trunc(v * 32768) SATURATED to
 *   [-32768, 32767]: a denoised sample can leave (-1, 1), where the reference's astype("int16") is undefined.  strength 0 reconstructs
 *   the input (to fp32 rounding).  E2ETTS_ESTATE when no bases or no bias are loaded, or wav_in == NULL with no resident wav.
 *   The resident wav / PCM are not modified.
 * e2etts_set_denoise: strength > 0 (needs bases and bias: E2ETTS_ESTATE otherwise) makes e2etts_synthesize[_ctl] denoise each row's valid
 *   samples (mel_lens[b] * hop_length; hop_length must be a multiple of the denoiser's hop) before the int16 conversion: its PCM, and the
 *   PCM e2etts_fetch_pcm hands out, are exactly e2etts_denoise of the resident wav (which e2etts_fetch_wav still returns as the vocoder
 *   left it); samples past a row's valid ones are 0.  0 (the default) leaves every path as it is without a denoiser.  e2etts_vocoder[_btc]
 *   and a stream opened with e2etts_vocoder_stream_begin are never denoised; e2etts_vocoder_stream_begin_denoised (above) opens a stream
 *   that is, with a strength of its own. */
E2ETTS_API int e2etts_denoiser_load(e2etts_engine* engine, const float* fwd_basis, const float* inv_basis, const float* win_sq_or_null,
                                    int filter_length, int hop);
E2ETTS_API int e2etts_denoiser_set_bias(e2etts_engine* engine, const float* bias, int n_bins);
E2ETTS_API int e2etts_denoiser_calibrate(e2etts_engine* engine, const float* mel_btc_or_null, int T, float* bias_out_or_null);
E2ETTS_API int e2etts_denoise(e2etts_engine* engine, const float* wav_in_or_null, const int64_t* n_valid_or_null, int B, int64_t n,
                              float strength, float* wav_out, int16_t* pcm_out);
E2ETTS_API int e2etts_set_denoise(e2etts_engine* engine, float strength);

/* Arithmetic of the convolutions / projections of (a) the vocoder and (b) the decoder + mel_linear + postnet.
 * The encoder and the variance adaptor are always exact fp32: the duration / pitch / energy decisions taken there
 * must be bit-exact, and nothing downstream of the length regulator is discrete.
 * E2ETTS_PRECISION_FP32 (default -- the reference's arithmetic): v_mfma_f32_32x32x2_f32, an exact fp32 FMA chain.
 * E2ETTS_PRECISION_BF16X3 (opt-in fast mode, 2.6 x the throughput): every fp32 operand is split into bf16 hi + lo and the
 * product keeps hi*hi + hi*lo + lo*hi on the bf16 matrix pipe with fp32 accumulation -- ~16 significant bits per operand;
 * measured against the reference's own outputs (bench.py `split_precision_mode`): wav mean-L1 1.1e-6 .. 1.3e-6 (fp32: 1.3e-7;
 * plain bf16: 5e-4; parity bar: 1e-4), int16 PCM within 1 LSB on 100 % of samples, discrete outputs untouched. */
#define E2ETTS_PRECISION_FP32 0
#define E2ETTS_PRECISION_BF16X3 1
#define E2ETTS_PRECISION_BF16 2 /* vocoder only: hi x hi product alone (plain bf16 operands, fp32 accumulation): the arithmetic
                                   BASELINE config 5 (long-form streaming) names; waveform error ~5e-4, above the fp32 bar */
/* E2ETTS_PRECISION_BF16_ACT (vocoder only): the arithmetic of the reference's HifiGan cast with .bfloat16() and fed a bf16 mel
 * (V/generator.py:37-53, V/layers.py:33-40 and 59-64).  Every tensor the vocoder keeps in HBM is bf16 [B, N, C]; each convolution
 * accumulates in fp32 (bf16 products) and rounds its output once; each elementwise step is computed in fp32 on bf16 values and rounded to
 * nearest-even:
 *   input            mel staged as bf16(mel)
 *   conv_pre         x = bf16(acc + b)                                                    (generator.py:38)
 *   per upsampler    x = bf16(lrelu_0.1(x)); x = bf16(acc + b) (ConvTranspose1d; the polyphase form has the same products)   (:40-41)
 *   ResBlock1 pair   xt = bf16(lrelu(x)); xt = bf16(c1 + b1); xt = bf16(lrelu(xt)); xt = bf16(c2 + b2); x = bf16(xt + x)  (layers.py:35-39)
 *   ResBlock2 step   xt = bf16(lrelu(x)); xt = bf16(c + b); x = bf16(xt + x)               (layers.py:62-64)
 *   stage sum        xs = rb_0; xs = bf16(xs + rb_j) in j order; x = bf16(xs / num_kernels)   (generator.py:45-48)
 *   tail             x = bf16(lrelu_0.01(x)); y = bf16(conv_post + b); wav = bf16(tanh(y))   (:49-51)
 *   PCM              trunc(wav * 32768) of the rounded wav
 * (note the double rounding bf16(lrelu(bf16(c1 + b1))): mode 2 rounds once, bf16(lrelu(c1 + b1))).  Weights: bf16 of the fp32 weight-norm
 * fold (mode 2's images); biases and conv_post's weights rounded to bf16 once, at load.  Difference from the reference's module: it
 * evaluates the weight norm in bf16 from bf16 weight_g / weight_v (two roundings); the engine rounds the fp32 fold once.  Accumulation
 * order differs from torch's CPU kernels, so single outputs may differ by one bf16 ulp, and such flips spread through later layers.
 * Served: the HiFi-GAN tail, ResBlock1 or ResBlock2, every vocoder width a multiple of 32 (>= 32).  e2etts_set_precision returns
 * E2ETTS_EINVAL up front for the iSTFT tail, narrower widths, and this value as the decoder precision.  Ragged batches: the vocoder
 * computes the padded rows (valid samples are the same with ragged on or off).  All fusion levels give the same bits. */
#define E2ETTS_PRECISION_BF16_ACT 3
/* E2ETTS_PRECISION_FP16_ACT (vocoder only): the arithmetic of the reference's HifiGan cast with .half() and fed an fp16 mel.  It is the
 * table above with "bf16" read as IEEE binary16 (fp16): every tensor the vocoder keeps in HBM is fp16 [B, N, C]; each convolution multiplies
 * fp16 operands on the fp16 MFMA (v_mfma_f32_32x32x16_f16: the bf16 instruction's shape and rate), accumulates in fp32, adds the bias in
 * fp32 and rounds once; each elementwise step is computed in fp32 on fp16 values and rounded once:
 *   input            mel staged as fp16(mel)
 *   conv_pre         x = fp16(acc + b)
 *   per upsampler    x = fp16(lrelu_0.1(x)); x = fp16(acc + b)
 *   ResBlock1 pair   xt = fp16(lrelu(x)); xt = fp16(c1 + b1); xt = fp16(lrelu(xt)); xt = fp16(c2 + b2); x = fp16(xt + x)
 *   ResBlock2 step   xt = fp16(lrelu(x)); xt = fp16(c + b); x = fp16(xt + x)
 *   stage sum        xs = rb_0; xs = fp16(xs + rb_j) in j order; x = fp16(xs / num_kernels)
 *   tail             x = fp16(lrelu_0.01(x)); y = fp16(conv_post + b); wav = fp16(tanh(y))
 *   PCM              trunc(wav * 32768) of the rounded wav
 * (the double rounding fp16(lrelu(fp16(c1 + b1))) is kept).  Conversions: round to nearest-even; overflow goes to infinity, as torch's
 * cast does; subnormal results are kept (the fp16 denormal mode is "preserve"); a plain _Float16 cast (v_cvt_pk_f16_f32), never a
 * round-toward-zero pack.  Subnormal MFMA operands are read as they are, not as zero (measured on the MI355X with
 * tools/mfma_f16_subnormal.hip: 2^-20 x 2^10 gives 2^-10 from either operand, sixteen products 2^-24 x 2^12 sum to 2^-8), as torch's CPU kernels do.
 * Weights: fp16 of the fp32 weight-norm fold, rounded ONCE from the fp32 weights of the blob (not from the bf16 hi + lo images); biases
 * and conv_post's weights rounded to fp16 once.  These images and copies are built when the mode is first selected: an engine that never
 * selects it owns no more HBM than before.  Difference from the reference's module: it evaluates the weight norm in fp16 from fp16
 * weight_g / weight_v (several roundings); the engine rounds the fp32 fold once.  Accumulation order differs from torch's CPU kernels, so
 * single outputs may differ by one fp16 ulp, and such flips spread through later layers.  Against the fp32 result the waveform lies ~1e-4
 * mean-L1 (bf16_act: 6e-4 .. 9e-4) at the same bytes and matrix rate.
 * Served geometries, refusals (E2ETTS_EINVAL up front for the iSTFT tail, narrower widths, and this value as the decoder precision),
 * ragged batches (padded rows computed), streaming and fusion levels: exactly as E2ETTS_PRECISION_BF16_ACT. */
#define E2ETTS_PRECISION_FP16_ACT 4
E2ETTS_API int e2etts_set_precision(e2etts_engine* engine, int vocoder_precision, int decoder_precision);

/* Ragged batches (default on).  e2etts_synthesize hands back, per utterance, only mel_lens[b] * hop valid samples; with
 * ragged != 0 it therefore skips, layer by layer, the rows of shorter utterances that no valid sample depends on (rows past
 * mel_len + the receptive field of the layers still to come, stage by stage), instead of computing the whole padded batch as the reference does.  Valid samples are
 * bit-identical either way; what lies beyond them in the padded PCM rows is then unspecified.  e2etts_acoustic /
 * e2etts_vocoder always compute the full padded tensors (their padded rows match the reference's).
 * The frame level (decoder, postnet, vocoder) is skipped from the mel lengths the engine computes itself; the phoneme level (encoder,
 * predictors) additionally when `lens` is HOST memory (the launch grids are built from the lengths on the host; with `lens` in device
 * memory the phoneme level computes the padded batch -- same results).  Batches of up to 64 utterances launch grids without idle
 * workgroups; larger ones still skip the rows but keep the padded grid.  With vocoder precision E2ETTS_PRECISION_BF16_ACT or _FP16_ACT the vocoder
 * computes the padded rows in either case (the decoder and postnet still skip them); valid samples are identical with ragged on or off. */
E2ETTS_API int e2etts_set_ragged(e2etts_engine* engine, int enable);

/* Test hook for ragged mode, present only in the TEST build of the library (compiled with -DE2ETTS_TEST_HOOKS into
 * libe2etts_hip_test.so; the product library libe2etts_hip.so does not export it): overwrite the activation workspaces (not the
 * weights, not the index buffers) with a large finite pattern (every byte 0x4B: 1.3e7 as fp32) and forget the resident results, so
 * that a test can show that no valid sample of the next call depends on what an earlier call left in the rows that ragged compute
 * skips. */
#ifdef E2ETTS_TEST_HOOKS
E2ETTS_API int e2etts_debug_poison_workspace(e2etts_engine* engine);
#endif

/* Fused ResBlocks (bf16 modes).  level 1: each (conv k, dilation d -> leaky ReLU -> conv k -> + x) pair of HiFi-GAN's ResBlock1
 * (reference V/layers.py:33-40) at 32 / 64 / 128 / 256 channels runs as ONE kernel whose intermediate stays in LDS.  level 2
 * (default): additionally a whole kernel-size-3 ResBlock1 (its three pairs) at 32 / 64 channels runs as one kernel whose residual
 * stream stays in registers.  level 0: two convolution launches per pair.  All three produce bit-identical output. */
E2ETTS_API int e2etts_set_fused_resblocks(e2etts_engine* engine, int level);

/* Per-kernel-class timing with HIP events on the engine's stream (bench.py roofline leg).
 * enable != 0 starts recording (and clears counters); e2etts_profile_read fills up to `cap` records. */
typedef struct e2etts_kernel_stat {
  char name[48];
  uint64_t launches;
  double ms;      /* sum of launch durations */
  double flops;   /* algorithmic FLOPs (2 x MAC) of those launches */
  double bytes;   /* algorithmic bytes (operands read once + result written once) */
} e2etts_kernel_stat;
/* Restrict the event bracketing to one kernel class (NULL or "": all classes).  Two hipEventRecord per launch cost ~8 us; with ~155
 * launches per step that is 2 % of a step, so a timed region that only needs the dominant kernel's duration brackets that class alone. */
E2ETTS_API int e2etts_profile_filter(e2etts_engine* engine, const char* kernel_class);
E2ETTS_API int e2etts_profile_enable(e2etts_engine* engine, int enable);
E2ETTS_API int e2etts_profile_read(e2etts_engine* engine, e2etts_kernel_stat* out, int cap);

/* Bytes of HBM currently owned by the engine (weights + workspace). */
E2ETTS_API size_t e2etts_device_bytes(const e2etts_engine* engine);

/* The engine's stream as a hipStream_t cast to void* (so a caller can order its own work after ours). */
E2ETTS_API void* e2etts_stream(e2etts_engine* engine);
/* Orders everything the engine does from now on after the work queued so far on `caller_stream` (a hipStream_t cast to
 * void*; NULL = the legacy default stream): an event recorded there, waited for on the engine's stream.  See "STREAM
 * ORDERING" at the top.  Costs two API calls, no host synchronisation. */
E2ETTS_API int e2etts_order_after(e2etts_engine* engine, void* caller_stream);
E2ETTS_API int e2etts_sync(e2etts_engine* engine);

#ifdef __cplusplus
}
#endif
#endif /* E2ETTS_H */
