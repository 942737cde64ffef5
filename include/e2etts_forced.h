/*
 * e2etts_forced.h -- C ABI of the teacher-forced acoustic pass, served by the companion library libe2etts_forced.so.
 *
 * The main library's ABI (include/e2etts.h: its entry points, e2etts_config, E2ETTS_ABI_VERSION) is frozen, so the pass has a header and a
 * library of its own, like the aligner, the mel front-end and the resampler.  Unlike those it has no handle: it works ON AN ENGINE of the
 * main library (e2etts_create of libe2etts_hip.so), whose resident results, taps, stream, mutex and error message it shares -- after a
 * call, e2etts_fetch_mel, e2etts_fetch_tap, e2etts_vocoder(NULL, ...) and e2etts_last_error of the main library serve it unchanged.  The
 * library is linked from the same objects as the main one (the engine included) and exports the entry points below and nothing else; both
 * must come from ONE source revision: e2etts_forced_engine_version() is the e2etts_version() string of the engine code inside this
 * library, and a host refuses the pair when it differs from the main library's (the Python binding does at load: e2e_tts_amd/forced.py).
 * That string does not record -DE2ETTS_TEST_HOOKS; the macro adds functions only and never changes the engine's layout.
 * Conventions (return codes, host or device pointers, stream ordering) are those of include/e2etts.h.
 * Paths: U/ = e2e_tts/models/acoustic/unsupervised_fastspeech2/ of the reference.
 */
#ifndef E2ETTS_FORCED_H
#define E2ETTS_FORCED_H

#include "e2etts.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define E2ETTS_FORCED_API __attribute__((visibility("default")))
#else
#define E2ETTS_FORCED_API
#endif

/* bumped whenever e2etts_forced's layout or a signature below changes */
#define E2ETTS_FORCED_ABI_VERSION 1

E2ETTS_FORCED_API const char* e2etts_forced_version(void);          /* this library's own build marker */
E2ETTS_FORCED_API int e2etts_forced_abi_version(void);
E2ETTS_FORCED_API const char* e2etts_forced_engine_version(void);   /* e2etts_version() of the engine code linked into this library */

/* Replaces: UnsupervisedFastSpeech2.forward in eval() (U/model.py:95-153), the TEACHER-FORCED pass of VarianceAdaptor.forward with
 * attn_prior given (U/layers.py:175-272) that generate_mel (src/tools/tools_for_data.py:216-256) runs for the ground-truth-aligned mels:
 * durations come from the aligner's MAS, the pitch / energy embeddings from the recording's targets instead of the predictors, and the
 * phonemes are expanded either by the soft alignment map (step < binarization_start_steps) or by the length regulator.
 * Every member is optional (NULL) and, like every pointer of this ABI, host or device memory; with ALL of them NULL the call IS
 * e2etts_acoustic_ctl, bit for bit.  No control is applied to a target; a feature without a target is embedded from prediction * control.
 *   durations  [B, L] fp32 holding integers >= 0 (duration_rounded = attn_hard.sum(2), U/layers.py:202-214).  NULL: the predicted ones.
 *              In HOST memory they are validated (negative, non-integral and non-finite values are refused, E2ETTS_EINVAL).  In DEVICE
 *              memory the kernel that scans them clamps instead: NaN and negative values count as 0, a fraction is truncated, a value above
 *              2^20 counts as 2^20 (the predicted path's cap), and every slot l >= lens[b] counts as 0 -- dur_out receives the clamped values.
 *   attn_soft  [B, T, L] fp32 with T and mel_lens [B] int64 (1 <= mel_lens[b] <= T): selects the SOFT expansion
 *              x[b, t, :] = sum_{l < lens[b]} attn_soft[b, t, l] * x[b, l, :] (torch.bmm, U/layers.py:244-245) in exact fp32; columns
 *              l >= lens[b] are not read (the map is 0 there).  T and mel_lens are returned as given: no host synchronisation.  A device
 *              map is read where it lies.  T is checked against the position tables exactly as the predicted path checks its own.
 *              Without attn_soft the length regulator runs on the durations and mel_lens / T are their sums, as in e2etts_acoustic.
 *   pitch      use_uv models: f0 AND uv (normalised f0 -- log2 f0 under pitch_log2 -- and the 0 / 1 unvoiced mark); pitch_no_uv models:
 *              `pitch`.  Giving the kind the model does not have, or one of f0 / uv alone, is E2ETTS_EINVAL.
 *   energy
 *   pitch_frames / energy_frames: 0 = the target is at the MODEL's level ([B, L] for a phoneme_level feature, [B, T] for a frame_level
 *              one); 1 = it is frame-resolved [B, T].  A frame-resolved target of a phoneme_level feature is averaged per phoneme over
 *              `durations` (required then) as get_phoneme_level / frame2phoneme do (U/function.py:155-175): the mean of frames
 *              [pos, pos + d), 0 for d == 0, numpy's float32 summation order; the reference works IN PLACE on the frame array, so a mean
 *              written to slot i > pos is what a later phoneme reads there, and that is reproduced; uv becomes 1 only where its mean is
 *              exactly 1.0 (U/layers.py:230-231).  The row sums of `durations` must not exceed T.  Rows of [B, T] targets have T columns
 *              (T must be given); in hard mode a frame_level feature reads its first max(mel_lens) columns, which must not exceed T.
 * Ragged batches: generate_mel keeps the valid frames only, so this entry follows e2etts_set_ragged as e2etts_synthesize does (default on:
 * rows of mel / mel_post / dec_in at or past mel_lens[b] are unspecified; valid rows are bit-identical either way); a frame_level feature
 * reads every row of the expanded tensor, so the soft expansion computes them all for such a model.
 * Results are resident exactly as after e2etts_acoustic (e2etts_fetch_mel, e2etts_vocoder(NULL, ...), the taps; pitch_pred / energy_pred of
 * a feature that has a target are the predictor's outputs BEFORE any control, as the reference returns them).  Further taps after this
 * call (e2etts_fetch_tap): "pitch_target" [B, N, 2] (f0, uv; [B, N] when pitch_no_uv) and "energy_target" [B, N] -- the targets at the
 * model's level as embedded (E2ETTS_ESTATE for a feature that had none) --, "dec_in" [B, T, hidden]: the decoder's input, positions included.
 * The decoder works in place, so every call of this entry keeps "dec_in" as one device-to-device copy of B * T * hidden floats on the engine's
 * stream (38 MB read and 38 MB written at B 32, T 768, hidden 384), whether or not the tap is fetched.
 * ABI: e2etts_forced carries its own struct_size (e2etts_config's rule: nothing beyond it is read, an unknown size is E2ETTS_EINVAL; this
 * revision knows one size); include/e2etts.h, its E2ETTS_ABI_VERSION and the exports of libe2etts_hip.so are untouched. */
typedef struct e2etts_forced {
  uint32_t struct_size;     /* = sizeof(e2etts_forced) of the header the caller was compiled against */
  int32_t T;                /* columns of attn_soft's rows and of every [B, T] target; 0 when neither is given */
  const float* durations;   /* [B, L] */
  const float* attn_soft;   /* [B, T, L] */
  const int64_t* mel_lens;  /* [B], with attn_soft */
  const float* f0;          /* use_uv */
  const float* uv;
  const float* pitch;       /* pitch_no_uv */
  const float* energy;
  int32_t pitch_frames;     /* 1: the pitch target(s) are frame-resolved [B, T] */
  int32_t energy_frames;    /* 1: the energy target is frame-resolved [B, T] */
} e2etts_forced;
E2ETTS_FORCED_API int e2etts_acoustic_forced(e2etts_engine* engine, const int64_t* ids, const int64_t* lens, int B, int L,
                           const int64_t* speaker, int n_spk_ids, const float* d_control, int n_d, const float* p_control, int n_p,
                           const float* e_control, int n_e, const e2etts_forced* forced, float* dur_out, int64_t* mel_lens_out, int* T_out,
                           int32_t* pitch_idx_out, int32_t* energy_idx_out, float* log_dur_out, float* pitch_pred_out, float* energy_pred_out);

#ifdef __cplusplus
}
#endif
#endif /* E2ETTS_FORCED_H */
