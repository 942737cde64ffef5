"""numpy restatement of the reference's TEACHER-FORCED forward: UnsupervisedFastSpeech2.forward in eval() (U/model.py:95-153) around
VarianceAdaptor.forward with attn_prior given (U/layers.py:175-272), on top of oracle.ref_numpy.AcousticOracle (encoder, predictors,
decoder, postnet).  The aligner and the monotonic alignment search have a restatement of their own (tests/aligner_ref.py); here the soft
map and the MAS durations are INPUTS, as the engine's e2etts_acoustic_forced takes them.

Quirks restated as they run:
  * frame2phoneme (U/function.py:155-166) works IN PLACE on the frame array: the mean of phoneme i is written to slot i, and a later
    phoneme whose frames start before its own index (possible only after a zero duration) reads that mean instead of the frame;
  * np.mean of a float32 slice keeps numpy's float32 pairwise summation (this file calls np.mean on float32 slices for that reason);
  * uv becomes 1 only where the phoneme mean is exactly 1.0 (U/layers.py:230-231);
  * a target is embedded without any control, the predictors still run and their outputs are returned (before the control when the
    feature has a target);
  * step < binarization_start_steps: x = attn_soft @ x on EVERY row, mel_lens as given; else the length regulator padded to max_mel_len.
"""
from __future__ import annotations

import numpy as np

from oracle.ref_numpy import AcousticOracle, get_mask_from_lengths, linear


def frame2phoneme(duration, prosody):
    """U/function.py:155-166, statement for statement; ``prosody`` (float32 [T]) is overwritten, as there."""
    pos = 0
    for i, d in enumerate(duration):
        d = int(d)
        if d > 0:
            prosody[i] = np.mean(prosody[pos: pos + d])
        else:
            prosody[i] = 0
        pos += d
    return prosody[: len(duration)]


def get_phoneme_level(frame_feature, src_len, duration, L=None):
    """U/function.py:169-175: per row frame2phoneme(dur[:len], var), zero-padded (pad_1D) -- to L columns here."""
    frame_feature = np.array(frame_feature, dtype=np.float32, copy=True)
    dur = np.asarray(duration).astype(np.int32)
    rows = [frame2phoneme(dur[b, :int(n)], frame_feature[b]) for b, n in enumerate(np.asarray(src_len))]
    width = max(len(r) for r in rows) if L is None else L
    out = np.zeros((len(rows), width), np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


class ForcedOracle(AcousticOracle):
    def pitch_embedding_forced(self, x, target, control):
        """U/layers.py:136-162 with a target: -> (prediction as returned, idx, embedding)."""
        if target is None:
            return self.pitch_embedding(x, control)
        dt = self.dt
        ve = self.fs["variance"]["variance_embedding"]
        if not ve["use_uv"]:
            pred = self.variance_predictor("pitch", x)[..., 0]
            idx = np.searchsorted(self.sd["variance_adaptor.pitch_bins"], np.asarray(target, self.dt), side="left").astype(np.int64)
            return pred, idx, self.sd["variance_adaptor.pitch_embedding.weight"][idx]
        pred = self.variance_predictor("pitch", x)
        f0, uv = np.asarray(target["f0"], self.dt), np.asarray(target["uv"], self.dt)
        if ve["pitch_quantization"] == "log":
            f0_denorm = np.power(dt(2), f0).astype(self.dt)
        else:
            f0_denorm = f0 * dt(self.stats["f0"]["std"]) + dt(self.stats["f0"]["mean"])
        f0_denorm = np.where(uv > 0, dt(0), f0_denorm)
        idx = self.f0_to_coarse(f0_denorm)
        return pred, idx, self.sd["variance_adaptor.pitch_embedding.weight"][idx]

    def energy_embedding_forced(self, x, target, control):
        if target is None:
            return self.energy_embedding(x, control)
        pred = self.variance_predictor("energy", x)[..., 0]
        idx = np.searchsorted(self.sd["variance_adaptor.energy_bins"], np.asarray(target, self.dt), side="left").astype(np.int64)
        return pred, idx, self.sd["variance_adaptor.energy_embedding.weight"][idx]

    def forward(self, speakers, ids, lens, mel_lens, dur, attn_soft, p_targets=None, e_targets=None, soft=True, p_control=1.0, e_control=1.0,
                max_mel_len=None):
        """speakers [B]; dur [B, L] (MAS durations); attn_soft [B, T, L]; p_targets: {"f0", "uv"} of [B, T] arrays (use_uv) or one [B, T]
        array, or None; e_targets [B, T] or None.  -> (mel, mel_post, mel_lens, (p_targets, e_targets) as the reference returns them);
        intermediates in self.trace (dec_in included)."""
        ids = np.asarray(ids, np.int64)
        lens = np.asarray(lens, np.int64)
        L = ids.shape[1]
        pad = get_mask_from_lengths(lens, L)
        x = self.encoder(ids, pad)
        x = x + self.sd["speaker_emb.weight"][np.asarray(speakers, np.int64)][:, None, :]
        log_d = self.duration_predictor(x, pad)
        ve = self.fs["variance"]["variance_embedding"]
        p_frame, e_frame = ve["pitch_feature"] == "frame_level", ve["energy_feature"] == "frame_level"
        dur = np.asarray(dur, np.float32)
        x_tmp = x
        if not p_frame:
            if isinstance(p_targets, dict):
                p_targets = {k: get_phoneme_level(v, lens, dur, L) for k, v in p_targets.items()}
                p_targets["uv"] = np.where(p_targets["uv"].astype(np.float64) == 1.0, 1.0, 0.0).astype(np.float32)
            elif p_targets is not None:
                p_targets = get_phoneme_level(p_targets, lens, dur, L)
            p_pred, p_idx, p_emb = self.pitch_embedding_forced(x, p_targets, p_control)
            x_tmp = x_tmp + p_emb
        if not e_frame:
            if e_targets is not None:
                e_targets = get_phoneme_level(e_targets, lens, dur, L)
            e_pred, e_idx, e_emb = self.energy_embedding_forced(x, e_targets, e_control)
            x_tmp = x_tmp + e_emb
        x = x_tmp
        mel_lens = np.asarray(mel_lens, np.int64)
        if soft:
            x = np.matmul(np.asarray(attn_soft, self.dt), x)
        else:
            x, mel_lens = self.length_regulator(x, dur)
            T = int(max_mel_len) if max_mel_len is not None else x.shape[1]
            if x.shape[1] < T:
                x = np.concatenate([x, np.zeros((x.shape[0], T - x.shape[1], x.shape[2]), x.dtype)], 1)
        x_tmp = x
        if p_frame:
            p_pred, p_idx, p_emb = self.pitch_embedding_forced(x, p_targets, p_control)
            x_tmp = x_tmp + p_emb
        if e_frame:
            e_pred, e_idx, e_emb = self.energy_embedding_forced(x, e_targets, e_control)
            x_tmp = x_tmp + e_emb
        x = x_tmp
        self.trace.update(log_d=log_d, pitch_pred=p_pred, pitch_idx=p_idx, energy_pred=e_pred, energy_idx=e_idx, lr_out=x)
        mel_pad = get_mask_from_lengths(mel_lens, x.shape[1])
        self.trace["dec_in"] = x + self._pos_enc("decoder", x.shape[1])[None]   # what the first decoder block receives
        x = self.decoder(x, mel_pad)
        self.trace["dec_out"] = x
        mel = linear(x, self.sd["mel_linear.weight"], self.sd["mel_linear.bias"])
        mel_post = self.postnet(mel) + mel
        return mel, mel_post, mel_lens, (p_targets, e_targets)
