"""Drop-in mirrors of the reference's host loop: ``TTS`` (reference e2e_tts/src/api/utils.py:22-160) and the
service wrapper ``Synthesizer`` (e2e_tts/src/api/inference.py:12-50).

Same constructor arguments, attributes (``hop_length``, ``sample_rate``, ``max_wav_value``, ``speakers``,
``config``, ``stats``, ``max_len``) and method signatures.  Differences, all deliberate:

* one HIP engine holds both models, so the mel never leaves HBM between acoustic model and vocoder and the
  only device->host traffic per batch is the int16 PCM (the reference copies fp32 audio, API/utils.py:145);
* ``input_parse`` sorts with a *stable* descending sort (torch.sort(descending=True) at :84 leaves the order of
  equal-length sentences unspecified; batches and audio are identical, only ties may be numbered differently);
* text -> phoneme ids defaults to ``e2e_tts_amd.g2p.text_to_sequence`` (a working restatement of the reference's
  Vietnamese g2p, pinned by a fixture converted with the reference's own code; the reference's ``text_to_sequence``
  cannot run as shipped: cleaners.py:12,26-30 recurses with a bad kwarg) and stays pluggable (``text_to_sequence=``);
* no network call to a text normaliser (API/inference.py:28-33 swallows its failure anyway), no upload;
* ``speed != 1`` is served by the model's duration control instead of an ffmpeg ``atempo`` subprocess (``audio_speed_change``
  keeps the reference's file-level signature on a WSOLA restatement; ffmpeg is absent, so that function is parity-unpinned).
"""
from __future__ import annotations

import json
import os
import time
import wave
from datetime import datetime
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import packer
from ._lib import Engine
from .config import N_SYMBOLS, dims_from_config
from .models import HifiGan, UnsupervisedFastSpeech2, _device_index


def _load_state(path: str):
    import torch
    ckpt = torch.load(path, map_location="cpu", weights_only=True)  # tensors only: nothing in the file is executed
    return ckpt["state_dict"]


class TTS:
    def __init__(self, acoustic_path: str, vocoder_path: str, max_len: int = 300, device=None,
                 text_to_sequence: Optional[Callable[[str], Sequence[int]]] = None, n_symbols: int = N_SYMBOLS,
                 pos_table_rows: int = 4096):
        import yaml
        self.device = device
        self._device_index = _device_index(device)
        base = os.path.dirname(acoustic_path)
        # the three side-car files written by save_information (reference tools_for_model.py:143-152)
        self.config = yaml.safe_load(open(os.path.join(base, "config.yaml"), "r"))  # plain scalars / lists / dicts only
        self.speakers = json.load(open(os.path.join(base, "speakers.json"), "r"))
        self.stats = json.load(open(os.path.join(base, "stats.json"), "r"))
        if self.config["models"]["fastspeech2"]["variance"]["duration_modelling"]["learn_alignment"] is not True:
            raise NotImplementedError("SupervisedFastSpeech2 checkpoints are out of scope (reference API/utils.py:37-40)")
        self._dims = dims_from_config(self.config, self.stats, len(self.speakers), n_symbols, pos_table_rows)
        self._acoustic_state = _load_state(acoustic_path)
        self._vocoder_state = _load_state(vocoder_path)
        self.engine = Engine(self._dims, self._device_index)
        self.engine.load_weights(packer.pack(self._dims, self._acoustic_state, self._vocoder_state))
        self.hop_length = self.config["audio"]["stft"]["hop_length"]
        self.sample_rate = self.config["audio"]["signal"]["sampling_rate"]
        self.max_wav_value = 32768.0
        self.max_len = max_len
        if text_to_sequence is None:
            from .g2p import text_to_sequence as _default_g2p
            text_to_sequence = _default_g2p
        self.text_to_sequence = text_to_sequence
        self._acoustic = None
        self._vocoder = None

    # the reference exposes the two modules as attributes; build the stand-alone mirrors only on demand
    @property
    def acoustic(self) -> UnsupervisedFastSpeech2:
        if self._acoustic is None:
            m = UnsupervisedFastSpeech2(self._dims.n_symbols, len(self.speakers), self._dims.n_mel,
                                        self.config["models"]["fastspeech2"], self.stats, device=self._device_index,
                                        hop_length=self.hop_length, sampling_rate=self.sample_rate)
            m.load_state_dict(self._acoustic_state)
            self._acoustic = m.eval().to(self._device_index)
        return self._acoustic

    @property
    def vocoder(self) -> HifiGan:
        if self._vocoder is None:
            v = HifiGan(self.config["models"]["hifigan"], device=self._device_index)
            v.load_state_dict(self._vocoder_state)
            self._vocoder = v.eval().to(self._device_index)
        return self._vocoder

    # ---- reference API/utils.py:64-80
    def arrange_text(self, text: List[str]) -> List[str]:
        return self.arrange_text_owners(text, self.max_len)[0]

    @staticmethod
    def arrange_text_owners(text: List[str], max_len: int):
        """arrange_text, and for every piece the index of the text it came from (a long line is cut at " , " into pieces that each
        belong to that line alone).  -> (pieces, owners)."""
        arranged_text: List[str] = []
        owners: List[int] = []
        for i, line in enumerate(text):
            if round(len(line) / max_len) != 1:
                pieces = line.split(" , ")
                arranged_text.append(pieces[0])
                owners.append(i)
                for piece in pieces[1:]:
                    if len(arranged_text[-1]) >= max_len:
                        arranged_text.append(piece)
                        owners.append(i)
                    else:
                        arranged_text[-1] = " , ".join([arranged_text[-1], piece])
            else:
                arranged_text.append(line)
                owners.append(i)
        return arranged_text, owners

    @staticmethod
    def pack_sequences(sequences: Sequence[Sequence[int]], max_len: int):
        """The batching arithmetic of reference API/utils.py:84-104 on already-tokenised sequences.

        Sort by length (descending, stable), then cut greedily into batches whose length sum stays <= max_len;
        the sentence that overflows a batch opens the next one WITHOUT being counted in its total (the
        reference's `s, total_lens = e, 0` at :96-99 -- reproduced, it decides the batch composition and the
        padded-batch results depend on it).  Returns ([(ids [B, L] int64, lens [B] int64), ...], revert_indices).
        """
        lens = np.asarray([len(s) for s in sequences], dtype=np.int64)
        order = np.argsort(-lens, kind="stable")
        revert = np.argsort(order, kind="stable")
        spans = []
        s = e = total = 0
        for i, n in enumerate(lens[order]):
            if s == e or total + n <= max_len:
                e = i + 1
                total += int(n)
            else:
                spans.append((s, e))
                s, total = e, 0
        if not spans or spans[-1][1] != len(lens):
            spans.append((s, len(lens)))
        batches = []
        for s, e in spans:
            rows = [sequences[j] for j in order[s:e]]
            L = max(len(r) for r in rows)
            ids = np.zeros((len(rows), L), dtype=np.int64)  # pad_sequence(batch_first=True): zero padding
            for r, row in enumerate(rows):
                ids[r, :len(row)] = np.asarray(row, dtype=np.int64)
            batches.append((ids, lens[order[s:e]].copy()))
        return batches, revert

    def input_parse(self, input_texts: List[str]):
        """-> (list of [ids LongTensor [B, L], lens LongTensor [B]], revert_indices LongTensor) like the reference."""
        import torch
        if self.text_to_sequence is None:
            raise RuntimeError("TTS was built without a text front-end: pass text_to_sequence=... or call inference_ids()")
        seqs = [list(self.text_to_sequence(t)) for t in self.arrange_text(input_texts)]
        batches, revert = self.pack_sequences(seqs, self.max_len)
        return [[torch.from_numpy(i), torch.from_numpy(l)] for i, l in batches], torch.from_numpy(revert)

    # ---- reference API/utils.py:108-117
    def combine_audio(self, audios, lengths, distance: int) -> np.ndarray:
        output_audio = []
        for i, audio in enumerate(audios):
            audio = np.asarray(audio)[: int(lengths[i]) * self.hop_length]
            audio = audio * self.max_wav_value
            output_audio.extend([audio, np.zeros(distance)])
        return np.concatenate(output_audio).astype("int16")

    def _combine_pcm(self, pcms: List[np.ndarray], lengths: List[int], distance: int) -> np.ndarray:
        """Same result as combine_audio, from the int16 the GPU already produced (trunc(wav * 32768))."""
        total = sum(int(n) * self.hop_length + distance for n in lengths)
        out = np.zeros(total, dtype=np.int16)
        pos = 0
        for pcm, n in zip(pcms, lengths):
            k = int(n) * self.hop_length
            out[pos:pos + k] = pcm[:k]
            pos += k + distance
        return out

    @staticmethod
    def _combine_samples(pcms: List[np.ndarray], n_samples: List[int], distance: int) -> np.ndarray:
        """_combine_pcm with the utterances' lengths given in samples (utterances converted to another rate)."""
        out = np.zeros(sum(int(k) + distance for k in n_samples), dtype=np.int16)
        pos = 0
        for pcm, k in zip(pcms, n_samples):
            out[pos:pos + int(k)] = pcm[:int(k)]
            pos += int(k) + distance
        return out

    def resampler(self, output_rate: int):
        """The handle that converts the model's rate to ``output_rate`` on the engine's GPU (default filter), made at first use."""
        from .resample import Resampler
        cache = self.__dict__.setdefault("_resamplers", {})
        if int(output_rate) not in cache:
            cache[int(output_rate)] = Resampler(self.sample_rate, int(output_rate), device=self._device_index)
        return cache[int(output_rate)]

    def _synthesize_at_rate(self, rs, b, p):
        """One batch whose PCM never visits the host at the model's rate: the engine's resident int16 rows go to a device tensor
        (e2etts_fetch_pcm takes a device pointer), the resampler's stream is ordered after the engine's, and only the converted PCM is
        copied out.  -> (pcm rows at the output rate, their lengths in samples)."""
        import torch
        from ._lib import _addr
        eng = self.engine
        _, mel_lens, T = eng.synthesize(b["ids"], b["lens"], b["speaker"], b["duration_control"], p, b["energy_control"], fetch_pcm=False)
        B = int(b["ids"].shape[0])
        dev = torch.empty((B, T * self.hop_length), dtype=torch.int16, device=f"cuda:{self._device_index}")
        eng._check(eng.lib.e2etts_fetch_pcm(eng._h, _addr(dev), dev.numel()), "e2etts_fetch_pcm")
        rs.load()
        rs.order_after_stream(eng.stream())
        out = rs.forward(dev, n_valid=np.asarray(mel_lens, np.int64) * self.hop_length, want=("pcm",))
        return list(out["pcm"]), [int(k) for k in out["n_out"]]

    @classmethod
    def plan_requests(cls, sequences: Sequence[Sequence[int]], max_len: int, speaker=0, duration_control=1.0, pitch_control=1.0,
                      energy_control=1.0):
        """The batches TTS.inference_ids runs, with per-request parameters: pack_sequences, and for every batch the speaker ids and the
        controls of its rows.  Pure host function.

        ``speaker`` is one speaker index or a list with one per sequence; each control is a number or a list with one entry per sequence,
        an entry being a number (per utterance) or an array of len(sequence) values (per phoneme).  An entry follows its sequence through
        the length sort and the batching.  Within a batch, equal numbers collapse to one (the scalar entry points: all-equal lists plan
        exactly what scalars plan); different numbers become a [B, 1] array; a batch with a per-phoneme entry gets a [B, L] array, every
        row padded with its last value (so a padded slot -- and a frame past the row's end at the frame level -- takes the control of the
        row's last phoneme).  -> ([dict(ids, lens, speaker, rows, duration_control, pitch_control, energy_control)], revert_indices)."""
        seqs = [list(q) for q in sequences]
        n = len(seqs)
        batches, revert = cls.pack_sequences(seqs, max_len)
        order = np.argsort(revert, kind="stable")

        def per_seq(v, name, arrays_ok):
            if not isinstance(v, (list, tuple)):
                return None
            if len(v) != n:
                raise ValueError(f"{name}: {len(v)} entries for {n} sequences")
            out = []
            for j, x in enumerate(v):
                if isinstance(x, (list, tuple, np.ndarray)) or hasattr(x, "shape"):
                    if not arrays_ok:
                        raise ValueError(f"{name}[{j}]: per-phoneme controls are taken per sequence (inference_ids), not per text")
                    a = np.asarray(x, np.float32).reshape(-1)
                    if a.size != len(seqs[j]):
                        raise ValueError(f"{name}[{j}]: {a.size} values for a sequence of {len(seqs[j])} phonemes")
                    out.append(a)
                else:
                    out.append(float(x))
            return out

        spk = per_seq(speaker, "speaker", False)
        ctls = [per_seq(v, name, True) for v, name in ((duration_control, "duration_control"), (pitch_control, "pitch_control"),
                                                       (energy_control, "energy_control"))]
        plan, s = [], 0
        for ids, lens in batches:
            rows = order[s:s + len(lens)]
            s += len(lens)
            item = dict(ids=ids, lens=lens, rows=rows)
            if spk is None:
                item["speaker"] = np.array([int(speaker)], np.int64)
            else:
                ks = [int(spk[j]) for j in rows]
                item["speaker"] = np.array(ks[:1] if len(set(ks)) == 1 else ks, np.int64)
            for key, scalar, entries in zip(("duration_control", "pitch_control", "energy_control"),
                                            (duration_control, pitch_control, energy_control), ctls):
                if entries is None:
                    item[key] = scalar
                    continue
                es = [entries[j] for j in rows]
                if all(isinstance(x, float) for x in es):
                    item[key] = es[0] if len(set(es)) == 1 else np.array(es, np.float32)[:, None]
                    continue
                L = ids.shape[1]
                a = np.empty((len(es), L), np.float32)
                for r, x in enumerate(es):
                    if isinstance(x, float):
                        a[r] = x
                    else:
                        a[r, :x.size] = x
                        a[r, x.size:] = x[-1]
                item[key] = a
            plan.append(item)
        return plan, revert

    # the denoiser behind ``denoise_strength``: the reference's defaults (V/denoiser.py:159-160: filter_length, n_overlap, win_length; Hann,
    # mode='zeros' = 88 zero frames); a subclass or an instance may set another geometry before the first denoised call
    denoiser_geometry = (1024, 4, 1024)

    def _prepare_denoiser(self) -> None:
        """Bases loaded and bias calibrated on the engine's own vocoder, at first use and again whenever the engine has been given other
        weights or other bases since (Engine.denoiser_calibrated).  Called under the engine's lock."""
        if getattr(self.engine, "denoiser_calibrated", None) == self.denoiser_geometry:
            return
        from .denoiser import engine_window, stft_bases
        N, V, W = self.denoiser_geometry
        fwd, inv, win_sq = stft_bases(N, N // V, W)
        self.engine.denoiser_load(fwd, inv, N, N // V, engine_window(win_sq, N, W, "hann"))
        self.engine.denoiser_calibrate(None, 88)
        self.engine.denoiser_calibrated = self.denoiser_geometry

    def inference_ids(self, sequences: Sequence[Sequence[int]], speaker_id, pitch_control=1.0, energy_control=1.0,
                      duration_control=1.0, silence_distance: float = 0.5, denoise_strength: float = 0.0,
                      output_rate: Optional[int] = None) -> np.ndarray:
        """TTS.inference from phoneme-id sequences (the part after text_to_sequence).  ``speaker_id`` and each control may be a list with
        one entry per sequence (a control entry may also be an array of per-phoneme values): requests with different settings share
        batches (plan_requests).  ``denoise_strength > 0`` subtracts that much of the vocoder's bias spectrum from every utterance
        (_prepare_denoiser: the reference's defaults, calibrated on the engine's own vocoder); 0, the default, is the path without a denoiser.
        ``output_rate`` (None or the model's rate: today's path, bit for bit): every utterance's PCM -- denoised, when that is asked for --
        is converted to that rate on the GPU (e2e_tts_amd.resample, n_valid = mel_lens * hop) and the silence between utterances is
        int(silence_distance * output_rate) samples."""
        pcms, lengths, rs = self._synthesize_requests(sequences, speaker_id, pitch_control, energy_control, duration_control, denoise_strength, output_rate)
        if rs is not None:
            return self._combine_samples(pcms, lengths, int(silence_distance * int(output_rate)))
        return self._combine_pcm(pcms, lengths, int(silence_distance * self.sample_rate))

    def _synthesize_requests(self, sequences, speaker_id, pitch_control, energy_control, duration_control, denoise_strength, output_rate):
        """The batch loop of ``inference_ids``: plans the requests, runs the batches and puts the utterances back into request order.
        -> (one int16 PCM row per request, its length -- in mel frames, or in samples when the PCM was converted to ``output_rate`` --, the
        resampler used or None)."""
        denoise_strength = float(denoise_strength)
        rs = None
        if output_rate is not None and int(output_rate) != int(self.sample_rate):
            rs = self.resampler(output_rate)
        if denoise_strength < 0:
            raise ValueError("denoise_strength must be >= 0")
        if isinstance(speaker_id, (list, tuple)):
            spk = [self.speakers[k] for k in speaker_id]   # KeyError for an unknown speaker, as the reference
        else:
            spk = self.speakers[speaker_id]
        plan, revert = self.plan_requests(sequences, self.max_len, spk, duration_control, pitch_control, energy_control)
        uv = not self._dims.pitch_no_uv
        pcms, lengths = [], []
        # the strength is engine-wide state: it is set, used and cleared under the engine's lock, so that another thread's call on this TTS
        # (or on the engine itself) with another strength cannot fall between set_denoise and synthesize
        with self.engine.lock:
            if denoise_strength > 0:
                self._prepare_denoiser()
                self.engine.set_denoise(denoise_strength)
            try:
                for b in plan:
                    p = b["pitch_control"]
                    if uv and isinstance(p, np.ndarray):
                        p = p[..., None]   # the reference's [B, 1, 1] / [B, L, 1]: one factor for the f0 and the uv column
                    if rs is not None:
                        pcm, n_samples = self._synthesize_at_rate(rs, b, p)
                        pcms.extend(pcm)
                        lengths.extend(n_samples)
                        continue
                    pcm, mel_lens, T = self.engine.synthesize(b["ids"], b["lens"], b["speaker"], b["duration_control"], p, b["energy_control"])
                    pcms.extend(list(pcm))
                    lengths.extend(int(x) for x in mel_lens)
            finally:
                if denoise_strength > 0:
                    self.engine.set_denoise(0.0)
        pcms = [pcms[i] for i in revert.tolist()]
        lengths = [lengths[i] for i in revert.tolist()]
        return pcms, lengths, rs

    def _recording_chain(self):
        """The mirror whose recording chain (condition, rate, mel front-end, pitch tracker) ``evaluate_ids`` uses: built without an
        engine of its own, with this checkpoint's audio configuration."""
        m = self.__dict__.get("_recording_model")
        if m is None:
            m = UnsupervisedFastSpeech2(self._dims.n_symbols, len(self.speakers), self._dims.n_mel, self.config["models"]["fastspeech2"], self.stats,
                                        device=self._device_index, hop_length=self.hop_length, sampling_rate=self.sample_rate)
            audio = self.config.get("audio", {})
            if all(k in audio for k in ("stft", "mel", "signal")):
                m.set_audio_config(audio)
            self._recording_model = m
        return m

    def evaluate_ids(self, sequences: Sequence[Sequence[int]], recordings, recording_lens, speaker_id, pitch_control=1.0, energy_control=1.0,
                     duration_control=1.0, denoise_strength: float = 0.0, wav_rate: Optional[int] = None, condition=None, mode: str = "dtw",
                     band: Optional[int] = None, return_path: bool = False, n_cep: int = 13):
        """How close every synthesized request is to the recording it should resemble: request i is synthesized through the path
        ``inference_ids`` uses (same planning, batching, controls and denoiser) and compared with row i of ``recordings`` [R, n] (float32
        in [-1, 1] or int16 PCM; numpy or torch, host or GPU; ``recording_lens`` [R] samples).  Both sides go down to log-mel and f0 on the
        GPU -- the recordings through the chain ``align_audio`` uses (``wav_rate``, ``condition``: as there), the synthesized PCM through
        the same mel front-end and pitch tracker at the model's rate -- and e2e_tts_amd.compare aligns them (``mode``, ``band``: as
        ``Comparator.run``).  -> one dict per request, in request order: ``mcd_db`` (on DCT cepstra of this project's log-mel: not
        comparable with SPTK / WORLD figures), ``mel_l1``, ``f0_rmse_hz``, ``f0_rmse_cents``, ``n_voiced_both``, ``n_vuv_mismatch``,
        ``n_path``, ``dist_total``, ``status``.  Side A is the recording, side B the synthesized utterance."""
        from .compare import Comparator
        seqs = [list(q) for q in sequences]
        if len(recordings) != len(seqs):
            raise ValueError(f"{len(recordings)} recordings for {len(seqs)} sequences")
        pcms, lengths, _ = self._synthesize_requests(seqs, speaker_id, pitch_control, energy_control, duration_control, denoise_strength, None)
        n = [int(k) * self.hop_length for k in lengths]
        synth = np.zeros((len(pcms), max(n)), np.int16)
        for i, (pcm, k) in enumerate(zip(pcms, n)):
            synth[i, :k] = pcm[:k]
        m = self._recording_chain()
        cmp_ = self.__dict__.get("_comparator")
        if cmp_ is None or cmp_.n_cep != int(n_cep):
            cmp_ = self._comparator = Comparator(self._dims.n_mel, int(n_cep), device=self._device_index)
        fe, trk, ml = m.recording_features(recordings, recording_lens, wav_rate=wav_rate, condition=condition)
        cmp_.set_a(fe, ml, trk)
        fe, trk, ml = m.recording_features(synth, np.asarray(n, np.int64))
        cmp_.set_b(fe, ml, trk)
        return cmp_.run(mode, band, return_path)

    def evaluate_vocoder(self, recordings, recording_lens, critic, wav_rate: Optional[int] = None, condition=None):
        """Copy synthesis, judged as the reference judges a vocoder: every recording goes down to log-mel through the chain ``align_audio``
        uses (``wav_rate``, ``condition``: as there), the mel goes through this checkpoint's vocoder, and ``critic`` (a loaded
        ``e2e_tts_amd.critic.Critic`` on this device) compares the result with the recording the mel was made from, cut to
        ``mel_len * hop`` samples: discriminator scores and the feature loss, sample-aligned (int16 recordings against the vocoder's int16
        PCM, float32 ones against its float32 waveform).  Everything stays on the device: the
        vocoder reads the front-end's resident mel, the critic reads the resident recording and the vocoder's output, its stream ordered
        after theirs.  -> ``Critic.run``'s list of dicts, one per recording.  Separates "the vocoder is worse" from "the acoustic model
        is worse", which ``evaluate_ids``' figures on log-mel cannot."""
        import torch
        m = self._recording_chain()
        stft = m._default_stft()
        wl = np.asarray(torch.as_tensor(recording_lens).cpu(), dtype=np.int64).reshape(-1)
        x, wl, after = m._recording_input(recordings, wl, stft, wav_rate, condition)
        fe = stft.frontend
        r = fe.forward(x, wl, want=())
        B, T = int(x.shape[0]), int(r["T"])
        hop = self.hop_length
        n = np.minimum(np.asarray(r["mel_lens"], np.int64).reshape(-1) * hop, np.asarray(wl, np.int64).reshape(-1))
        # an int16 recording is compared with the vocoder's int16 PCM, a float32 one with its float32 waveform: one sample format per call
        pcm = "int16" in str(x.dtype)
        wav = torch.empty((B, T * hop), dtype=torch.int16 if pcm else torch.float32, device=torch.device("cuda", self._device_index))
        import ctypes as C
        eng, mel = self.engine, fe.resident()[0]
        with eng.lock:   # e2etts_vocoder_btc on the front-end's HBM: the engine's stream after torch's (the output tensor) and after the front-end's
            eng._order(wav)
            eng._check(eng.lib.e2etts_order_after(eng._h, C.c_void_p(fe.stream())), "e2etts_order_after")
            eng._check(eng.lib.e2etts_vocoder_btc(eng._h, mel.data_ptr(), B, T, None if pcm else wav.data_ptr(), wav.data_ptr() if pcm else None), "e2etts_vocoder")
            critic.order_after_stream(eng.stream())
        if after:
            critic.order_after_stream(after)
        return critic.run(x, n, wav, n)

    def build_stats(self, recordings, recording_lens, wav_rate: Optional[int] = None, condition=None, batch: int = 32) -> dict:
        """``stats.json`` of a corpus of recordings, as the reference's ``TextMelLoader.build_stats`` computes it from files on disk:
        ``recordings`` [R, n] (float32 in [-1, 1] or int16 PCM; numpy or torch, host or GPU; ``recording_lens`` [R] samples) go through the
        chain ``align_audio`` uses (``wav_rate``, ``condition``: as there), ``batch`` rows at a time, and the mel front-end's frame energies
        and the pitch tracker's f0 are accumulated where they lie on the device (e2e_tts_amd.stats: the definition is
        include/e2etts_stats.h).  -> ``{"f0": {mean, std}, "energy": {max, min, mean, std}}``, Python floats; no ``"pitch"`` block (the
        reference's pyworld track is not built; see ``stats.CorpusStats.result``).  The result does not depend on ``batch``."""
        from .models import build_stats
        if int(batch) < 1:
            raise ValueError("batch must be at least 1")
        lens = np.asarray(recording_lens.cpu() if hasattr(recording_lens, "cpu") else recording_lens, dtype=np.int64).reshape(-1)
        if len(recordings) != len(lens):
            raise ValueError(f"{len(recordings)} recordings for {len(lens)} lengths")
        batches = ((recordings[i:i + int(batch)], lens[i:i + int(batch)]) for i in range(0, len(lens), int(batch)))
        return build_stats(self._recording_chain(), batches, wav_rate=wav_rate, condition=condition)

    def evaluate(self, texts: list, recordings, recording_lens, speaker_id, **kwargs):
        """``evaluate_ids`` from texts: one recording per text.  A text that ``arrange_text`` would cut into pieces is refused: a
        recording is compared with one utterance."""
        if isinstance(texts, str):
            texts = [texts]
        if self.text_to_sequence is None:
            raise RuntimeError("TTS was built without a text front-end: pass text_to_sequence=... or call evaluate_ids()")
        pieces, owners = self.arrange_text_owners(texts, self.max_len)
        if len(pieces) != len(texts):
            raise ValueError("a text is cut into several utterances (arrange_text): evaluate it piece by piece, one recording per piece")
        return self.evaluate_ids([list(self.text_to_sequence(t)) for t in pieces], recordings, recording_lens, speaker_id, **kwargs)

    def inference(self, texts: list, speaker_id, pitch_control=1.0, energy_control=1.0, duration_control=1.0,
                  silence_distance: float = 0.5, denoise_strength: float = 0.0, output_rate: Optional[int] = None) -> np.ndarray:
        """reference API/utils.py:119-160 -> 1-D np.int16 (at ``output_rate`` when one is given: see ``inference_ids``).  ``speaker_id`` and each control may also be a list with one entry (a name /
        a number) per text: every piece arrange_text cuts from a text inherits that text's entry."""
        if isinstance(texts, str):
            texts = [texts]  # API/inference.py:39-40 passes a bare str, which the reference would iterate per character
        if self.text_to_sequence is None:
            raise RuntimeError("TTS was built without a text front-end: pass text_to_sequence=... or call inference_ids()")
        pieces, owners = self.arrange_text_owners(texts, self.max_len)

        def follow(v, name):
            if not isinstance(v, (list, tuple)):
                return v
            if len(v) != len(texts):
                raise ValueError(f"{name}: {len(v)} entries for {len(texts)} texts")
            return [v[i] for i in owners]
        seqs = [list(self.text_to_sequence(t)) for t in pieces]
        generated_audio = self.inference_ids(seqs, follow(speaker_id, "speaker_id"), follow(pitch_control, "pitch_control"),
                                             follow(energy_control, "energy_control"), follow(duration_control, "duration_control"),
                                             silence_distance, denoise_strength, output_rate)
        print(f"Audio Saved: {time.strftime('%H:%M:%S', time.gmtime(generated_audio.size / (output_rate or self.sample_rate)))}")
        return generated_audio


def write_wav(path: str, audio: np.ndarray, samplerate: int) -> None:
    """16-bit mono PCM WAV (what soundfile.write(path, int16 array, sr) produces at API/inference.py:47)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(samplerate))
        f.writeframes(np.ascontiguousarray(audio, dtype="<i2").tobytes())


def read_wav(path: str):
    """-> (int16 mono samples, sample rate) of a 16-bit PCM WAV (multi-channel files are averaged)."""
    with wave.open(path, "rb") as f:
        if f.getsampwidth() != 2:
            raise ValueError("only 16-bit PCM WAV files are supported")
        sr, ch = f.getframerate(), f.getnchannels()
        a = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    if ch > 1:
        a = a.reshape(-1, ch).astype(np.int32).mean(axis=1).astype(np.int16)
    return a, sr


def time_stretch_wsola(x: np.ndarray, speed: float, sr: int = 22050, frame_ms: float = 40.0, search_ms: float = 10.0) -> np.ndarray:
    """Tempo change without pitch change by waveform-similarity overlap-add (WSOLA, Verhelst & Roelands 1993) -- the family
    of algorithm behind ffmpeg's ``atempo`` filter, which the reference shells out to (API/utils.py:163-172).  ffmpeg is not
    part of this build, so this is a restatement of the published method, not of ffmpeg's code: *parity unpinned*.
    Host-side utility, not on the GPU hot path (see ``Synthesizer.synthesis`` for the tempo control that is)."""
    if not (0.25 <= speed <= 4.0):
        raise ValueError("speed must lie in [0.25, 4]")
    x = np.asarray(x, dtype=np.float64)
    if speed == 1.0 or x.size == 0:
        return x.copy()
    n = max(int(sr * frame_ms / 1000.0) // 2 * 2, 64)      # frame length (even)
    hop_out = n // 2                                       # 50 % overlap of Hann windows sums to one
    hop_in = hop_out * speed
    delta = max(int(sr * search_ms / 1000.0), 1)
    win = np.hanning(n + 1)[:n]
    n_frames = max(int(np.ceil((x.size / speed) / hop_out)), 1)
    xp = np.concatenate([np.zeros(delta + n), x, np.zeros(2 * n + delta + int(hop_in) + 1)])
    out = np.zeros(n_frames * hop_out + n)
    pos = delta + n  # index in xp of the natural continuation of the previous frame
    for i in range(n_frames):
        target = int(round(i * hop_in)) + delta + n
        if i == 0:
            best = target
        else:
            # the candidate within +-delta of `target` that best continues what was just written (template = natural successor)
            tmpl = xp[pos:pos + n]
            lo = target - delta
            seg = xp[lo:lo + n + 2 * delta]
            corr = np.correlate(seg, tmpl, mode="valid")    # 2 delta + 1 lags
            best = lo + int(np.argmax(corr))
        out[i * hop_out:i * hop_out + n] += xp[best:best + n] * win
        pos = best + hop_out
    return out[: int(round(x.size / speed))]


def audio_speed_change(input_path: str, output_path: str = None, speed_rate: float = 1.0, engine: Optional[Engine] = None) -> str:
    """Same signature, output naming and return value as reference API/utils.py:163-172, without the ffmpeg subprocess:
    reads the WAV, time-stretches it and writes ``<input>_<speed>.<ext>``.  With ``engine`` the stretch runs on the GPU
    (``Engine.tempo`` -> ``e2etts_tempo``, the WSOLA kernel); without one, on the host (``time_stretch_wsola``, the same algorithm in
    numpy).  Parity unpinned either way: the reference's ffmpeg ``atempo`` filter is not available here."""
    if output_path is None:
        file_type = input_path.split(".")[-1]
        output_path = f"{input_path[:-len(file_type) - 1]}_{round(speed_rate, 2)}.{file_type}"
    audio, sr = read_wav(input_path)
    if engine is not None:
        pcm = engine.tempo(audio, float(speed_rate), sr)
    else:
        y = time_stretch_wsola(audio.astype(np.float64), float(speed_rate), sr)
        pcm = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    write_wav(output_path, pcm, sr)
    return output_path


class Synthesizer:
    """reference e2e_tts/src/api/inference.py:12-50."""

    def __init__(self, acoustic_path: str, vocoder_path: str, output_dir: str = "outputs", **tts_kwargs) -> None:
        self.model = TTS(acoustic_path=acoustic_path, vocoder_path=vocoder_path, **tts_kwargs)
        os.makedirs(output_dir, exist_ok=True)
        self.output_dir = output_dir

    def tts_to_file(self, text: str, file_path: str, speed: float = 1):
        return self.synthesis(text, file_path, speed)

    def synthesis(self, text: str, save_filepath: str = None, speed: float = 1, speaker_id: str = "hn_minhphuong", sr: int = 22050,
                  speed_mode: str = "duration", denoise_strength: float = 0.0, resample: bool = False):
        """reference API/inference.py:24-50.  ``sr`` only labels the file, as in the reference (the samples stay at the model's rate);
        with ``resample=True`` the audio is converted to ``sr`` on the GPU before it is written (``TTS.inference(output_rate=sr)``).  ``denoise_strength``: see ``TTS.inference_ids`` (0 = off).  ``speed != 1``: the reference synthesises at normal tempo and then runs ffmpeg's
        ``atempo`` on the file (API/utils.py:163-172).  Here, by default (``speed_mode="duration"``), the tempo goes into the
        model instead -- ``duration_control = 1 / speed`` (U/layers.py:218-221), i.e. the phonemes are simply generated shorter
        or longer on the GPU path, with no vocoded-audio artefacts; ``speed_mode="wsola"`` post-processes the file like the
        reference does (``audio_speed_change``).  Either way the returned path is named ``<file>_<speed>.wav`` as in the reference,
        and -- as in the reference, which writes the file before it runs ffmpeg on it -- ``save_filepath`` itself exists too
        (callers such as the top-level ``synthesizer.Synthesizer`` hand that path on); in duration mode it holds the same
        tempo-adjusted audio."""
        assert len(text) > 0
        if speed_mode not in ("duration", "wsola"):
            raise ValueError("speed_mode must be 'duration' or 'wsola'")
        if not save_filepath:
            save_filepath = os.path.join(self.output_dir, datetime.now().strftime("%m_%d_%Y_%H_%M_%S") + ".wav")
        in_model = speed != 1 and speed_mode == "duration"
        audio = self.model.inference(texts=[text], speaker_id=speaker_id, pitch_control=1.0, energy_control=1.0,
                                     duration_control=(1.0 / float(speed)) if in_model else 1.0, silence_distance=0.5,
                                     # (handed on only when set: self.model may be any object with the reference's TTS.inference signature)
                                     **({"denoise_strength": denoise_strength} if denoise_strength else {}),
                                     **({"output_rate": int(sr)} if resample else {}))
        write_wav(save_filepath, audio, sr)
        if in_model:
            file_type = save_filepath.split(".")[-1]
            save_filepath = f"{save_filepath[:-len(file_type) - 1]}_{round(speed, 2)}.{file_type}"
            write_wav(save_filepath, audio, sr)
        if speed != 1 and not in_model:
            save_filepath = audio_speed_change(save_filepath, speed_rate=speed, engine=getattr(self.model, "engine", None))
        return save_filepath
