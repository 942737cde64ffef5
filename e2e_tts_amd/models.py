"""Drop-in mirrors of the reference's two model classes, backed by the HIP engine.

``UnsupervisedFastSpeech2`` mirrors reference e2e_tts/models/acoustic/unsupervised_fastspeech2/model.py:8-68,
155-194 and ``HifiGan`` mirrors e2e_tts/models/vocoder/generator.py:13-62: same constructor arguments, same
``load_state_dict`` / ``eval`` / ``to`` call sequence that ``TTS.__init__`` performs (API/utils.py:41-56), same
``inference`` / ``forward`` signatures and return structure (torch tensors, on the engine's GPU).

They are NOT nn.Modules and hold no torch parameters: ``load_state_dict`` packs the checkpoint into the
engine's HBM image.  Training-side methods (``forward`` with targets, ``parse_batch``) are out of scope.

Forced alignment -- the reference's ``AlignmentEncoder`` and ``b_mas``, i.e. the ``attn_out`` of its training forward -- is served by the
companion library (include/e2etts_align.h): ``AlignmentEncoder``, ``b_mas`` and ``UnsupervisedFastSpeech2.align`` below.

The analysis side -- the reference's ``TorchSTFT.mel_spectrogram`` / ``generate_melspecs`` (e2e_tts/src/tools/stft.py), a recording to
log-mel frames and frame energies -- is served by the mel library (include/e2etts_mel.h): ``TorchSTFT``, ``generate_melspecs`` and
``UnsupervisedFastSpeech2.align_audio`` (recording -> mel -> durations, all on the device).

The f0 track of a recording and the data loader's pitch targets -- the reference's ``extract_f0`` (parselmouth) and ``get_f0`` -- are
served by the pitch library (include/e2etts_f0.h; unpinned against parselmouth): ``extract_f0``, ``f0_targets`` and
``UnsupervisedFastSpeech2.forward_audio(p_targets="extract")``.

The corpus statistics every normalising link reads -- the reference's ``TextMelLoader.build_stats``, ``stats.json`` -- and the data
loader's energy target are served by the statistics library (include/e2etts_stats.h): ``build_stats`` and
``UnsupervisedFastSpeech2.forward_audio(e_targets="extract")``.
"""
from __future__ import annotations

from typing import Mapping, Optional

import numpy as np

from . import packer
from ._lib import Engine
from .config import EngineDims, dims_from_config, default_config


def _torch():
    import torch
    return torch


def _device_index(device) -> int:
    if device is None:
        return 0
    if isinstance(device, int):
        return device
    torch = _torch()
    d = torch.device(device)
    if d.type != "cuda":
        raise RuntimeError(f"e2e_tts_amd runs on MI355X GPUs only; device={device!r} was requested (no CPU fallback)")
    return d.index or 0


class _EngineBacked:
    """Shared plumbing: one Engine, (re)created lazily on the requested GPU, weights packed on load."""

    def __init__(self):
        self._engine: Optional[Engine] = None
        self._device = 0
        self._blob = None
        self.training = False

    def _dims(self) -> EngineDims:
        raise NotImplementedError

    def _pack(self, state) -> np.ndarray:
        raise NotImplementedError

    def _ensure_engine(self) -> Engine:
        if self._engine is None:
            self._engine = Engine(self._dims(), self._device)
            if self._blob is not None:
                self._engine.load_weights(self._blob)
        return self._engine

    # nn.Module-style surface used by TTS.__init__
    def load_state_dict(self, state_dict: Mapping[str, object], strict: bool = True):
        self._blob = self._pack(state_dict)
        if self._engine is not None:
            self._engine.load_weights(self._blob)
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("the HIP engine is inference only")
        return self

    def to(self, device):
        idx = _device_index(device)
        if idx != self._device and self._engine is not None:
            self._engine.close()
            self._engine = None
        self._device = idx
        self._ensure_engine()
        return self

    def cuda(self, device=None):
        return self.to(device if device is not None else 0)

    @property
    def engine(self) -> Engine:
        return self._ensure_engine()


class UnsupervisedFastSpeech2(_EngineBacked):
    def __init__(self, n_symbols: int, n_speakers: int, n_channels: int, config: dict, stats: dict, device=None,
                 hop_length: int = 256, sampling_rate: int = 22050, hifigan_config: Optional[dict] = None,
                 pos_table_rows: int = 4096):
        """``config`` is the ``models.fastspeech2`` sub-dictionary, exactly as the reference passes it
        (API/utils.py:41-47).  The extra keyword arguments only matter when this object shares an engine with a
        vocoder (see ``e2e_tts_amd.api.TTS``)."""
        super().__init__()
        self.config = config
        self.stats = stats
        self.n_symbols, self.n_speakers, self.n_channels = n_symbols, n_speakers, n_channels
        full = default_config()
        full["models"]["fastspeech2"] = config
        if hifigan_config is not None:
            full["models"]["hifigan"] = hifigan_config
        full["audio"]["mel"]["channels"] = n_channels
        full["audio"]["stft"]["hop_length"] = hop_length
        full["audio"]["signal"]["sampling_rate"] = sampling_rate
        self._full_config = full
        self._dims_cache = dims_from_config(full, stats, n_speakers, n_symbols, pos_table_rows)
        self._device = _device_index(device)

    def _dims(self) -> EngineDims:
        return self._dims_cache

    def _pack(self, state) -> np.ndarray:
        return packer.pack(self._dims_cache, state, None)

    def inference(self, speaker, texts, txt_lens, max_txt_len=None, d_control: float = 1.0, p_control: float = 1.0,
                  e_control: float = 1.0):
        """-> ((mel [B, T, n_mel], mel_post [B, T, n_mel], duration_rounded [B, L] fp32), mel_lens [B] int64),
        torch tensors on the engine's GPU (reference U/model.py:155-194).  ``max_txt_len`` is accepted for
        signature compatibility; like the reference's mask it must equal texts.shape[1].

        Each control is a number or, as the reference's tensor arithmetic allows (U/layers.py:145,157,168,218-221), a tensor or array
        (host or GPU) per utterance ([B, 1]; pitch under use_uv [B, 1, 1]) or per phoneme ([B, L], [1, L], [L]; pitch under use_uv
        [B, L, 1]) -- e2etts_acoustic_ctl, _lib.control_array.  With frame-level features a per-phoneme control is expanded along the
        rounded durations (include/e2etts.h)."""
        torch = _torch()
        eng = self._ensure_engine()
        dev = torch.device("cuda", self._device)
        ids = torch.as_tensor(texts, dtype=torch.int64).contiguous()
        lens = torch.as_tensor(txt_lens, dtype=torch.int64).contiguous()
        spk = torch.as_tensor(speaker, dtype=torch.int64).reshape(-1).contiguous()
        if max_txt_len is not None and int(max_txt_len) != ids.shape[1]:
            raise ValueError(f"max_txt_len={int(max_txt_len)} != texts.shape[1]={ids.shape[1]}")
        with eng.lock:  # the mel tensors are the RESIDENT result of this acoustic() call: no other thread's call in between
            r = eng.acoustic(ids, lens, spk, d_control, p_control, e_control, want=("dur", "mel_lens"))
            B, T = r["B"], r["T"]
            mel = torch.empty((B, T, self.n_channels), dtype=torch.float32, device=dev)
            mel_post = torch.empty_like(mel)
            eng.fetch_mel(B, T, out_mel=mel, out_mel_post=mel_post)
        dur = torch.from_numpy(r["dur"]).to(dev)
        mel_lens = torch.from_numpy(r["mel_lens"]).to(dev)
        return (mel, mel_post, dur), mel_lens

    def load_state_dict(self, state_dict: Mapping[str, object], strict: bool = True):
        """As before for synthesis; additionally keeps what forced alignment reads (``variance_adaptor.aligner.*``, the phoneme and speaker
        embedding tables) when the checkpoint holds it.  Nothing is sent to a GPU for it until ``align`` is called."""
        super().load_state_dict(state_dict, strict)
        self._aligner = None
        self._align_state = None
        if any(k.startswith(packer.ALIGNER_PREFIX) for k in state_dict):
            keep = [k for k in state_dict if k.startswith(packer.ALIGNER_PREFIX)] + ["encoder.src_word_emb.weight", "speaker_emb.weight"]
            self._align_state = {k: packer._np(state_dict[k]) for k in keep}
        return self

    def _ensure_aligner(self):
        if getattr(self, "_align_state", None) is None:
            raise RuntimeError("align() needs a loaded state dict that holds variance_adaptor.aligner.* (load_state_dict first)")
        if self._aligner is None or self._aligner[0].encoder.device != self._device:
            torch = _torch()
            dev = torch.device("cuda", self._device)
            temperature = self.config["variance"]["duration_modelling"]["aligner_temperature"]
            H = self.config["encoder_hidden"]
            enc = AlignmentEncoder(self.n_channels, self.n_channels, H, temperature, device=self._device)   # U/layers.py:30-35: n_att = n_mel
            enc.load_state_dict({k[len(packer.ALIGNER_PREFIX):]: v for k, v in self._align_state.items() if k.startswith(packer.ALIGNER_PREFIX)})
            emb = torch.from_numpy(np.ascontiguousarray(self._align_state["encoder.src_word_emb.weight"], dtype=np.float32)).to(dev)
            spk = torch.from_numpy(np.ascontiguousarray(self._align_state["speaker_emb.weight"], dtype=np.float32)).to(dev)
            self._aligner = (enc, emb, spk)
        return self._aligner

    def align(self, speaker, texts, txt_lens, mels, mel_lens, attn_prior=None):
        """Forced alignment of recordings with the model's own aligner: the reference's ``attn_out`` (U/layers.py:203-212) without the rest
        of the training forward.  speaker [B] (or one id for the batch), texts [B, L] int64, txt_lens [B], mels [B, T, n_mel] (the layout
        ``inference`` returns; the reference's parse_batch transposes to it, U/model.py:80), mel_lens [B], attn_prior [B, T, L] or None -- the
        beta-binomial prior is then built per row, as the reference's data preparation does (scipy on the host, then uploaded) -- or
        "device": the same prior (P trials evaluated at 0 .. P - 1, include/e2etts_align.h) generated inside the aligner's attention
        pass; no prior array is built or uploaded.
        -> (attn_soft [B, 1, T, L], attn_hard [B, 1, T, L], attn_hard_dur [B, L], attn_logprob [B, 1, T, L]), torch tensors on the GPU."""
        from . import aligner as al
        torch = _torch()
        enc, emb, spk_table = self._ensure_aligner()
        dev = torch.device("cuda", self._device)
        ids = torch.as_tensor(texts, dtype=torch.int64).to(dev)
        B, L = ids.shape
        mel = torch.as_tensor(mels, dtype=torch.float32).to(dev).contiguous()
        if mel.dim() != 3 or mel.shape[0] != B or mel.shape[2] != self.n_channels:
            raise ValueError(f"expected mels of shape [{B}, T, {self.n_channels}], got {tuple(mel.shape)}")
        T = int(mel.shape[1])
        tl = np.asarray(torch.as_tensor(txt_lens).cpu(), dtype=np.int64).reshape(-1)
        ml = np.asarray(torch.as_tensor(mel_lens).cpu(), dtype=np.int64).reshape(-1)
        sp = torch.as_tensor(speaker, dtype=torch.int64).reshape(-1).to(dev)
        if sp.numel() == 1:
            sp = sp.expand(B)
        keys = emb[ids].contiguous()          # plumbing: the embedding rows are gathered with torch
        spk = spk_table[sp].contiguous()
        if attn_prior is None:
            if tl.shape != (B,) or ml.shape != (B,) or (tl < 1).any() or (tl > L).any() or (ml < 1).any() or (ml > T).any():
                raise ValueError("txt_lens must lie in [1, L] and mel_lens in [1, T], one per row")
            attn_prior = al.batch_prior(tl, ml, T, L)
        prior = self._prior_argument(attn_prior, dev)
        soft = torch.empty((B, T, L), dtype=torch.float32, device=dev)
        hard, logprob = torch.empty_like(soft), torch.empty_like(soft)
        dur = torch.empty((B, L), dtype=torch.float32, device=dev)
        enc.encoder.align(mel, keys, spk, tl, ml, prior, out_dur=dur, out_hard=hard, out_attn=soft, out_logprob=logprob, want=())
        return soft.unsqueeze(1), hard.unsqueeze(1), dur, logprob.unsqueeze(1)

    @staticmethod
    def _prior_argument(attn_prior, dev):
        """What ``Aligner.align`` takes as its prior: "device" as it is (generated there), anything else as a float32 tensor on the GPU."""
        if isinstance(attn_prior, str):
            if attn_prior != "device":
                raise ValueError(f"attn_prior must be None, a [B, T, L] array, or 'device' (got {attn_prior!r})")
            return attn_prior
        return _torch().as_tensor(attn_prior, dtype=_torch().float32).to(dev).contiguous()

    def set_audio_config(self, audio: Mapping[str, object]):
        """The ``audio`` section of the reference's preprocessing configuration (``stft.filter_length / hop_length / win_length``,
        ``mel.channels / mel_fmin / mel_fmax``, ``signal.sampling_rate``): what ``align_audio`` builds its transform from."""
        if int(audio["mel"]["channels"]) != self.n_channels:
            raise ValueError(f"audio.mel.channels = {audio['mel']['channels']}, this model has {self.n_channels} mel channels")
        au = self._full_config["audio"]
        for sec in ("stft", "mel", "signal"):
            au[sec].update(audio[sec])
        self._audio_given, self._stft = True, None
        return self

    def _default_stft(self):
        au = self._full_config["audio"]
        if not getattr(self, "_audio_given", False) and (au["signal"]["sampling_rate"], au["stft"]["hop_length"]) != (22050, 256):
            raise ValueError(f"this model was built with sampling_rate {au['signal']['sampling_rate']} and hop_length {au['stft']['hop_length']}, for which no "
                             "filter_length / mel_fmin / mel_fmax is known: call set_audio_config(audio) or pass stft=")
        stft = getattr(self, "_stft", None)
        if stft is None or stft.frontend.device != self._device:
            stft = self._stft = TorchSTFT(au["stft"]["filter_length"], au["stft"]["hop_length"], au["stft"]["win_length"], self.n_channels,
                                          au["signal"]["sampling_rate"], au["mel"]["mel_fmin"], au["mel"]["mel_fmax"], device=self._device)
        return stft

    def align_audio(self, speaker, texts, txt_lens, wavs, wav_lens, attn_prior=None, return_energy=False, stft=None, wav_rate=None, condition=None):
        """Forced alignment of RECORDINGS: wavs [B, n] (float32 in [-1, 1] or int16 PCM; numpy or torch, host or GPU), wav_lens [B] samples
        -> ``align``'s tuple (attn_soft, attn_hard, attn_hard_dur, attn_logprob), plus the frame energies [B, T] when ``return_energy``.
        The mel is computed on the device by the mel library, every row over its own length (mel_lens = wav_lens // hop, as
        e2emel_forward returns them), and the aligner reads it where it lies: the mel never visits the host.  ``stft`` is a ``TorchSTFT``
        to use (e.g. one holding librosa's own filterbank); by default one is built from this model's audio configuration with
        ``mel.mel_filterbank`` (see its docstring: unpinned against librosa) -- the shipped 22.05 kHz defaults, or what
        ``set_audio_config`` was given; a model built with another sampling rate or hop and no audio configuration raises instead of
        guessing a transform.  ``wav_rate``: the sampling rate of ``wavs`` when it is not the transform's (studio recordings are usually 44.1
        or 48 kHz): the recordings are converted to the transform's rate on the device (e2e_tts_amd.resample, default filter), the mel
        library reads the result where it lies, and mel_lens follow from the converted lengths ceil(wav_lens * L / M).  None: the
        recordings are taken to be at the transform's rate, as before.  ``condition``: ``dict(trim=None | "reference" | "both",
        loudness_dBFS=None | dB, channels=1 | 2)`` prepares the recordings first as the reference's normalize_signal does
        (e2e_tts_amd.condition; unpinned against pydub, see there), on the device and in its order: downmix ([B, n, 2] or [B, 2 n]
        interleaved frames, wav_lens in frames), rate, silence trim, loudness; wav_lens and mel_lens then follow from the kept samples.
        Conditioning works on int16 PCM: with ``wav_rate`` it takes the resampler's int16 output, float32 ``wavs`` at the transform's own
        rate raise ValueError.  None: today's path, bit for bit.  ``attn_prior``: as for ``align``; with "device" the mel lengths the mel
        front-end returned go straight to the aligner, which generates the prior in its attention pass."""
        out, energy, _ = self._align_audio(speaker, texts, txt_lens, wavs, wav_lens, attn_prior, return_energy, stft, wav_rate, condition)
        return out + (energy,) if return_energy else out

    def _conditioned(self, wavs, wl, stft, wav_rate, condition):
        """``align_audio``'s recordings through downmix, rate, trim and loudness -> (int16 rows in the conditioner's HBM, their lengths,
        the stream the mel library has to wait for)."""
        from .condition import Conditioner, loudness_gain
        cond = dict(condition)
        trim, loud, channels = cond.pop("trim", None), cond.pop("loudness_dBFS", None), int(cond.pop("channels", 1))
        if cond:
            raise ValueError(f"condition: unknown keys {sorted(cond)} (trim, loudness_dBFS, channels)")
        if channels not in (1, 2):
            raise ValueError(f"condition: channels must be 1 or 2 (got {channels})")
        rate = int(stft.sampling_rate)
        resampling = wav_rate is not None and int(wav_rate) != rate
        cache = self.__dict__.setdefault("_conditioners", {})
        if (rate, self._device) not in cache:
            cache[(rate, self._device)] = Conditioner(rate, device=self._device)
        c = cache[(rate, self._device)]
        after = None
        if channels == 2:
            if not isinstance(wavs, np.ndarray) and not hasattr(wavs, "data_ptr"):
                wavs = np.asarray(wavs)
            if "int16" not in str(wavs.dtype):
                raise ValueError("condition: the downmix works on int16 PCM")
            c.downmix(wavs, fetch=False)
            x, after = c.resident_mono(), c.hip_stream()
        else:
            x = stft._audio(wavs)
        if resampling:
            from .resample import Resampler
            rcache = self.__dict__.setdefault("_resamplers", {})
            key = (int(wav_rate), rate, self._device)
            if key not in rcache:
                rcache[key] = Resampler(key[0], key[1], device=self._device)
            rsm = rcache[key]
            if after:
                rsm.order_after_stream(after)
            wl = rsm.forward(x, n_valid=wl, want=())["n_out"]
            x, after = rsm.resident()[1], rsm.hip_stream()          # the int16 output
        elif "int16" not in str(x.dtype):
            raise ValueError("condition: conditioning works on int16 PCM; float32 recordings are taken only with wav_rate (the resampler's int16 output)")
        if after:
            c.order_after_stream(after)
        a = c.analyze(x, wl, trim)
        gain = np.ones(len(wl), np.float64)
        if loud is not None:
            gain = np.array([loudness_gain(int(s), int(n), loud) for s, n in zip(a["sumsq"], a["n_out"])], np.float64)
        c.apply(gain, want=("pcm",), fetch=False)
        return c.resident()[0], a["n_out"].astype(np.int64), c.hip_stream()

    def _recording_input(self, wavs, wl, stft, wav_rate, condition):
        """The samples the mel front-end of ``stft`` is handed for recordings ``wavs`` of ``wl`` samples: after ``condition`` and / or
        ``wav_rate`` they lie resident in the stage before, and the front-end's stream is ordered after that stage's.
        -> (samples, their lengths, that stage's stream or None)."""
        fe = stft.frontend
        after = None
        if condition is not None:
            x, wl, after = self._conditioned(wavs, wl, stft, wav_rate, condition)
            fe._call("order_after", after)                          # the mel's stream after the conditioner's
            wav_rate = None
        else:
            x = stft._audio(wavs)
        if wav_rate is not None and int(wav_rate) != int(stft.sampling_rate):
            from .resample import Resampler
            cache = self.__dict__.setdefault("_resamplers", {})
            key = (int(wav_rate), int(stft.sampling_rate), self._device)
            if key not in cache:
                cache[key] = Resampler(key[0], key[1], device=self._device)
            rsm = cache[key]
            wl = rsm.forward(x, n_valid=wl, want=())["n_out"]   # raises ValueError on a bad length before anything is enqueued
            x = rsm.resident()[0]                                # [B, width] float32 in the resampler's HBM, until its next forward
            after = rsm.hip_stream()
            fe._call("order_after", after)                       # the mel's stream after the resampler's
        return x, wl, after

    def recording_features(self, wavs, wav_lens, stft=None, wav_rate=None, condition=None, with_f0=True):
        """Recordings down to mel and f0, through the chain ``align_audio`` uses (``condition``, ``wav_rate``, the mel front-end) and the
        pitch tracker on the same samples, everything left where it lies on the device.  -> (the ``MelFrontend`` holding the log-mel
        [B, T, n_mel] resident, the ``PitchTracker`` holding the f0 track [B, T] resident or None, mel_lens [B] int64): what
        ``compare.Comparator.set_a`` / ``set_b`` take.  Valid until the next call that uses this model's front-end or tracker."""
        torch = _torch()
        if stft is None:
            stft = self._default_stft()
        wl = np.asarray(torch.as_tensor(wav_lens).cpu(), dtype=np.int64).reshape(-1)
        x, wl, after = self._recording_input(wavs, wl, stft, wav_rate, condition)
        fe = stft.frontend
        r = fe.forward(x, wl, want=())
        trk = None
        if with_f0:
            from .f0 import PitchTracker
            key = (int(stft.sampling_rate), int(stft.hop_length), self._device)
            cache = self.__dict__.setdefault("_trackers", {})
            if key not in cache:
                cache[key] = PitchTracker(key[0], key[1], device=self._device)
            trk = cache[key]
            if after:
                trk.order_after_stream(after)
            t = trk.forward(x, wl, want=())
            if t["T"] != r["T"]:
                raise RuntimeError(f"the pitch track has {t['T']} frames, the mel {r['T']}")
        return fe, trk, np.asarray(r["mel_lens"], dtype=np.int64).reshape(-1)

    def _align_audio(self, speaker, texts, txt_lens, wavs, wav_lens, attn_prior, return_energy, stft, wav_rate, condition=None, tap=None):
        """``align_audio``'s work -> (its 4-tuple, the frame energies or None, the mel front-end's mel_lens [B] int64 on the host).
        ``tap``: a dict that receives what the mel front-end was handed -- "x" (the samples, resident in the stage before when there is
        one), "lens", "after" (that stage's stream, or None), "stft" -- for ``forward_audio``'s pitch tracker."""
        from . import aligner as al
        torch = _torch()
        if stft is None:
            stft = self._default_stft()
        enc, emb, spk_table = self._ensure_aligner()
        dev = torch.device("cuda", self._device)
        if stft.n_mel_channels != self.n_channels or stft.frontend.device != self._device:
            raise ValueError(f"stft has {stft.n_mel_channels} mel channels on GPU {stft.frontend.device}; this model has {self.n_channels} on GPU {self._device}")
        ids = torch.as_tensor(texts, dtype=torch.int64).to(dev)
        B, L = ids.shape
        tl = np.asarray(torch.as_tensor(txt_lens).cpu(), dtype=np.int64).reshape(-1)
        sp = torch.as_tensor(speaker, dtype=torch.int64).reshape(-1).to(dev)
        if sp.numel() == 1:
            sp = sp.expand(B)
        keys = emb[ids].contiguous()
        spk = spk_table[sp].contiguous()
        fe = stft.frontend
        wl = np.asarray(torch.as_tensor(wav_lens).cpu(), dtype=np.int64).reshape(-1)
        x, wl, after = self._recording_input(wavs, wl, stft, wav_rate, condition)
        if tap is not None:
            tap.update(x=x, lens=wl, after=after, stft=stft)
        energy = None
        if return_energy:
            energy = torch.zeros((B, max(1, int(wl.max()) // fe.hop)), dtype=torch.float32, device=dev)
        r = fe.forward(x, wl, out_energy=energy, want=())          # raises ValueError on a bad length before anything is enqueued
        T, ml = r["T"], r["mel_lens"]
        if attn_prior is None:
            if tl.shape != (B,) or (tl < 1).any() or (tl > L).any():
                raise ValueError("txt_lens must lie in [1, L], one per row")
            attn_prior = al.batch_prior(tl, ml, T, L)
        prior = self._prior_argument(attn_prior, dev)
        soft = torch.empty((B, T, L), dtype=torch.float32, device=dev)
        hard, logprob = torch.empty_like(soft), torch.empty_like(soft)
        dur = torch.empty((B, L), dtype=torch.float32, device=dev)
        mel_dev, _ = fe.resident()
        a = enc.encoder
        a._check(a.lib.e2ealign_order_after(a._h, fe.stream()), "e2ealign_order_after")   # the aligner's stream after the mel's
        a.align(mel_dev, keys, spk, tl, ml, prior, out_dur=dur, out_hard=hard, out_attn=soft, out_logprob=logprob, want=())
        return (soft.unsqueeze(1), hard.unsqueeze(1), dur, logprob.unsqueeze(1)), energy, np.asarray(ml, dtype=np.int64).reshape(-1)

    def _forced(self, speaker, texts, txt_lens, attn_out, mel_lens, T, p_targets, e_targets, step, after_stream):
        """The engine's teacher-forced pass on an aligner result that lies on the device.  -> the reference's two tuples."""
        import ctypes
        torch = _torch()
        eng = self._ensure_engine()
        dev = torch.device("cuda", self._device)
        soft4, hard4, dur, logprob4 = attn_out
        ids = torch.as_tensor(texts, dtype=torch.int64).contiguous()
        B, L = ids.shape
        lens = torch.as_tensor(txt_lens, dtype=torch.int64).reshape(-1).contiguous()
        spk = torch.as_tensor(speaker, dtype=torch.int64).reshape(-1).contiguous()
        ml = torch.as_tensor(np.asarray(mel_lens, dtype=np.int64))
        ve = self.config["variance"]["variance_embedding"]
        use_uv = bool(ve["use_uv"])
        dm = self.config["variance"]["duration_modelling"]
        soft = int(step) < int(dm["binarization_start_steps"])
        kw = {}
        f32 = lambda v: torch.as_tensor(v, dtype=torch.float32).contiguous()   # noqa: E731
        if p_targets is not None:
            if use_uv != isinstance(p_targets, Mapping):
                raise ValueError("p_targets must be {'f0', 'uv'} for a use_uv model and one tensor otherwise")
            if use_uv:
                kw.update(f0=f32(p_targets["f0"]), uv=f32(p_targets["uv"]))
            else:
                kw.update(pitch=f32(p_targets))
        if e_targets is not None:
            kw.update(energy=f32(e_targets))
        with eng.lock:
            # the engine's stream after the aligner's, as align_audio orders the aligner after the mel (a tuple: after each of them)
            for s in after_stream if isinstance(after_stream, tuple) else (after_stream,):
                if s:
                    eng._check(eng.lib.e2etts_order_after(eng._h, ctypes.c_void_p(s)), "e2etts_order_after")
            r = eng.acoustic_forced(ids, lens, spk, durations=dur.contiguous(), attn_soft=soft4[:, 0].contiguous() if soft else None,
                                    mel_lens=ml if soft else None, pitch_frames=True, energy_frames=True, T=T,
                                    want=("mel_lens", "log_d"), **kw)
            To = r["T"]
            mel = torch.empty((B, To, self.n_channels), dtype=torch.float32, device=dev)
            mel_post = torch.empty_like(mel)
            eng.fetch_mel(B, To, out_mel=mel, out_mel_post=mel_post)
            pf, ef = ve["pitch_feature"] == "frame_level", ve["energy_feature"] == "frame_level"

            def tap(name, shape):   # a tap copied into a tensor on the device: no visit to the host
                t = torch.empty(shape, dtype=torch.float32, device=dev)
                eng.fetch_tap_into(name, t)
                return t

            p_shape = (B, To if pf else L, 2) if use_uv else (B, To if pf else L)
            p_pred, e_pred = tap("pitch_pred", p_shape), tap("energy_pred", (B, To if ef else L))
            p_ret = e_ret = None
            if p_targets is not None:
                pt = tap("pitch_target", p_shape)
                p_ret = {"f0": pt[..., 0].contiguous(), "uv": pt[..., 1].contiguous()} if use_uv else pt
            if e_targets is not None:
                e_ret = tap("energy_target", (B, To if ef else L))
        out_lens = torch.from_numpy(r["mel_lens"]).to(dev)
        lens_d = lens.to(dev)
        txt_masks = torch.arange(L, device=dev)[None, :] >= lens_d[:, None]           # get_mask_from_lengths
        mel_masks = torch.arange(To, device=dev)[None, :] >= out_lens[:, None]
        return ((mel, mel_post, torch.from_numpy(r["log_d"]).to(dev), p_pred, e_pred, lens_d, txt_masks, out_lens, mel_masks,
                 (soft4, hard4, dur, logprob4)), (p_ret, e_ret))

    @staticmethod
    def _check_lengths(txt_lens, mel_lens):
        tl = np.asarray(_torch().as_tensor(txt_lens).cpu(), dtype=np.int64).reshape(-1)
        ml = np.asarray(_torch().as_tensor(mel_lens).cpu(), dtype=np.int64).reshape(-1)
        bad = np.nonzero(ml < tl)[0]
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"row {b}: mel_len {int(ml[b])} < txt_len {int(tl[b])}: the monotonic alignment needs a frame per phoneme")
        return tl, ml

    def forward(self, inputs=None, step=0):
        """The reference's teacher-forced forward in eval() (U/model.py:95-153; what generate_mel calls): ``inputs`` is its 10-tuple
        (speakers, texts, mels [B, T, n_mel], attn_priors (as ``align``'s attn_prior: an array, None or "device"), p_targets, e_targets,
        txt_lens, max_txt_len, mel_lens, max_mel_len) with the
        targets at FRAME level ({"f0", "uv"} of [B, T], or one [B, T] tensor for a model without use_uv; None = embed the prediction).
        -> the reference's two tuples, (mel, mel_post, log_d, pitch_pred, energy_pred, txt_lens, txt_masks, mel_lens, mel_masks, attn_out),
        (p_targets, e_targets) as embedded; attn_out comes from the aligner library, and its soft map and durations are handed to the
        engine where they lie.  step < binarization_start_steps (generate_mel: 0) expands the phonemes with the soft map, else with the
        length regulator on the MAS durations.  Training (no inputs, or train mode) stays out of scope."""
        if inputs is None or self.training:
            raise NotImplementedError("training forward is out of scope; use .inference(), or .align() for the aligner's attn_out")
        speakers, texts, mels, attn_priors, p_targets, e_targets, txt_lens, max_txt_len, mel_lens, max_mel_len = inputs
        torch = _torch()
        ids = torch.as_tensor(texts)
        if max_txt_len is not None and int(max_txt_len) != ids.shape[1]:
            raise ValueError(f"max_txt_len={int(max_txt_len)} != texts.shape[1]={ids.shape[1]}")
        T = int(torch.as_tensor(mels).shape[1])
        if max_mel_len is not None and int(max_mel_len) != T:
            raise ValueError(f"max_mel_len={int(max_mel_len)} != mels.shape[1]={T}")
        _, ml = self._check_lengths(txt_lens, mel_lens)   # before any launch
        attn_out = self.align(speakers, texts, txt_lens, mels, mel_lens, attn_prior=attn_priors)
        return self._forced(speakers, texts, txt_lens, attn_out, ml, T, p_targets, e_targets, step, self._ensure_aligner()[0].encoder.stream())

    __call__ = forward

    def forward_audio(self, speaker, texts, txt_lens, wavs, wav_lens, p_targets=None, e_targets=None, step=0, wav_rate=None, condition=None,
                      attn_prior=None):
        """``align_audio`` followed by the teacher-forced pass: recordings -> ground-truth-aligned mels, with the mel, the soft map and the
        durations never leaving the device.  p_targets / e_targets: frame-level targets [B, T] as for ``forward`` (T = the mel frames of
        the longest recording: max(wav_lens) // hop at the transform's rate).  ``wav_rate``, ``condition``, ``attn_prior``: as for
        ``align_audio`` (with ``condition`` T follows from the kept samples).  ``p_targets="extract"``: the pitch targets are made from the recordings
        themselves, on the device: the pitch tracker (e2e_tts_amd.f0; unpinned against parselmouth, see there) reads the same samples
        the mel front-end reads -- after ``condition`` and / or ``wav_rate`` too --, its track lies on the mel grid, and the data
        loader's targets (``f0_targets`` with this model's stats and pitch_quantization) feed the pass where they lie.  That needs a
        use_uv model: one without takes pyworld's extract_pitch in the reference, which is out of scope, and raises ValueError.
        ``e_targets="extract"``: the energy targets are the data loader's ``(e - mean) / std`` (float32, ``stats["energy"]``) of the frame
        energies the mel front-end has just left resident, made on the device (e2e_tts_amd.stats) and handed to the pass where they
        lie; any other string raises ValueError.
        -> ``forward``'s two tuples.

        How close the teacher-forced ``mel_post`` (the second element of the first tuple, [B, T, n_mel] on the device) is to the
        recording's own mel: both lie on one frame grid, so they are compared frame-synchronously, without a search
        (e2e_tts_amd.compare, mode "sync")::

            out, _ = model.forward_audio(speaker, texts, txt_lens, wavs, wav_lens)
            fe, trk, mel_lens = model.recording_features(wavs, wav_lens)      # the recording's mel (and f0), resident
            cmp = compare.Comparator(n_mel)
            cmp.set_a(fe, mel_lens, trk)
            cmp.set_b(out[1], out[7])                                        # mel_post, mel_lens
            figures = cmp.run(mode="sync")                                   # mcd_db, mel_l1 per utterance

        (``mcd_db`` there is on DCT cepstra of this project's log-mel, see include/e2etts_compare.h.)"""
        tap = None
        extract_p = extract_e = False
        if isinstance(p_targets, str):
            if p_targets != "extract":
                raise ValueError(f"p_targets must be None, targets, or 'extract' (got {p_targets!r})")
            if not self.config["variance"]["variance_embedding"]["use_uv"]:
                raise ValueError("p_targets='extract' needs a use_uv model: the targets of a model without come from pyworld's extract_pitch "
                                 "in the reference, which this package does not restate")
            extract_p = True
        if isinstance(e_targets, str):
            if e_targets != "extract":
                raise ValueError(f"e_targets must be None, targets, or 'extract' (got {e_targets!r})")
            es = self.stats.get("energy", {}) if isinstance(self.stats, Mapping) else {}
            if "mean" not in es or "std" not in es:
                raise ValueError("e_targets='extract' needs stats['energy']['mean'] and ['std'] (models.build_stats makes them from recordings)")
            extract_e = True
        if extract_p or extract_e:
            tap = {}
        attn_out, _, ml = self._align_audio(speaker, texts, txt_lens, wavs, wav_lens, attn_prior, False, None, wav_rate, condition, tap=tap)
        self._check_lengths(txt_lens, ml)
        T = int(attn_out[0].shape[2])
        after = self._ensure_aligner()[0].encoder.stream()
        if extract_p:
            p_targets = self._extracted_targets(tap, T)
        if extract_e:
            e_targets, stats_stream = self._extracted_energy(tap["stft"].frontend, ml, T)
            after = (after, stats_stream)
        return self._forced(speaker, texts, txt_lens, attn_out, ml, T, p_targets, e_targets, step, after)

    def _extracted_energy(self, fe, mel_lens, T):
        """The data loader's energy target [B, T] on the device (get_prosody, src/tools/dataloader.py:179-183: ``(e - mean) / std`` in
        float32, 0 beyond each length) from the frame energies the mel front-end's last forward left resident, with this model's
        ``stats["energy"]``.  -> (the target, the stream it is enqueued on: the teacher-forced pass is ordered after it)."""
        from .stats import CorpusStats
        torch = _torch()
        es = self.stats["energy"]
        cache = self.__dict__.setdefault("_stats_handles", {})
        if self._device not in cache:
            cache[self._device] = CorpusStats(device=self._device)
        st = cache[self._device]
        energy = fe.resident()[1]
        if int(energy.shape[1]) != T:
            raise RuntimeError(f"the frame energies have {int(energy.shape[1])} frames, the mel {T}")
        st.order_after_stream(fe.stream())                          # the statistics' stream after the mel's
        out = torch.empty((len(mel_lens), T), dtype=torch.float32, device=torch.device("cuda", self._device))
        st.normalize(energy, mel_lens, float(es["mean"]), float(es["std"]), out=out)
        return out, st.hip_stream()

    def _extracted_targets(self, tap, T):
        """{"f0", "uv"} [B, T] on the device from the samples the mel front-end was handed."""
        from .f0 import PitchTracker
        torch = _torch()
        stft = tap["stft"]
        key = (int(stft.sampling_rate), int(stft.hop_length), self._device)
        cache = self.__dict__.setdefault("_trackers", {})
        if key not in cache:
            cache[key] = PitchTracker(key[0], key[1], device=self._device)
        trk = cache[key]
        if tap["after"]:
            trk.order_after_stream(tap["after"])                   # the tracker's stream after the stage the samples lie in
        r = trk.forward(tap["x"], tap["lens"], want=())
        if r["T"] != T:
            raise RuntimeError(f"the pitch track has {r['T']} frames, the mel {T}")
        dev = torch.device("cuda", self._device)
        B = len(tap["lens"])
        f0 = torch.empty((B, T), dtype=torch.float32, device=dev)
        uv = torch.empty((B, T), dtype=torch.float32, device=dev)
        ve = self.config["variance"]["variance_embedding"]
        trk.targets(self.stats, ve["pitch_quantization"], out_f0=f0, out_uv=uv)
        return {"f0": f0, "uv": uv}


def build_stats(model, batches, wav_rate=None, condition=None) -> dict:
    """``stats.json`` of a corpus of recordings (the reference's ``TextMelLoader.build_stats``, src/tools/dataloader.py:106-151): every
    ``(wavs, wav_lens)`` of ``batches`` goes through ``model.recording_features`` and its frame energies and f0 are accumulated on the
    device (``stats.CorpusStats.add_recordings``).  -> ``CorpusStats.result()``; it does not depend on how the corpus was batched."""
    from .stats import CorpusStats
    st = CorpusStats(device=model._device)
    try:
        for wavs, wav_lens in batches:
            st.add_recordings(model, wavs, wav_lens, wav_rate=wav_rate, condition=condition)
        return st.result()
    finally:
        st.close()


def f0_targets(f0_hz, stats: Mapping[str, object], pitch_quantization: str = "linear", pitch_eps: float = 0.000000001):
    """A recording's f0 track in Hz (0 = unvoiced) -> (f0 target, uv target) as the reference's data loader makes them (get_f0,
    src/tools/dataloader.py:185-196): uv = f0 == 0; f0 normalised with stats["f0"] -- or log2(f0 + pitch_eps) for pitch_quantization
    "log" --; unvoiced stretches filled by linear interpolation between their voiced neighbours (np.interp: constant beyond the first and
    the last voiced frame), an all-unvoiced track set to 0.  The Hz track comes from ``extract_f0`` below (the pitch library,
    e2e_tts_amd.f0: Boersma's autocorrelation method restated, unpinned against the parselmouth the reference calls) or from any
    extractor of the caller's; ``PitchTracker.targets`` computes the same on the device.
    -> (f0 in the input's float dtype, uv float32), numpy arrays of one utterance [T]."""
    f0 = np.array(f0_hz, copy=True)
    if f0.ndim != 1:
        raise ValueError(f"f0_targets takes one utterance's track [T], got shape {f0.shape}")
    if f0.dtype.kind != "f":
        f0 = f0.astype(np.float64)
    uv = f0 == 0
    f0 = np.log2(f0 + pitch_eps) if pitch_quantization == "log" else (f0 - stats["f0"]["mean"]) / stats["f0"]["std"]
    if sum(uv) == len(f0):
        f0[uv] = 0
    elif sum(uv) > 0:
        f0[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], f0[~uv])
    return f0, uv.astype(np.float32)


_TRACKER_CACHE = {}
# f0_to_coarse's constants (src/tools/utils.py:15-19)
_F0_BIN, _F0_MIN, _F0_MAX = 256, 50.0, 1100.0


def f0_to_coarse(f0):
    """The reference's f0_to_coarse (src/tools/utils.py:81-90), restated: Hz -> mel-scaled bins 1 .. 255 (np.rint, then a plain integer
    cast where the reference uses the retired ``np.int``)."""
    f0 = np.asarray(f0, np.float64)
    mel_min, mel_max = 1127 * np.log(1 + _F0_MIN / 700), 1127 * np.log(1 + _F0_MAX / 700)
    f0_mel = 1127 * np.log(1 + f0 / 700)
    f0_mel[f0_mel > 0] = (f0_mel[f0_mel > 0] - mel_min) * (_F0_BIN - 2) / (mel_max - mel_min) + 1
    f0_mel[f0_mel <= 1] = 1
    f0_mel[f0_mel > _F0_BIN - 1] = _F0_BIN - 1
    return np.rint(f0_mel).astype(np.int64)


def extract_f0(wav_data, mel_len: int, sample_rate: int, hop_length: int, with_pitch: bool = False, device=None):
    """The reference's ``extract_f0`` (src/tools/utils.py:46-78) for one utterance, on the pitch library: wav_data [n] (float in [-1, 1]
    or int16 PCM) -> the f0 track in Hz [mel_len] float64, 0 = unvoiced (and ``f0_to_coarse`` of it with ``with_pitch``).  The reference
    calls parselmouth and then truncates and pads its track onto the mel length; here the track is computed on the mel grid (frame t is
    centred where mel frame t of ``TorchSTFT`` is), so it has floor(n / hop_length) frames by construction: ``mel_len`` must be that
    number, and nothing is padded.  Unpinned against parselmouth (e2e_tts_amd.f0)."""
    from .f0 import PitchTracker
    x = np.asarray(wav_data)
    if x.ndim != 1:
        raise ValueError(f"extract_f0 takes one utterance [n], got shape {x.shape}")
    if x.dtype != np.int16:
        x = x.astype(np.float32)
    frames = x.shape[0] // int(hop_length)
    if int(mel_len) != frames:
        raise ValueError(f"mel_len = {int(mel_len)}, but {x.shape[0]} samples at hop {int(hop_length)} are {frames} mel frames")
    key = (int(sample_rate), int(hop_length), _device_index(device))
    if key not in _TRACKER_CACHE:
        _TRACKER_CACHE[key] = PitchTracker(*key[:2], device=key[2])
    f0 = _TRACKER_CACHE[key].forward(x[None])["f0"][0].astype(np.float64)
    return (f0, f0_to_coarse(f0)) if with_pitch else f0


class AlignmentEncoder:
    """Mirror of the reference's ``AlignmentEncoder`` (U/layers.py:275-369) on the alignment library: same constructor arguments,
    ``load_state_dict`` with the submodule's key names, ``forward(queries [B, C, T1], keys [B, C2, T2], mask, attn_prior, speaker_embed)``
    -> ``(attn, attn_logprob)``, both [B, 1, T1, T2] torch tensors on the GPU.  ``mask`` is the reference's [B, T2, 1] boolean mask (True =
    padded); it must be a prefix mask (get_mask_from_lengths), which is what the library takes as lengths."""

    def __init__(self, n_mel_channels: int, n_att_channels: int, n_text_channels: int, temperature: float, device=None):
        from . import aligner as al
        self.n_mel_channels, self.n_att_channels, self.n_text_channels = int(n_mel_channels), int(n_att_channels), int(n_text_channels)
        self.temperature = temperature
        self.encoder = al.Aligner(n_mel_channels, n_att_channels, n_text_channels, temperature, _device_index(device))
        self.training = False

    def load_state_dict(self, state_dict: Mapping[str, object], strict: bool = True):
        dims = packer.aligner_dims(state_dict, "")
        if dims != (self.n_mel_channels, self.n_att_channels, self.n_text_channels):
            raise ValueError(f"state dict is of an AlignmentEncoder{dims}, this one is "
                             f"{(self.n_mel_channels, self.n_att_channels, self.n_text_channels)}")
        self.encoder.load_weights(packer.pack_aligner(state_dict, ""))
        return self

    def eval(self):
        return self

    def forward(self, queries, keys, mask=None, attn_prior=None, speaker_embed=None):
        torch = _torch()
        dev = torch.device("cuda", self.encoder.device)
        q = torch.as_tensor(queries, dtype=torch.float32).to(dev).transpose(1, 2).contiguous()   # channels-last, the library's layout
        k = torch.as_tensor(keys, dtype=torch.float32).to(dev).transpose(1, 2).contiguous()
        B, T, L = q.shape[0], q.shape[1], k.shape[1]
        lens = None
        if mask is not None:
            m = torch.as_tensor(mask).reshape(B, L).bool().cpu()
            lens = (~m).sum(1).to(torch.int64)
            if not torch.equal(m, torch.arange(L)[None, :] >= lens[:, None]):
                raise ValueError("mask must be a prefix mask (True from each row's length on)")
            lens = lens.numpy()
        prior = None if attn_prior is None else torch.as_tensor(attn_prior, dtype=torch.float32).to(dev).contiguous()
        spk = None if speaker_embed is None else torch.as_tensor(speaker_embed, dtype=torch.float32).to(dev).contiguous()
        attn = torch.empty((B, T, L), dtype=torch.float32, device=dev)
        logprob = torch.empty_like(attn)
        self.encoder.forward(q, k, spk, lens, prior, out_attn=attn, out_logprob=logprob, want=())
        return attn.unsqueeze(1), logprob.unsqueeze(1)

    __call__ = forward


_MAS_HANDLES = {}


def b_mas(attn, in_lens, out_lens, width: int = 1, device=None):
    """The reference's ``b_mas`` (U/function.py:128-137) on the GPU: attn [B, 1, T, L] probabilities (numpy, as the reference takes it, or a
    torch tensor) -> attn_hard of the same kind and shape.  ``width`` must be 1, as there."""
    if width != 1:
        raise NotImplementedError("b_mas: width != 1 is out of scope (the reference asserts width == 1)")
    from . import aligner as al
    torch = _torch()
    is_np = isinstance(attn, np.ndarray)
    if device is None and not is_np and attn.is_cuda:
        device = attn.device
    idx = _device_index(device)
    if idx not in _MAS_HANDLES:
        _MAS_HANDLES[idx] = al.Aligner(4, 1, 4, 1.0, idx)   # the search needs no weights: any dims do
    a = torch.as_tensor(attn, dtype=torch.float32)
    if a.dim() != 4 or a.shape[1] != 1:
        raise ValueError(f"expected attn of shape [B, 1, T, L], got {tuple(a.shape)}")
    a3 = a[:, 0].contiguous()
    a3 = a3.numpy() if not a3.is_cuda else a3
    to_np = lambda v: np.asarray(torch.as_tensor(v).cpu(), dtype=np.int64).reshape(-1)  # noqa: E731
    if is_np or not attn.is_cuda:
        hard = _MAS_HANDLES[idx].mas(a3, to_np(in_lens), to_np(out_lens), want=("attn_hard",))["attn_hard"][:, None]
        return hard.astype(attn.dtype) if is_np else torch.from_numpy(hard)
    hard = torch.empty_like(a3)
    _MAS_HANDLES[idx].mas(a3, to_np(in_lens), to_np(out_lens), out_hard=hard, want=())
    return hard.unsqueeze(1)


def _vocoder_only_dims(hifigan_config: dict, n_mel: int = 80, vocoder: str = "hifigan") -> EngineDims:
    cfg = default_config()
    cfg["models"][vocoder] = hifigan_config
    cfg["audio"]["mel"]["channels"] = n_mel
    hop = 1
    for r in hifigan_config["upsample_rates"]:
        hop *= r
    if vocoder == "istft":
        hop *= hifigan_config["gen_istft_hop_size"]
    cfg["audio"]["stft"]["hop_length"] = hop
    from .config import DEFAULT_STATS
    return dims_from_config(cfg, DEFAULT_STATS, n_speakers=1, vocoder=vocoder)


class HifiGan(_EngineBacked):
    def __init__(self, config: dict, device=None, _shared: Optional[_EngineBacked] = None):
        """``config`` is the ``models.hifigan`` sub-dictionary (reference V/generator.py:14)."""
        super().__init__()
        self.config = config
        self.num_kernels = len(config["resblock_kernel_sizes"])
        self.num_upsamples = len(config["upsample_rates"])
        self._dims_cache = _vocoder_only_dims(config)
        self._device = _device_index(device)

    def _dims(self) -> EngineDims:
        return self._dims_cache

    def _pack(self, state) -> np.ndarray:
        return packer.pack(self._dims_cache, None, state)

    def remove_weight_norm(self):
        """No-op: weight norm is folded when the checkpoint is packed (reference V/generator.py:55-62)."""
        return None

    def bfloat16(self):
        """The reference module's ``.bfloat16()``: the engine's vocoder precision "bf16_act" (every activation bf16, rounded where that
        module rounds; include/e2etts.h).  ``forward`` then takes a bf16 or fp32 mel and returns a bf16 tensor.  Returns self."""
        if self._engine is not None:
            self._engine.set_precision("bf16_act")   # ValueError for a geometry it does not serve; the engine keeps its mode
        self._bf16, self._fp16 = True, False
        return self

    def half(self):
        """The reference module's ``.half()``: the engine's vocoder precision "fp16_act" (every activation fp16, rounded where that module
        rounds; include/e2etts.h).  ``forward`` then takes an fp16 or fp32 mel and returns a ``torch.float16`` tensor.  Returns self."""
        if self._engine is not None:
            self._engine.set_precision("fp16_act")   # ValueError for a geometry it does not serve; the engine keeps its mode
        self._bf16, self._fp16 = False, True
        return self

    def float(self):
        """Back to the reference's fp32 arithmetic (precision "fp32").  Returns self."""
        if self._engine is not None:
            self._engine.set_precision("fp32")
        self._bf16 = self._fp16 = False
        return self

    def _ensure_engine(self) -> Engine:
        fresh = self._engine is None
        eng = super()._ensure_engine()
        if fresh and getattr(self, "_bf16", False):
            eng.set_precision("bf16_act")
        if fresh and getattr(self, "_fp16", False):
            eng.set_precision("fp16_act")
        return eng

    def forward(self, x):
        """x [B, 80, T] (torch tensor, any device, or numpy) -> wav [B, 1, T * hop] on the GPU (V/generator.py:37-53); after ``bfloat16()``
        the wav is a bf16 tensor, after ``half()`` an fp16 one (the engine's wav values are bf16 / fp16 values: the cast is exact)."""
        torch = _torch()
        eng = self._ensure_engine()
        dev = torch.device("cuda", self._device)
        x = torch.as_tensor(x).to(torch.float32).contiguous()   # a bf16 or fp16 mel widens exactly
        if x.dim() != 3 or x.shape[1] != self._dims_cache.n_mel:
            raise ValueError(f"expected mel of shape [B, {self._dims_cache.n_mel}, T], got {tuple(x.shape)}")
        B, _, T = x.shape
        wav = torch.empty((B, T * self._dims_cache.hop_length), dtype=torch.float32, device=dev)
        eng.vocoder(x, B, T, channels_first=True, out_wav=wav)
        if getattr(self, "_bf16", False):
            wav = wav.to(torch.bfloat16)
        if getattr(self, "_fp16", False):
            wav = wav.to(torch.float16)
        return wav.unsqueeze(1)

    __call__ = forward


class iSTFT(HifiGan):
    """Mirror of reference ``models.vocoder.iSTFT`` (V/generator.py:65-118; iSTFTNet): same constructor,
    ``load_state_dict`` / ``eval`` / ``to`` / ``remove_weight_norm``, ``forward(x) -> (spec, phase)``.

    ``inference(x)`` additionally returns the waveform the reference obtains with ``inverse_stft(spec, phase, n_fft, hop,
    win)`` (src/tools/stft.py:138-148) -- on the engine the exp / sin heads, the per-frame inverse DFT, the window and the
    overlap-add are one tail after conv_post, so the waveform needs no second call.  ResBlock selection reproduces the
    reference's comparison with the string '1' (V/generator.py:71): the shipped yaml's integer 1 selects ResBlock2."""

    def __init__(self, config: dict, device=None):
        _EngineBacked.__init__(self)
        self.config = config
        self.num_kernels = len(config["resblock_kernel_sizes"])
        self.num_upsamples = len(config["upsample_rates"])
        self.post_n_fft = config["gen_istft_n_fft"]
        self._dims_cache = _vocoder_only_dims(config, vocoder="istft")
        self._device = _device_index(device)

    def bfloat16(self):
        raise NotImplementedError("bf16 activations (precision 'bf16_act') serve the HiFi-GAN tail only, not the iSTFT tail")

    def half(self):
        raise NotImplementedError("fp16 activations (precision 'fp16_act') serve the HiFi-GAN tail only, not the iSTFT tail")

    def _run(self, x):
        torch = _torch()
        eng = self._ensure_engine()
        dev = torch.device("cuda", self._device)
        x = torch.as_tensor(x, dtype=torch.float32).contiguous()
        if x.dim() != 3 or x.shape[1] != self._dims_cache.n_mel:
            raise ValueError(f"expected mel of shape [B, {self._dims_cache.n_mel}, T], got {tuple(x.shape)}")
        B, _, T = x.shape
        wav = torch.empty((B, T * self._dims_cache.hop_length), dtype=torch.float32, device=dev)
        eng.vocoder(x, B, T, channels_first=True, out_wav=wav)
        return eng, B, T, wav

    def forward(self, x):
        """x [B, 80, T] -> (spec [B, n_fft/2 + 1, F], phase [B, n_fft/2 + 1, F]) on the GPU, F = T * prod(upsample_rates) + 1."""
        torch = _torch()
        up = 1
        for r in self.config["upsample_rates"]:
            up *= r
        with self._ensure_engine().lock:  # the tap belongs to this vocoder call
            eng, B, T, _ = self._run(x)
            F, bins = T * up + 1, self.post_n_fft // 2 + 1
            sp = torch.empty((B, F, 2 * bins), dtype=torch.float32, device=torch.device("cuda", self._device))
            eng.fetch_tap_into("istft_spec_phase", sp)
        sp = sp.transpose(1, 2)
        return sp[:, :bins, :], sp[:, bins:, :]

    __call__ = forward

    def inference(self, x):
        """x [B, 80, T] -> wav [B, 1, T * hop] (= inverse_stft(*forward(x)))."""
        return self._run(x)[3].unsqueeze(1)


class Denoiser:
    """Mirror of reference ``models.vocoder.denoiser.Denoiser`` (V/denoiser.py:156-186): same constructor arguments, ``bias_spec``
    [1, filter_length / 2 + 1, 1] and ``forward(audio [B, n], strength=0.1) -> [B, 1, n]``, torch tensors on the engine's GPU.

    ``vocoder`` is a ``HifiGan`` / ``iSTFT`` mirror: the bias is taken from ITS engine's vocoder in its current precision
    (e2etts_denoiser_calibrate) -- mode='zeros' on 88 zero frames, mode='normal' on a standard-normal mel, as the reference draws it.
    Differences from the reference, which runs one padded batch: ``n`` must be a multiple of the hop (vocoder output is), and
    ``forward(audio, strength, n_valid=[...])`` denoises every row alone over its own valid samples (include/e2etts.h: e2etts_denoise)."""

    def __init__(self, vocoder, filter_length: int = 1024, n_overlap: int = 4, win_length: int = 1024, mode: str = "zeros"):
        from . import denoiser as dn
        torch = _torch()
        if mode not in ("zeros", "normal"):
            raise ValueError(f"mode must be 'zeros' or 'normal', got {mode!r}")
        self.filter_length, self.hop_length, self.win_length = int(filter_length), int(filter_length) // int(n_overlap), int(win_length)
        dn.check_geometry(self.filter_length, self.hop_length)
        fwd, inv, win_sq = dn.stft_bases(self.filter_length, self.hop_length, self.win_length)
        self._vocoder = vocoder
        eng = vocoder.engine
        n_mel = eng.dims.n_mel
        mel = None if mode == "zeros" else np.ascontiguousarray(torch.randn((1, n_mel, 88)).numpy()[0].T)
        with eng.lock:
            eng.denoiser_load(fwd, inv, self.filter_length, self.hop_length, dn.engine_window(win_sq, self.filter_length, self.win_length, "hann"))
            bias = eng.denoiser_calibrate(mel, 88)
        self.bias_spec = torch.from_numpy(bias).to(torch.device("cuda", eng.device))[None, :, None]

    def forward(self, audio, strength: float = 0.1, n_valid=None):
        from . import denoiser as dn
        torch = _torch()
        eng = self._vocoder.engine
        dev = torch.device("cuda", eng.device)
        x = torch.as_tensor(audio).to(torch.float32).contiguous()
        if x.dim() != 2:
            raise ValueError(f"expected audio of shape [B, n], got {tuple(x.shape)}")
        B, n = x.shape
        nv = dn.check_lengths([n] * B if n_valid is None else n_valid, n, self.hop_length)
        out = torch.empty((B, n), dtype=torch.float32, device=dev)
        eng.denoise(x, nv, strength, out_wav=out)
        return out.unsqueeze(1)

    __call__ = forward

    def stream(self, mel_chunks, strength: float = 0.1, want_pcm: bool = False, output_rate: Optional[int] = None, source_rate: int = 22050):
        """Generator over channels-last mel chunks [B, n, n_mel] (numpy / torch) on the vocoder's engine: yields numpy pieces
        [B, n_emit * hop] (float32, or int16 with ``want_pcm``) that concatenate to ``forward(vocoder(whole mel), strength)`` bit for bit
        while HBM use stays bounded by the chunk (e2etts_vocoder_stream_begin_denoised).  An EXTENSION: the reference has no stream --
        its Denoiser takes the whole waveform.  B is read from the first chunk; the bases and the bias cannot be replaced (another
        Denoiser on the same vocoder) until the generator is exhausted.  ``output_rate`` (None: the pieces as they are): the denoised fp32
        pieces, at ``source_rate``, go through ``resample.Resampler.stream`` on the same GPU and the pieces yielded are at ``output_rate``
        ([B, n_ready] each; they concatenate to the one-shot conversion of the whole denoised waveform bit for bit)."""
        eng = self._vocoder.engine
        it = iter(mel_chunks)
        first = next(it, None)
        if first is None:
            return
        if len(first.shape) != 3 or int(first.shape[2]) != eng.dims.n_mel:
            raise ValueError(f"expected mel chunks of shape [B, n, {eng.dims.n_mel}], got {tuple(first.shape)}")

        def chunks():
            yield first
            yield from it

        if output_rate is None or int(output_rate) == int(source_rate):
            yield from eng.vocoder_stream(chunks(), int(first.shape[0]), want_pcm=want_pcm, denoise_strength=float(strength))
            return
        from .resample import Resampler
        pieces = eng.vocoder_stream(chunks(), int(first.shape[0]), want_pcm=False, denoise_strength=float(strength))
        yield from Resampler(source_rate, output_rate, device=eng.device).stream(pieces, want_pcm=want_pcm)


class TorchSTFT:
    """Mirror of the reference's ``TorchSTFT`` (e2e_tts/src/tools/stft.py:11-89) on the mel library: same constructor arguments,
    ``mel_basis`` [n_mel, bins] and ``window`` [win_length] attributes (torch tensors on the GPU), ``mel_spectrogram(input_data [B, n],
    center=False, return_energy=False)`` -> log-mel [B, n_mel, T] (and energy [B, T]), torch tensors on the GPU.

    ``mel_basis=`` replaces the filterbank: by default it is ``mel.mel_filterbank``, a restatement of librosa 0.9.2's formula that has not
    been compared against librosa itself (librosa is not available where this project is built); pass librosa's matrix to be sure.
    Differences from the reference: ``input_data`` may be int16 PCM (divided by 32768 on the device); ``n_valid=[...]`` selects the ragged
    form, every row padded, reflected and framed over its own samples (the reference, given one padded batch, reflects at the batch's end);
    only center=False, the reference's default and the only form its callers use, is served."""

    def __init__(self, filter_length: int = 1024, hop_length: int = 256, win_length: int = 1024, n_mel_channels: int = 80, sampling_rate: int = 22050,
                 mel_fmin: float = 0.0, mel_fmax: Optional[float] = 8000.0, device=None, mel_basis=None, clip_val: float = 1e-5):
        from . import mel as mp
        torch = _torch()
        self.sampling_rate, self.n_mel_channels = sampling_rate, int(n_mel_channels)
        self.filter_length, self.hop_length, self.win_length = int(filter_length), int(hop_length), int(win_length)
        self.fmin, self.fmax = mel_fmin, mel_fmax
        pad = int((self.filter_length - self.hop_length) / 2)
        self.stft_pad = (pad, pad)
        self.frontend = mp.MelFrontend(self.filter_length, self.hop_length, self.n_mel_channels, _device_index(device))
        if mel_basis is None:
            mel_basis = mp.mel_filterbank(sampling_rate, self.filter_length, self.n_mel_channels, mel_fmin, mel_fmax)
        basis = np.ascontiguousarray(torch.as_tensor(mel_basis).detach().cpu().numpy(), dtype=np.float32)
        self.frontend.load(mp.dft_basis(self.filter_length, self.win_length), basis, clip_val)
        self.device = torch.device("cuda", self.frontend.device)
        self.mel_basis = torch.from_numpy(basis).to(self.device)
        self.window = torch.hann_window(self.win_length).to(self.device)

    def _audio(self, x):
        """[B, n] float32 or int16, numpy or torch, as the library takes it."""
        torch = _torch()
        if not isinstance(x, np.ndarray) and not hasattr(x, "data_ptr"):
            x = np.asarray(x)
        if str(x.dtype).replace("torch.", "") not in ("float32", "int16"):
            x = x.astype(np.float32) if isinstance(x, np.ndarray) else x.to(torch.float32)
        if x.ndim != 2:
            raise ValueError(f"expected audio of shape [B, n], got {tuple(x.shape)}")
        return x

    def mel_spectrogram(self, input_data, center: bool = False, return_energy: bool = False, n_valid=None):
        if center:
            raise NotImplementedError("center=True is out of scope: the reference's mel_spectrogram defaults to center=False (e2e_tts/src/tools/stft.py:46) "
                                      "after its own reflect padding (:60-64), and so do all its callers")
        torch = _torch()
        x = self._audio(input_data)
        if str(x.dtype).replace("torch.", "") == "float32":   # the reference's two asserts (stft.py:56-57)
            t = torch.as_tensor(x)
            assert torch.min(t) >= -1
            assert torch.max(t) <= 1
        B, n = int(x.shape[0]), int(x.shape[1])
        T = n // self.hop_length if n_valid is None else int(np.asarray(torch.as_tensor(n_valid).cpu()).max()) // self.hop_length
        mel = torch.zeros((B, max(T, 1), self.n_mel_channels), dtype=torch.float32, device=self.device)
        energy = torch.zeros((B, max(T, 1)), dtype=torch.float32, device=self.device) if return_energy else None
        self.frontend.forward(x, n_valid, out_mel=mel, out_energy=energy, want=())
        mel = mel.transpose(1, 2).contiguous()
        return (mel, energy) if return_energy else mel


_STFT_CACHE = {}


def generate_melspecs(y, n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0.0, fmax=8000.0, center=False, device=None):
    """The function form (e2e_tts/src/tools/stft.py:107-135): y [B, n] -> log-mel [B, num_mels, T] on the GPU.  Like the reference it only
    warns about samples outside [-1, 1]; the transform objects are cached per geometry and device."""
    import warnings
    torch = _torch()
    if device is None and hasattr(y, "is_cuda") and y.is_cuda:
        device = y.device
    key = (n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, _device_index(device))
    if key not in _STFT_CACHE:
        _STFT_CACHE[key] = TorchSTFT(n_fft, hop_size, win_size, num_mels, sampling_rate, fmin, fmax, device=device)
    stft = _STFT_CACHE[key]
    if center:
        return stft.mel_spectrogram(y, center=True)   # raises
    x = stft._audio(y)
    t = torch.as_tensor(x)
    if t.dtype == torch.float32:
        if torch.min(t) < -1.:
            warnings.warn(f"min value is {torch.min(t).item()}")
        if torch.max(t) > 1.:
            warnings.warn(f"max value is {torch.max(t).item()}")
    B, n = int(x.shape[0]), int(x.shape[1])
    mel = torch.zeros((B, max(n // hop_size, 1), num_mels), dtype=torch.float32, device=stft.device)
    stft.frontend.forward(x, None, out_mel=mel, want=())
    return mel.transpose(1, 2).contiguous()


class _Discriminators:
    """What the two mirrors below share: one ``critic.Critic`` (both families live in one handle; a mirror made with ``critic=other.critic``
    shares it), the state dicts until both are there, and the reference's ``forward(y, y_hat)``.

    The library loads both families as one blob.  A mirror used ALONE therefore loads the other family with seeded stand-in weights
    (``synth_critic_state(0)``): they cost device memory and the other family's launches, and nothing they compute is returned.  A forward
    runs the whole critic once per side and materialises every map (``Critic.forward``), which come back through the host: the mirrors
    are for parity checks against the reference's classes; ``Critic.run`` is the path for figures.  ``strict`` is accepted for signature
    compatibility; missing or misshapen tensors are always an error (``packer.pack_critic``)."""
    _family = ""

    def __init__(self, config: Optional[dict] = None, device=None, critic=None):
        from . import critic as cr
        self.critic = critic if critic is not None else cr.Critic(config, _device_index(device))
        self.training = False

    def load_state_dict(self, state_dict: Mapping[str, object], strict: bool = True):
        """Weights reach the device once both families' state dicts are known (the library packs them into one blob); a family that is
        never loaded gets a seeded stand-in, so that one mirror can be used alone."""
        self.critic._states[self._family] = state_dict
        self.critic._loaded = False
        return self

    def eval(self):
        return self

    def _load(self):
        c = self.critic
        if not c._loaded:
            from .synth_weights import synth_critic_state
            stand_in = dict(zip(("mpd", "msd"), synth_critic_state(0, c.config)))
            if self._family not in c._states:
                raise RuntimeError(f"{type(self).__name__}: forward before load_state_dict")
            c.load(c._states.get("mpd", stand_in["mpd"]), c._states.get("msd", stand_in["msd"]))

    def forward(self, y, y_hat):
        """y, y_hat [B, 1, T] -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) as the reference returns them: per discriminator the flattened scores
        [B, n] and the list of feature maps [B, C, T', p] / [B, C, T'], torch tensors on the GPU."""
        torch = _torch()
        self._load()
        c = self.critic
        dev = torch.device("cuda", c.device)
        mine = [d for d, t in enumerate(c.tables) if t[0] == self._family]
        out = []
        for x in (y, y_hat):
            x = torch.as_tensor(x, dtype=torch.float32)
            if x.dim() != 3 or x.shape[1] != 1:
                raise ValueError(f"expected samples of shape [B, 1, T], got {tuple(x.shape)}")
            x = x.to(dev).contiguous()
            c.forward(x, np.full(x.shape[0], x.shape[2], np.int64))
            maps = [[torch.from_numpy(c.fmap(d, l)[0]).to(dev) for l in range(len(c.tables[d][2]))] for d in mine]
            out.append(([m[-1].flatten(1, -1) for m in maps], maps))
        return [s for s in out[0][0]], [s for s in out[1][0]], out[0][1], out[1][1]

    __call__ = forward


class MultiPeriodDiscriminator(_Discriminators):
    """Mirror of the reference's ``MultiPeriodDiscriminator`` (V/discriminator.py:6-30) in eval(), on the critic library."""
    _family = "mpd"


class MultiScaleDiscriminator(_Discriminators):
    """Mirror of the reference's ``MultiScaleDiscriminator`` (V/discriminator.py:33-62) in eval(), on the critic library."""
    _family = "msd"
