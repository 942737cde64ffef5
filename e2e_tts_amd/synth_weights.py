"""Deterministic synthetic checkpoints for tests and benchmarks.

No trained checkpoint ships with the reference (its .gitignore excludes *.pt),
so parity and throughput are measured on synthetic weights.
The *manifest* below is this project's own statement of the reference
state-dict layout (SURVEY.md 8(a) "State-dict manifest"); oracle/make_goldens.py
proves it exact by ``load_state_dict(strict=True)`` into the reference modules.

Generator: numpy ``Generator(PCG64(seed))``, tensors drawn in sorted-key order.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np

from .config import N_SYMBOLS

Shape = Tuple[int, ...]


def sinusoid_table(n_position: int, d_hid: int) -> np.ndarray:
    """FFT-block position table: float64 numpy, sin on even / cos on odd columns, cast to fp32.

    Restates reference U/blocks/utils.py:14-34 in vectorised form (same float64
    operations: ``pos / 10000 ** (2 * (j // 2) / d_hid)`` then sin / cos).
    """
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    j = np.arange(d_hid)
    denom = np.power(10000, 2 * (j // 2) / d_hid)
    table = pos / denom[None, :]
    table[:, 0::2] = np.sin(table[:, 0::2])
    table[:, 1::2] = np.cos(table[:, 1::2])
    return table.astype(np.float32)


def acoustic_manifest(config: dict, n_speakers: int, n_symbols: int = N_SYMBOLS) -> "OrderedDict[str, Tuple[Shape, str]]":
    """name -> (shape, kind) for UnsupervisedFastSpeech2.state_dict()."""
    fs = config["models"]["fastspeech2"]
    bt = fs["building_block"]["block_type"]
    tr = fs["building_block"][bt]
    H = fs["encoder_hidden"]
    if bt == "conformer":
        F, k1, k2 = H * tr["ffn_expansion_factor"], tr["conv_kernel_size"], 1
    else:
        F = tr["conv_filter_size"]
        k1, k2 = tr["conv_kernel_size"]
    n_mel = config["audio"]["mel"]["channels"]
    vp = fs["variance"]["variance_predictor"]
    ve = fs["variance"]["variance_embedding"]
    pn = fs["postnet"]
    m: "OrderedDict[str, Tuple[Shape, str]]" = OrderedDict()

    def add(name, shape, kind):
        m[name] = (tuple(shape), kind)

    for side, layers in (("encoder", fs["encoder_layers"]), ("decoder", fs["decoder_layers"])):
        add(f"{side}.position_enc", (1, fs["max_seq_len"] + 1, H), "posenc")
        if side == "encoder":
            add("encoder.src_word_emb.weight", (n_symbols + 1, H), "emb_pad0")
        for l in range(layers if bt == "conformer" else 0):
            # ConformerBlock.state_dict() (U/blocks/conformer.py:214-249): FFN, rel-pos MHSA, conv module, FFN, LayerNorm
            p = f"{side}.layer_stack.{l}.sequential"
            nh = tr[f"{side}_head"]
            for i in (0, 3):
                q = f"{p}.{i}.module.sequential"
                add(f"{q}.0.weight", (H,), "gamma")
                add(f"{q}.0.bias", (H,), "beta")
                add(f"{q}.1.linear.weight", (F, H), "w")
                add(f"{q}.1.linear.bias", (F,), "b")
                add(f"{q}.4.linear.weight", (H, F), "w")
                add(f"{q}.4.linear.bias", (H,), "b")
            q = f"{p}.1.module"
            add(f"{q}.positional_encoding", (1, fs["max_seq_len"] + 1, H), "posenc")  # the side's table, registered again (:330)
            add(f"{q}.layer_norm.weight", (H,), "gamma")
            add(f"{q}.layer_norm.bias", (H,), "beta")
            add(f"{q}.attention.u_bias", (nh, H // nh), "emb")
            add(f"{q}.attention.v_bias", (nh, H // nh), "emb")
            for w in ("query_proj", "key_proj", "value_proj", "pos_proj", "out_proj"):
                add(f"{q}.attention.{w}.linear.weight", (H, H), "w")  # LinearNorm default: no bias (U/blocks/utils.py:182)
            q = f"{p}.2.module.sequential"
            add(f"{q}.0.weight", (H,), "gamma")
            add(f"{q}.0.bias", (H,), "beta")
            add(f"{q}.2.conv.weight", (2 * H, H, 1), "w")
            add(f"{q}.2.conv.bias", (2 * H,), "b")
            add(f"{q}.4.conv.weight", (H, 1, k1), "w")
            add(f"{q}.5.weight", (H,), "gamma")
            add(f"{q}.5.bias", (H,), "beta")
            add(f"{q}.5.running_mean", (H,), "bn_mean")
            add(f"{q}.5.running_var", (H,), "bn_var")
            add(f"{q}.5.num_batches_tracked", (), "i64")
            add(f"{q}.7.conv.weight", (H, H, 1), "w")
            add(f"{q}.7.conv.bias", (H,), "b")
            add(f"{p}.4.weight", (H,), "gamma")
            add(f"{p}.4.bias", (H,), "beta")
        for l in range(layers if bt == "fastformer" else 0):
            # FFTBlock.state_dict() of U/blocks/fastformer.py:144-165: PreNorm(FastAttention), PreNorm(PositionwiseFeedForward) per layer.
            # hidden / n_head heads of size n_head (:152,190-191); the two logit layers of every layer ARE layer 0's modules (:161-165), and
            # state_dict() lists them under each layer's name: "tied" entries repeat layer 0's values
            p = f"{side}.layer_stack.layers.{l}"
            NH = H // tr[f"{side}_head"]
            add(f"{p}.0.norm.weight", (H,), "gamma")
            add(f"{p}.0.norm.bias", (H,), "beta")
            for w in ("query", "key", "transform"):
                add(f"{p}.0.fn.{w}.weight", (H, H), "w")
                add(f"{p}.0.fn.{w}.bias", (H,), "b")
            for w, kind in (("to_q_attn_logits", "ff_qlogit"), ("to_k_attn_logits", "ff_klogit")):
                first = f"{side}.layer_stack.layers.0.0.fn.{w}"
                add(f"{p}.0.fn.{w}.weight", (NH, H), kind if l == 0 else f"tied:{first}.weight")
                add(f"{p}.0.fn.{w}.bias", (NH,), "b" if l == 0 else f"tied:{first}.bias")
            add(f"{p}.1.norm.weight", (H,), "gamma")
            add(f"{p}.1.norm.bias", (H,), "beta")
            add(f"{p}.1.fn.w_1.weight", (F, H, k1), "w")
            add(f"{p}.1.fn.w_1.bias", (F,), "b")
            add(f"{p}.1.fn.w_2.weight", (H, F, k2), "w")
            add(f"{p}.1.fn.w_2.bias", (H,), "b")
        for l in range(0 if bt in ("conformer", "fastformer") else layers):
            p = f"{side}.layer_stack.{l}"
            for w in ("w_qs", "w_ks", "w_vs", "fc"):
                add(f"{p}.slf_attn.{w}.weight", (H, H), "w")
                add(f"{p}.slf_attn.{w}.bias", (H,), "b")
            add(f"{p}.slf_attn.layer_norm.weight", (H,), "gamma")
            add(f"{p}.slf_attn.layer_norm.bias", (H,), "beta")
            add(f"{p}.pos_ffn.w_1.weight", (F, H, k1), "w")
            add(f"{p}.pos_ffn.w_1.bias", (F,), "b")
            add(f"{p}.pos_ffn.w_2.weight", (H, F, k2), "w")
            add(f"{p}.pos_ffn.w_2.bias", (H,), "b")
            add(f"{p}.pos_ffn.layer_norm.weight", (H,), "gamma")
            add(f"{p}.pos_ffn.layer_norm.bias", (H,), "beta")
    va = "variance_adaptor"
    add(f"{va}.pitch_bins", (ve["n_bins"] - 1,), "pitch_bins")
    add(f"{va}.energy_bins", (ve["n_bins"] - 1,), "energy_bins")
    # aligner: unused by synthesis (packer.pack leaves it out); forced alignment packs it into a blob of its own (packer.pack_aligner, U/layers.py:275-369)
    add(f"{va}.aligner.key_proj.0.conv.weight", (2 * H, H, 3), "w")
    add(f"{va}.aligner.key_proj.0.conv.bias", (2 * H,), "b")
    add(f"{va}.aligner.key_proj.2.conv.weight", (n_mel, 2 * H, 1), "w")
    add(f"{va}.aligner.key_proj.2.conv.bias", (n_mel,), "b")
    add(f"{va}.aligner.query_proj.0.conv.weight", (2 * n_mel, n_mel, 3), "w")
    add(f"{va}.aligner.query_proj.0.conv.bias", (2 * n_mel,), "b")
    add(f"{va}.aligner.query_proj.2.conv.weight", (n_mel, 2 * n_mel, 1), "w")
    add(f"{va}.aligner.query_proj.2.conv.bias", (n_mel,), "b")
    add(f"{va}.aligner.query_proj.4.conv.weight", (n_mel, n_mel, 1), "w")
    add(f"{va}.aligner.query_proj.4.conv.bias", (n_mel,), "b")
    add(f"{va}.aligner.key_spk_proj.linear.weight", (H, H), "w")
    add(f"{va}.aligner.query_spk_proj.linear.weight", (n_mel, H), "w")
    dc = n_mel  # duration predictor width = mel channels (U/layers.py:39)
    for i in range(vp["dur_predictor_layers"]):
        cin = H if i == 0 else dc
        add(f"{va}.duration_predictor.conv.{i}.1.weight", (dc, cin, vp["dur_predictor_kernel"]), "w")
        add(f"{va}.duration_predictor.conv.{i}.1.bias", (dc,), "b")
        add(f"{va}.duration_predictor.conv.{i}.3.weight", (dc,), "gamma")
        add(f"{va}.duration_predictor.conv.{i}.3.bias", (dc,), "beta")
    add(f"{va}.duration_predictor.linear.weight", (1, dc), "dur_w")
    add(f"{va}.duration_predictor.linear.bias", (1,), "dur_b")
    vc = vp["filter_size"]
    for which, odim, layers, kern in (("pitch", 2 if ve["use_uv"] else 1, vp["pit_predictor_layers"], vp["pit_predictor_kernel"]),
                                      ("energy", 1, vp["ener_predictor_layers"], vp["ener_predictor_kernel"])):
        p = f"{va}.{which}_predictor"
        add(f"{p}.pos_embed_alpha", (1,), "alpha")
        for i in range(layers):
            cin = H if i == 0 else vc
            add(f"{p}.conv.{i}.1.weight", (vc, cin, kern), "w")
            add(f"{p}.conv.{i}.1.bias", (vc,), "b")
            add(f"{p}.conv.{i}.3.weight", (vc,), "gamma")
            add(f"{p}.conv.{i}.3.bias", (vc,), "beta")
        pb = "pitch_b" if ve["use_uv"] and ve["pitch_quantization"] != "log" else ("pitch_b_log" if ve["use_uv"] else "pitch_b_nouv")
        add(f"{p}.linear.weight", (odim, vc), f"{which}_w")
        add(f"{p}.linear.bias", (odim,), pb if which == "pitch" else f"{which}_b")
        add(f"{p}.embed_positions._float_tensor", (1,), "zero")
        rows = ve["n_bins"] if (which == "energy" or ve["use_uv"]) else ve["f0_bins"]   # U/layers.py:60-63
        add(f"{va}.{which}_embedding.weight", (rows, H), "emb")
    add("mel_linear.weight", (n_mel, H), "w")
    add("mel_linear.bias", (n_mel,), "b")
    P = pn["embedding_dim"]
    for i in range(pn["conv_layers"]):
        cin = n_mel if i == 0 else P
        cout = n_mel if i == pn["conv_layers"] - 1 else P
        p = f"postnet.convolutions.{i}"
        add(f"{p}.0.conv.weight", (cout, cin, pn["kernel_size"]), "w")
        add(f"{p}.0.conv.bias", (cout,), "b")
        add(f"{p}.1.weight", (cout,), "gamma")
        add(f"{p}.1.bias", (cout,), "beta")
        add(f"{p}.1.running_mean", (cout,), "bn_mean")
        add(f"{p}.1.running_var", (cout,), "bn_var")
        add(f"{p}.1.num_batches_tracked", (), "i64")
    add("speaker_emb.weight", (n_speakers, H), "emb")
    return m


def vocoder_manifest(config: dict, vocoder: str = "hifigan") -> "OrderedDict[str, Tuple[Shape, str]]":
    """name -> (shape, kind) for HifiGan.state_dict() / iSTFT.state_dict() (weight-normed: weight_g / weight_v).

    ``vocoder="istft"``: reference V/generator.py:65-94 -- same trunk from ``config["models"]["istft"]``, conv_post with
    n_fft + 2 output channels, and ResBlock2 (``resblocks.N.convs.{0,1}``) unless ``resblock == '1'`` (the string; :71)."""
    hg = config["models"][vocoder]
    n_mel = config["audio"]["mel"]["channels"]
    C0 = hg["upsample_initial_channel"]
    rb1 = (hg["resblock"] == "1") if vocoder == "istft" else (hg["resblock"] == 1)
    m: "OrderedDict[str, Tuple[Shape, str]]" = OrderedDict()

    def add_wn(prefix, vshape, kind="wn"):
        m[f"{prefix}.bias"] = ((vshape[0],) if kind != "wn_t" else (vshape[1],), "b")
        m[f"{prefix}.weight_g"] = ((vshape[0], 1, 1), "wn_g")
        m[f"{prefix}.weight_v"] = (tuple(vshape), kind)

    add_wn("conv_pre", (C0, n_mel, 7))
    ch = C0
    for i, (u, k) in enumerate(zip(hg["upsample_rates"], hg["upsample_kernel_sizes"])):
        add_wn(f"ups.{i}", (C0 // 2 ** i, C0 // 2 ** (i + 1), k), kind="wn_t")
    nk = len(hg["resblock_kernel_sizes"])
    for i in range(len(hg["upsample_rates"])):
        ch = C0 // 2 ** (i + 1)
        for j, (k, dil) in enumerate(zip(hg["resblock_kernel_sizes"], hg["resblock_dilation_sizes"])):
            if rb1:
                for cs in ("convs1", "convs2"):
                    for d in range(len(dil)):
                        add_wn(f"resblocks.{i * nk + j}.{cs}.{d}", (ch, ch, k))
            else:
                for d in range(2):
                    add_wn(f"resblocks.{i * nk + j}.convs.{d}", (ch, ch, k))
    add_wn("conv_post", ((hg["gen_istft_n_fft"] + 2) if vocoder == "istft" else 1, ch, 7))
    return m


def _draw(rng: np.random.Generator, name: str, shape: Shape, kind: str, *, stats: dict, mode: str,
          frames_per_phoneme: int) -> np.ndarray:
    f32 = np.float32
    if kind == "i64":
        return np.zeros(shape, dtype=np.int64)
    if kind == "zero":
        return np.zeros(shape, dtype=f32)
    if kind == "posenc":
        return sinusoid_table(shape[1], shape[2])[None]
    if kind in ("w", "wn"):
        fan_in = int(np.prod(shape[1:]))
        return (rng.standard_normal(shape) * (1.0 / math.sqrt(fan_in))).astype(f32)
    if kind in ("ff_qlogit", "ff_klogit"):
        # Fastformer logit layers: scaled so that the logits are of order 1 and the sequence softmaxes are far from uniform (the module's own
        # init, std 0.02, would leave them flat and a parity test blind).  The key logits see k * pooled_query, a few times smaller than q
        fan_in = shape[-1]
        return (rng.standard_normal(shape) * ((2.0 if kind == "ff_qlogit" else 6.0) / math.sqrt(fan_in))).astype(f32)
    if kind.startswith("tied:"):
        return None  # copied from the named tensor after the draw (no random numbers consumed)
    if kind == "wn_t":  # ConvTranspose1d weight [Cin, Cout, k]; each output sees Cin * k / stride taps
        fan_in = shape[0] * 2
        return (rng.standard_normal(shape) * (1.0 / math.sqrt(fan_in))).astype(f32)
    if kind == "wn_g":
        return None  # filled after weight_v (needs its norm)
    if kind == "b":
        return (0.05 * rng.standard_normal(shape)).astype(f32)
    if kind == "gamma":
        return (1.0 + 0.1 * rng.standard_normal(shape)).astype(f32)
    if kind == "beta":
        return (0.1 * rng.standard_normal(shape)).astype(f32)
    if kind == "bn_mean":
        return (0.1 * rng.standard_normal(shape)).astype(f32)
    if kind == "bn_var":
        return (1.0 + 0.1 * rng.random(shape)).astype(f32)
    if kind == "emb":
        return (0.3 * rng.standard_normal(shape)).astype(f32)
    if kind == "emb_pad0":
        w = rng.standard_normal(shape).astype(f32)
        w[0] = 0.0  # padding_idx row (U/blocks/transformer.py:41-43)
        return w
    if kind == "alpha":
        return np.ones(shape, dtype=f32)
    if kind == "dur_w":
        w = rng.standard_normal(shape)
        return ((0.06 * w) if mode == "varied" else (0.0 * w)).astype(f32)
    if kind == "dur_b":
        rng.standard_normal(shape)  # keep the stream aligned between modes
        if mode == "varied":
            return np.full(shape, math.log(4.6), dtype=f32)
        # exp(b) - 1 == frames_per_phoneme + 0.25: far from a rounding boundary
        return np.full(shape, math.log(frames_per_phoneme + 1.25), dtype=f32)
    if kind in ("pitch_w", "energy_w"):
        fan_in = shape[-1]
        return (rng.standard_normal(shape) * (0.4 / math.sqrt(fan_in))).astype(f32)
    if kind == "pitch_b":
        b = (0.05 * rng.standard_normal(shape)).astype(f32)
        b[-1] -= 0.8  # bias the uv logit towards "voiced" so the f0 buckets are exercised
        return b
    if kind == "pitch_b_log":   # f0 = 2 ** prediction: centre the f0 channel on log2(190 Hz)
        b = (0.05 * rng.standard_normal(shape)).astype(f32)
        b[0] += 7.57
        b[-1] -= 0.8
        return b
    if kind == "pitch_b_nouv":  # one output bucketized on pitch_bins (stats "pitch" min .. max): centre it inside the range
        return (4.0 + 0.05 * rng.standard_normal(shape)).astype(f32)
    if kind == "energy_b":
        return (2.5 + 0.05 * rng.standard_normal(shape)).astype(f32)
    if kind == "pitch_bins":   # (the reference's "log" variant needs positive stats; the synthetic ones are not: linear bins)
        return np.linspace(stats["pitch"]["min"], stats["pitch"]["max"], shape[0]).astype(f32)
    if kind == "energy_bins":
        return np.linspace(stats["energy"]["min"], stats["energy"]["max"], shape[0]).astype(f32)
    raise KeyError(kind)


def _fill(manifest, seed: int, **kw) -> Dict[str, np.ndarray]:
    rng = np.random.Generator(np.random.PCG64(seed))
    out: Dict[str, np.ndarray] = {}
    for name in sorted(manifest):
        shape, kind = manifest[name]
        out[name] = _draw(rng, name, shape, kind, **kw)
    for name in manifest:
        if manifest[name][1].startswith("tied:"):
            out[name] = out[manifest[name][1][len("tied:"):]].copy()
    # weight_g = ||v|| * (1 + 0.1 N) over all dims but 0 (weight_norm dim=0; V/generator.py:18,23,33)
    for name in sorted(manifest):
        if manifest[name][1] == "wn_g":
            v = out[name[: -len("weight_g")] + "weight_v"].astype(np.float64)
            norm = np.sqrt((v * v).sum(axis=(1, 2), keepdims=True))
            out[name] = (norm * (1.0 + 0.1 * rng.standard_normal(norm.shape))).astype(np.float32)
    return OrderedDict((k, out[k]) for k in manifest)


def make_acoustic_state(config: dict, stats: dict, n_speakers: int, seed: int = 1234, mode: str = "fixed",
                        frames_per_phoneme: int = 6, n_symbols: int = N_SYMBOLS) -> "OrderedDict[str, np.ndarray]":
    """mode='fixed': exactly ``frames_per_phoneme`` frames per real phoneme (benchmarks);
    mode='varied': data-dependent durations of roughly 1..9 frames (correctness fixtures)."""
    return _fill(acoustic_manifest(config, n_speakers, n_symbols), seed, stats=stats, mode=mode,
                 frames_per_phoneme=frames_per_phoneme)


def make_aligner_state(hidden: int, n_mel: int, n_speakers: int = 4, seed: int = 77, n_symbols: int = N_SYMBOLS,
                       weight_scale: float = 1.0) -> "OrderedDict[str, np.ndarray]":
    """The tensors forced alignment reads, alone and at any widths: ``variance_adaptor.aligner.*`` (the AlignmentEncoder of
    U/layers.py:275-369, n_att_channels = n_mel), ``encoder.src_word_emb.weight`` and ``speaker_emb.weight``, under their checkpoint names.
    ``weight_scale`` multiplies the aligner's weight matrices (not its biases): random weights at the shipped temperature give nearly flat
    attention, and a fixture that wants a decided alignment without a prior sharpens it this way (tools/make_aligner_goldens.py)."""
    va = "variance_adaptor.aligner."
    m: "OrderedDict[str, Tuple[Shape, str]]" = OrderedDict()
    m["encoder.src_word_emb.weight"] = ((n_symbols + 1, hidden), "emb_pad0")
    m["speaker_emb.weight"] = ((n_speakers, hidden), "emb")
    for name, shape in (("key_proj.0.conv", (2 * hidden, hidden, 3)), ("key_proj.2.conv", (n_mel, 2 * hidden, 1)),
                        ("query_proj.0.conv", (2 * n_mel, n_mel, 3)), ("query_proj.2.conv", (n_mel, 2 * n_mel, 1)),
                        ("query_proj.4.conv", (n_mel, n_mel, 1))):
        m[f"{va}{name}.weight"] = (shape, "w")
        m[f"{va}{name}.bias"] = ((shape[0],), "b")
    m[f"{va}key_spk_proj.linear.weight"] = ((hidden, hidden), "w")
    m[f"{va}query_spk_proj.linear.weight"] = ((n_mel, hidden), "w")
    sd = _fill(m, seed, stats=None, mode="fixed", frames_per_phoneme=0)
    if weight_scale != 1.0:
        for k in sd:
            if k.startswith(va) and k.endswith("weight"):
                sd[k] = (sd[k] * np.float32(weight_scale)).astype(np.float32)
    return sd


def make_vocoder_state(config: dict, seed: int = 4321, vocoder: str = "hifigan") -> "OrderedDict[str, np.ndarray]":
    sd = _fill(vocoder_manifest(config, vocoder), seed, stats=None, mode="fixed", frames_per_phoneme=0)
    # keep the pre-tanh signal in the unsaturated range so waveform parity is informative (iSTFT: log-magnitudes of O(1))
    sd["conv_post.weight_g"] = (sd["conv_post.weight_g"] * 0.25).astype(np.float32)
    return sd


def to_torch(state: Dict[str, np.ndarray]):
    import torch

    return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in state.items())


def synth_critic_state(seed: int = 2024, config=None):
    """(state_mpd, state_msd): seeded state dicts of the reference's MultiPeriodDiscriminator / MultiScaleDiscriminator under their own key
    names, at the widths of ``config`` (e2e_tts_amd.critic.default_config()).  One PCG64 stream per state dict (seed, seed + 1), drawn in
    sorted-key order: weight_v / weight_orig ~ N(0, 2 / (1.01 fan_in)) with fan_in = Cin / groups * k (He for leaky ReLU 0.1), bias =
    0.05 N, weight_g = ||v|| (1 + 0.1 N).  The first scale discriminator is spectral-normed: its weight_u / weight_v are the singular
    vectors 30 power iterations in float64 reach from the all-ones vector (no draw).  This scaling keeps every feature map's RMS within a
    decade of 0.1; with torch's default init the scale discriminators overflow float32."""
    from .critic import default_config, disc_tables
    cfg = default_config() if config is None else config
    states = {"mpd": OrderedDict(), "msd": OrderedDict()}
    shapes = {"mpd": {}, "msd": {}}
    for kind, idx, layers in disc_tables(cfg):
        cin = 1
        for l, (cout, k, s, g, pad) in enumerate(layers):
            prefix = f"discriminators.{idx}." + ("conv_post" if l == len(layers) - 1 else f"convs.{l}")
            wshape = (cout, cin // g, k, 1) if kind == "mpd" else (cout, cin // g, k)
            spectral = kind == "msd" and idx == 0
            shapes[kind][prefix + ".bias"] = ((cout,), "b")
            if spectral:
                shapes[kind][prefix + ".weight_orig"] = (wshape, "w")
            else:
                shapes[kind][prefix + ".weight_v"] = (wshape, "w")
                shapes[kind][prefix + ".weight_g"] = ((cout,) + (1,) * (len(wshape) - 1), "g")
            cin = cout
    for n, kind in enumerate(("mpd", "msd")):
        rng = np.random.Generator(np.random.PCG64(seed + n))
        out = states[kind]
        for name in sorted(shapes[kind]):
            shape, what = shapes[kind][name]
            z = rng.standard_normal(shape)
            if what == "w":
                fan_in = int(np.prod(shape[1:]))
                out[name] = (z * np.sqrt(2.0 / (1.01 * fan_in))).astype(np.float32)
            elif what == "b":
                out[name] = (0.05 * z).astype(np.float32)
            else:
                out[name] = z   # weight_g: finished below, from its weight_v
        for name in sorted(shapes[kind]):
            if shapes[kind][name][1] == "g":
                v = out[name[: -len("weight_g")] + "weight_v"].astype(np.float64)
                norm = np.sqrt((v * v).reshape(v.shape[0], -1).sum(1)).reshape(out[name].shape)
                out[name] = (norm * (1.0 + 0.1 * out[name])).astype(np.float32)
            elif name.endswith(".weight_orig"):
                W = out[name].astype(np.float64).reshape(out[name].shape[0], -1)
                u = np.ones(W.shape[0]) / np.sqrt(W.shape[0])
                for _ in range(30):
                    v = W.T @ u
                    v /= max(np.linalg.norm(v), 1e-12)
                    u = W @ v
                    u /= max(np.linalg.norm(u), 1e-12)
                out[name[: -len("weight_orig")] + "weight_u"] = u.astype(np.float32)
                out[name[: -len("weight_orig")] + "weight_v"] = v.astype(np.float32)
        states[kind] = OrderedDict((k, out[k]) for k in sorted(out))
    return states["mpd"], states["msd"]
