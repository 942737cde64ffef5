"""CPU restatement of the vocoder precisions with 16-bit activations -- "fp16_act" (E2ETTS_PRECISION_FP16_ACT) and "bf16_act" -- with the
element type as a parameter: HiFi-GAN with every tensor between layers in that type, written from the rounding tables of
include/e2etts.h, not from the reference.  Helper module for the tests (not collected).

Each convolution is F.conv1d / F.conv_transpose1d on fp32 tensors that hold 16-bit values, bias added in the accumulation type, then one
rounding to the element type (nearest-even, overflow to infinity, subnormals kept: torch's cast).  Each elementwise step is computed in
fp32 on 16-bit values, then rounded.

dtype: torch.float16 or torch.bfloat16.
weights="engine": the element type of the fp32 weight-norm fold (packer.fold_weight_norm), rounded once; rounded biases -- the engine's.
weights="module": torch._weight_norm on weight_v / weight_g cast to the element type -- what .half() / .bfloat16() gives the module.
acc: the accumulation type of the convolutions (torch.float32, or torch.float64 to estimate the size of accumulation-order flips).
drop: names of rounding points to leave out (a check that the tests notice a missing one): "c1" = the round after c1 + b1.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from e2e_tts_amd import packer

LRELU = 0.1


def lrelu(x: torch.Tensor, slope: float) -> torch.Tensor:
    return torch.where(x >= 0, x, x * slope)


class Act16Vocoder:
    def __init__(self, state, hifigan_config: dict, dtype=torch.float16, weights: str = "engine", acc=torch.float32, drop=()):
        if weights not in ("engine", "module"):
            raise ValueError(weights)
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(dtype)
        self.hg = hifigan_config
        self.dtype = dtype
        self.acc = acc
        self.drop = set(drop)
        self.w, self.b = {}, {}
        for k in state:
            if not k.endswith(".weight_v"):
                continue
            p = k[: -len(".weight_v")]
            g, v = np.asarray(state[p + ".weight_g"], np.float32), np.asarray(state[k], np.float32)
            if weights == "engine":
                w = self.r(torch.from_numpy(packer.fold_weight_norm(g, v)))
            else:
                w = torch._weight_norm(torch.from_numpy(v).to(dtype), torch.from_numpy(g).to(dtype), 0).float()
            self.w[p] = w
            self.b[p] = self.r(torch.from_numpy(np.asarray(state[p + ".bias"], np.float32)))

    def r(self, x: torch.Tensor) -> torch.Tensor:
        """round to the nearest element-type value (ties to even), kept as a float32 tensor"""
        return x.to(self.dtype).to(torch.float32)

    def _conv(self, x, p, **kw):
        return self.r(F.conv1d(x.to(self.acc), self.w[p].to(self.acc), self.b[p].to(self.acc), **kw).float())

    def _convt(self, x, p, **kw):
        return self.r(F.conv_transpose1d(x.to(self.acc), self.w[p].to(self.acc), self.b[p].to(self.acc), **kw).float())

    def _resblock(self, idx, x, k, dils):
        r = self.r
        if int(self.hg.get("resblock", 1)) == 1:
            for m, d in enumerate(dils):
                xt = r(lrelu(x, LRELU))
                xt = F.conv1d(xt.to(self.acc), self.w[f"resblocks.{idx}.convs1.{m}"].to(self.acc),
                              self.b[f"resblocks.{idx}.convs1.{m}"].to(self.acc), padding=(k * d - d) // 2, dilation=d).float()
                if "c1" not in self.drop:
                    xt = r(xt)
                xt = r(lrelu(xt, LRELU))
                xt = self._conv(xt, f"resblocks.{idx}.convs2.{m}", padding=(k - 1) // 2)
                x = r(xt + x)
        else:
            for m, d in enumerate(dils[:2]):
                xt = r(lrelu(x, LRELU))
                xt = self._conv(xt, f"resblocks.{idx}.convs.{m}", padding=(k * d - d) // 2, dilation=d)
                x = r(xt + x)
        return x

    @torch.no_grad()
    def forward(self, mel_btc: np.ndarray) -> np.ndarray:
        """mel [B, T, n_mel] channels-last -> wav [B, T * hop] float32 holding element-type values"""
        hg, r = self.hg, self.r
        x = r(torch.from_numpy(np.ascontiguousarray(np.asarray(mel_btc, np.float32).transpose(0, 2, 1))))
        x = self._conv(x, "conv_pre", padding=3)
        nk = len(hg["resblock_kernel_sizes"])
        for i, (u, k) in enumerate(zip(hg["upsample_rates"], hg["upsample_kernel_sizes"])):
            x = r(lrelu(x, LRELU))
            x = self._convt(x, f"ups.{i}", stride=u, padding=(k - u) // 2)
            xs = None
            for j in range(nk):
                rb = self._resblock(i * nk + j, x, hg["resblock_kernel_sizes"][j], hg["resblock_dilation_sizes"][j])
                xs = rb if xs is None else r(xs + rb)
            x = r(xs / nk)
        x = r(lrelu(x, 0.01))
        x = self._conv(x, "conv_post", padding=3)
        return r(torch.tanh(x))[:, 0].numpy()


GEOMETRY_KEYS = ("resblock", "upsample_rates", "upsample_kernel_sizes", "upsample_initial_channel", "resblock_kernel_sizes",
                 "resblock_dilation_sizes")


def fixture_case(g, tag: str):
    """(config, vocoder state, mel [B, T, 80]) of case `tag` of fixture hifigan_fp16 (tools/make_fp16_goldens.py): the geometry and the
    weight seed come from the file."""
    from e2e_tts_amd import config as cfgmod, synth_weights as sw
    cfg = cfgmod.default_config()
    hg = cfg["models"]["hifigan"]
    for k in GEOMETRY_KEYS:
        v = g[f"{tag}.{k}"]
        hg[k] = v.tolist() if v.ndim else int(v)
    hop = int(g[f"{tag}.hop"])
    cfg["audio"]["stft"]["hop_length"] = hop
    if hop == 512:
        cfg["audio"]["signal"]["sampling_rate"] = 48000
    return cfg, sw.make_vocoder_state(cfg, seed=int(g[f"{tag}.weight_seed"])), g[f"{tag}.mel"]
