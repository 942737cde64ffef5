"""CPU restatement of the vocoder precision "bf16_act" (E2ETTS_PRECISION_BF16_ACT, include/e2etts.h): HiFi-GAN with every tensor between
layers in bf16, written from the rounding table of the header, not from the reference.  Helper module for the tests (not collected).

Each convolution is F.conv1d / F.conv_transpose1d on fp32 tensors that hold bf16 values, bias added in the accumulation type, then one
rounding to bf16.  Each elementwise step is computed in fp32 on bf16 values, then rounded.

weights="engine": bf16 of the fp32 weight-norm fold (packer.fold_weight_norm), bf16 biases -- the engine's parameters.
weights="module": torch._weight_norm on bf16 weight_v / weight_g, bf16 biases -- what .bfloat16() gives the reference's module.
acc: the accumulation type of the convolutions (torch.float32, or torch.float64 to estimate the size of accumulation-order flips).
drop: names of rounding points to leave out (a check that the tests notice a missing one): "c1" = the round after c1 + b1.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from e2e_tts_amd import packer

LRELU = 0.1


def r16(x: torch.Tensor) -> torch.Tensor:
    """round to nearest-even bf16, kept as a float32 tensor of bf16 values"""
    return x.to(torch.bfloat16).to(torch.float32)


def lrelu(x: torch.Tensor, slope: float) -> torch.Tensor:
    return torch.where(x >= 0, x, x * slope)


class Bf16ActVocoder:
    def __init__(self, state, hifigan_config: dict, weights: str = "engine", acc=torch.float32, drop=()):
        if weights not in ("engine", "module"):
            raise ValueError(weights)
        self.hg = hifigan_config
        self.acc = acc
        self.drop = set(drop)
        self.w, self.b = {}, {}
        for k in state:
            if not k.endswith(".weight_v"):
                continue
            p = k[: -len(".weight_v")]
            g, v = np.asarray(state[p + ".weight_g"], np.float32), np.asarray(state[k], np.float32)
            if weights == "engine":
                w = r16(torch.from_numpy(packer.fold_weight_norm(g, v)))
            else:
                w = torch._weight_norm(torch.from_numpy(v).bfloat16(), torch.from_numpy(g).bfloat16(), 0).float()
            self.w[p] = w
            self.b[p] = r16(torch.from_numpy(np.asarray(state[p + ".bias"], np.float32)))

    def _conv(self, x, p, **kw):
        return r16(F.conv1d(x.to(self.acc), self.w[p].to(self.acc), self.b[p].to(self.acc), **kw).float())

    def _convt(self, x, p, **kw):
        return r16(F.conv_transpose1d(x.to(self.acc), self.w[p].to(self.acc), self.b[p].to(self.acc), **kw).float())

    def _resblock(self, idx, x, k, dils):
        if int(self.hg.get("resblock", 1)) == 1:
            for m, d in enumerate(dils):
                xt = r16(lrelu(x, LRELU))
                xt = F.conv1d(xt.to(self.acc), self.w[f"resblocks.{idx}.convs1.{m}"].to(self.acc),
                              self.b[f"resblocks.{idx}.convs1.{m}"].to(self.acc), padding=(k * d - d) // 2, dilation=d).float()
                if "c1" not in self.drop:
                    xt = r16(xt)
                xt = r16(lrelu(xt, LRELU))
                xt = self._conv(xt, f"resblocks.{idx}.convs2.{m}", padding=(k - 1) // 2)
                x = r16(xt + x)
        else:
            for m, d in enumerate(dils[:2]):
                xt = r16(lrelu(x, LRELU))
                xt = self._conv(xt, f"resblocks.{idx}.convs.{m}", padding=(k * d - d) // 2, dilation=d)
                x = r16(xt + x)
        return x

    @torch.no_grad()
    def forward(self, mel_btc: np.ndarray) -> np.ndarray:
        """mel [B, T, n_mel] channels-last (fp32 or bf16 values) -> wav [B, T * hop] float32 holding bf16 values"""
        hg = self.hg
        x = r16(torch.from_numpy(np.ascontiguousarray(np.asarray(mel_btc, np.float32).transpose(0, 2, 1))))
        x = self._conv(x, "conv_pre", padding=3)
        nk = len(hg["resblock_kernel_sizes"])
        for i, (u, k) in enumerate(zip(hg["upsample_rates"], hg["upsample_kernel_sizes"])):
            x = r16(lrelu(x, LRELU))
            x = self._convt(x, f"ups.{i}", stride=u, padding=(k - u) // 2)
            xs = None
            for j in range(nk):
                r = self._resblock(i * nk + j, x, hg["resblock_kernel_sizes"][j], hg["resblock_dilation_sizes"][j])
                xs = r if xs is None else r16(xs + r)
            x = r16(xs / nk)
        x = r16(lrelu(x, 0.01))
        x = self._conv(x, "conv_post", padding=3)
        return r16(torch.tanh(x))[:, 0].numpy()
