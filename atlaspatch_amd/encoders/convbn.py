"""Convolution + BatchNorm on the host, shared by the encoders whose checkpoints carry BatchNorm (``resnet``, ``clip_resnet``,
the stem of ``swin``): key names, the four-stage ResNet enumeration, the eval-mode fold into one convolution with bias, and
the seeded random init of a conv + BatchNorm stack.  A layer is ``(name, cout, cin, k, stride)``."""
from __future__ import annotations

import re

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
BN_PARAMS = ("weight", "bias", "running_mean", "running_var")


def bn_name(conv: str) -> str:
    """BatchNorm name of a convolution: conv1 -> bn1, layerX.Y.convK -> layerX.Y.bnK, downsample -> downsample.1"""
    if conv.endswith("downsample"):
        return conv + ".1"
    head, _, last = conv.rpartition(".")
    return (head + "." if head else "") + "bn" + last[len("conv"):]


def conv_key(conv: str) -> str:
    return conv + (".0.weight" if conv.endswith("downsample") else ".weight")


def conv_bn_keys(layers: list) -> dict:
    """{checkpoint key: shape} of the unfolded convolutions and their BatchNorms, in the layers' order."""
    keys = {}
    for name, cout, cin, k, _ in layers:
        keys[conv_key(name)] = (cout, cin, k, k)
        for p in BN_PARAMS:
            keys[f"{bn_name(name)}.{p}"] = (cout,)
    return keys


def stage_layers(width: int, depths, *, bottleneck: bool, stride_in_conv: bool) -> list:
    """The layers of the four stages behind a stem of ``width`` channels, in forward order: ``layer<S>.<B>.conv<K>`` and
    ``downsample`` for the shortcut's projection.  The first block of stages 2..4 has stride 2, on its 3x3 convolution when
    ``stride_in_conv`` (torchvision), else carried by a 2x2 average pool (CLIP: every convolution has stride 1); the
    projection's entry holds the block's stride either way."""
    out = []
    inplanes = width
    for s, depth in enumerate(depths):
        planes = width << s
        outc = planes * 4 if bottleneck else planes
        for b in range(depth):
            stride = 2 if (s > 0 and b == 0) else 1
            conv_stride = stride if stride_in_conv else 1
            pre = f"layer{s + 1}.{b}."
            if bottleneck:
                out += [(pre + "conv1", planes, inplanes, 1, 1), (pre + "conv2", planes, planes, 3, conv_stride),
                        (pre + "conv3", outc, planes, 1, 1)]
            else:
                out += [(pre + "conv1", planes, inplanes, 3, conv_stride), (pre + "conv2", planes, planes, 3, 1)]
            if stride != 1 or inplanes != outc:
                out.append((pre + "downsample", outc, inplanes, 1, stride))
            inplanes = outc
    return out


def fold_conv_bn(canonical: dict, conv: str, bn: str, dtype: torch.dtype, eps: float = BN_EPS):
    """Conv + BatchNorm (eval) -> (W', b') of one convolution with bias, in float32: W' = W g / sqrt(var + eps),
    b' = beta - mean g / sqrt(var + eps).  A folded weight that is not finite in ``dtype`` (or a bias that is not finite) is
    refused."""
    scale = canonical[f"{bn}.weight"] / torch.sqrt(canonical[f"{bn}.running_var"] + eps)
    w = canonical[conv_key(conv)] * scale.view(-1, 1, 1, 1)
    b = canonical[f"{bn}.bias"] - canonical[f"{bn}.running_mean"] * scale
    if not bool(torch.isfinite(w.to(dtype)).all()) or not bool(torch.isfinite(b).all()):
        raise ValueError(f"{conv}: the BatchNorm-folded weights are not finite in {dtype} (max |w'| = "
                         f"{float(w.abs().max()):.3g}); this checkpoint cannot run in that precision")
    return w.contiguous(), b.contiguous()


def fold_layers(canonical: dict, layers: list, dtype: torch.dtype, eps: float = BN_EPS) -> dict:
    """``fold_conv_bn`` of every layer under ``<name>.weight`` / ``<name>.bias``."""
    out = {}
    for name, *_ in layers:
        out[f"{name}.weight"], out[f"{name}.bias"] = fold_conv_bn(canonical, name, bn_name(name), dtype, eps)
    return out


def random_conv_bn(layers: list, depths, last_conv: int, g: torch.Generator) -> dict:
    """Seeded init of the layers, three draws a layer in the layers' order: a He-normal convolution, a BatchNorm gain in
    [0.8, 1.2] -- the last BatchNorm of every block (``conv<last_conv>``) scaled by 1 / sqrt(blocks in its stage) -- and a
    shift of 0.1 N(0, 1).  The running statistics come from ``calibrate_bn``."""
    sd = {}
    for name, cout, cin, k, _ in layers:
        sd[conv_key(name)] = torch.randn(cout, cin, k, k, generator=g) * float(np.sqrt(2.0 / (cin * k * k)))
        gain = 0.8 + 0.4 * torch.rand(cout, generator=g)
        m = re.match(r"layer(\d+)\.\d+\.conv(\d+)$", name)
        if m and int(m.group(2)) == last_conv:
            gain = gain / float(np.sqrt(depths[int(m.group(1)) - 1]))
        sd[f"{bn_name(name)}.weight"] = gain
        sd[f"{bn_name(name)}.bias"] = 0.1 * torch.randn(cout, generator=g)
    return sd


def calibrate_bn(sd: dict, t: torch.Tensor, name: str) -> torch.Tensor:
    """Sets the running statistics of BatchNorm ``name`` to the batch statistics of its input ``t`` (rounded to float16
    precision so that they do not depend on the host's summation order) and returns the normalised tensor."""
    sd[f"{name}.running_mean"] = t.mean(dim=(0, 2, 3)).half().float()
    sd[f"{name}.running_var"] = t.var(dim=(0, 2, 3), unbiased=False).half().float()
    return F.batch_norm(t, sd[f"{name}.running_mean"], sd[f"{name}.running_var"], sd[f"{name}.weight"], sd[f"{name}.bias"],
                        False, 0.0, BN_EPS)
