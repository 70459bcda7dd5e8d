"""CHIEF-CTransPath encoder on the native HIP kernels (models/patch/chief_ctranspath.py of the reference).

The reference builds timm ``swin_tiny_patch4_window7_224`` with a convolutional stem (``ConvStem``: two 3x3 stride-2
convolutions with BatchNorm + ReLU, a 1x1 projection to 96 channels, LayerNorm) and ``head = Identity``, and returns the mean
over the 49 tokens of the final LayerNorm's output (768-d).  Preprocessing is ``Resize(224)`` on the PIL tile -- Pillow
BILINEAR resize of the shorter side to 224, no crop -- then ``ToTensor`` and ImageNet normalisation; through the device front
end that is ``resize=(224, "bilinear")`` followed by the (no-op) centre crop of 224.

Here the shifted-window attention and the patch merging + LayerNorm run in ``swin.hip``, the LayerNorms in ``convnext.hip`` and
every linear layer and the stem in ``conv.hip``'s implicit GEMM, behind ``ap_swin_*``.  BatchNorm is folded into the stem's
convolutions on the host (f32).  Checkpoints come as a bare dict or wrapped in ``{"model": ...}``, in one of three layouts,
all detected:

* current timm keys (``layers.{1,2,3}.downsample.*`` at the head of a stage) -- the canonical form;
* the original CTransPath checkpoint (``layers.{0,1,2}.downsample.*`` at the end of a stage), which the reference renames at
  lines 142-151;
* transformers ``SwinModel`` keys for the stages (``encoder.layers.S.blocks.J.attention.{q,k,v,o}_proj`` ..., an optional
  ``swin.`` prefix stripped) beside the stem's ``patch_embed.proj.*`` keys.

``relative_position_index``, ``attn_mask``, ``num_batches_tracked``, ``head.*`` and ``classifier.*`` are dropped.

The name is not in ``build_default_registry``: it is registered by ``register_chief_ctranspath``, which the shipped plugin
``atlaspatch_amd/plugins/chief_ctranspath.py`` calls (``--feature-plugin``).
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Optional

import numpy as np
import torch

from .. import _lib
from . import convbn
from .base import HipViTFeatureExtractor, NativeEncoder
from .checkpoints import IMAGENET_MEAN, IMAGENET_STD, _env_seed, check_canonical, resolve_weights

LN_EPS = 1e-5
BN_EPS = convbn.BN_EPS
WINDOW = 7
TRANSFORM_RESIZE = (224, "bilinear")      # transforms.Resize(224) on the PIL tile

ARCHS = {
    "chief-ctranspath": {"depths": (2, 2, 6, 2), "heads": (3, 6, 12, 24), "embed_dim": 96},
}
DEFAULTS = {"window": WINDOW, "image_size": 224}
MAX_BATCH = 256         # device batch: the four activation buffers at 256 tiles are 1.1 GB in float16

_BN = convbn.BN_PARAMS
_STEM_BN = {"patch_embed.proj.0": "patch_embed.proj.1", "patch_embed.proj.3": "patch_embed.proj.4"}


def _spec(arch) -> dict:
    spec = dict(DEFAULTS)
    spec.update(ARCHS[arch] if isinstance(arch, str) else arch)
    return spec


def canonical_keys(arch) -> dict:
    """{timm key: shape} of the unfolded checkpoint without the head, in forward order."""
    spec = _spec(arch)
    e = int(spec["embed_dim"])
    keys = {"patch_embed.proj.0.weight": (e // 8, 3, 3, 3)}
    keys.update({f"patch_embed.proj.1.{p}": (e // 8,) for p in _BN})
    keys["patch_embed.proj.3.weight"] = (e // 4, e // 8, 3, 3)
    keys.update({f"patch_embed.proj.4.{p}": (e // 4,) for p in _BN})
    keys.update({"patch_embed.proj.6.weight": (e, e // 4, 1, 1), "patch_embed.proj.6.bias": (e,),
                 "patch_embed.norm.weight": (e,), "patch_embed.norm.bias": (e,)})
    for s, depth in enumerate(spec["depths"]):
        c = e << s
        if s > 0:
            d = f"layers.{s}.downsample."
            keys.update({d + "norm.weight": (2 * c,), d + "norm.bias": (2 * c,), d + "reduction.weight": (c, 2 * c)})
        for j in range(depth):
            p = f"layers.{s}.blocks.{j}."
            keys.update({p + "norm1.weight": (c,), p + "norm1.bias": (c,),
                         p + "attn.qkv.weight": (3 * c, c), p + "attn.qkv.bias": (3 * c,),
                         p + "attn.relative_position_bias_table": ((2 * WINDOW - 1) ** 2, spec["heads"][s]),
                         p + "attn.proj.weight": (c, c), p + "attn.proj.bias": (c,),
                         p + "norm2.weight": (c,), p + "norm2.bias": (c,),
                         p + "mlp.fc1.weight": (4 * c, c), p + "mlp.fc1.bias": (4 * c,),
                         p + "mlp.fc2.weight": (c, 4 * c), p + "mlp.fc2.bias": (c,)})
    keys.update({"norm.weight": (e << 3,), "norm.bias": (e << 3,)})
    return keys


_DROPPED = ("relative_position_index", "attn_mask", "num_batches_tracked")
_HF_PART = {"layernorm_before": "norm1", "layernorm_after": "norm2", "attention.o_proj": "attn.proj",
            "mlp.fc1": "mlp.fc1", "mlp.fc2": "mlp.fc2"}
_HF_BLOCK = re.compile(r"^encoder\.layers\.(\d+)\.blocks\.(\d+)\.(.+)$")
_HF_DOWN = re.compile(r"^encoder\.layers\.(\d+)\.downsample\.(norm\.weight|norm\.bias|reduction\.weight)$")
_HF_TABLE = "attention.relative_position_bias.relative_position_bias_table"


def detect_source(sd: dict) -> str:
    keys = list(sd)
    if any(k.startswith(("encoder.layers.", "swin.encoder.")) for k in keys):
        return "hf"
    if any(k.startswith("layers.0.downsample.") for k in keys):
        return "ctranspath"
    if any(k.startswith("layers.") for k in keys):
        return "timm"
    raise ValueError("Swin checkpoint: neither timm keys (layers.S.blocks.J.*) nor transformers SwinModel keys "
                     f"(encoder.layers.S.blocks.J.*) found; first keys: {keys[:5]}")


def _hf_to_timm(sd: dict):
    """transformers SwinModel stage keys -> timm keys; q / k / v projections are gathered and concatenated.  Returns
    (renamed dict, unknown keys)."""
    out, unknown, qkv = {}, [], {}
    for key, value in sd.items():
        k = key[len("swin."):] if key.startswith("swin.") else key
        if k.startswith(("patch_embed.", "norm.")):
            out[k] = value
        elif k.startswith("embeddings.norm."):
            out["patch_embed.norm." + k[len("embeddings.norm."):]] = value
        elif k.startswith("layernorm."):
            out["norm." + k[len("layernorm."):]] = value
        elif _HF_DOWN.match(k):
            s, rest = _HF_DOWN.match(k).groups()
            out[f"layers.{int(s) + 1}.downsample.{rest}"] = value       # the end of stage s = the head of stage s + 1
        elif _HF_BLOCK.match(k):
            s, j, rest = _HF_BLOCK.match(k).groups()
            pre = f"layers.{int(s)}.blocks.{int(j)}."
            part, _, param = rest.rpartition(".")
            if rest == _HF_TABLE:
                out[pre + "attn.relative_position_bias_table"] = value
            elif part in ("attention.q_proj", "attention.k_proj", "attention.v_proj") and param in ("weight", "bias"):
                qkv.setdefault((pre, param), {})[part[-6]] = value
            elif part in _HF_PART and param in ("weight", "bias"):
                out[pre + _HF_PART[part] + "." + param] = value
            else:
                unknown.append(key)
        else:
            unknown.append(key)
    for (pre, param), parts in qkv.items():
        if set(parts) == {"q", "k", "v"}:
            out[pre + "attn.qkv." + param] = torch.cat([torch.as_tensor(parts[x]) for x in "qkv"], 0)
    return out, unknown


def canonical_state_dict(sd: dict, *, arch="chief-ctranspath", source: str = "auto") -> dict:
    """The checkpoint as unfolded float32 tensors under current timm keys (``canonical_keys``).  ``source``: "timm",
    "ctranspath" (the original checkpoint: ``layers.{0,1,2}.downsample`` renamed to ``layers.{1,2,3}``), "hf" (transformers
    ``SwinModel`` keys for the stages) or "auto".  A ``{"model": ...}`` wrapper is opened; buffers and the head are dropped;
    any other unknown key, a missing key or a wrong shape is a ``ValueError``."""
    if isinstance(sd.get("model"), dict):
        sd = sd["model"]
    sd = {k: v for k, v in sd.items()
          if not any(d in k for d in _DROPPED) and not k.startswith(("head.", "classifier."))}
    if source == "auto":
        source = detect_source(sd)
    if source not in ("timm", "ctranspath", "hf"):
        raise ValueError(f"unknown Swin checkpoint layout {source!r}")
    want = canonical_keys(arch)
    unknown = []
    if source == "hf":
        sd, unknown = _hf_to_timm(sd)
    out = {}
    for key, value in sd.items():
        name = key
        if source == "ctranspath":
            m = re.match(r"^layers\.(\d+)\.downsample\.(.+)$", name)
            if m:
                name = f"layers.{int(m.group(1)) + 1}.downsample.{m.group(2)}"
        if name not in want:
            unknown.append(key)
            continue
        out[name] = torch.as_tensor(value).detach().to(torch.float32).cpu().contiguous()
    return check_canonical(out, want, unknown, family="Swin", source=source)


def fold_batchnorm(canonical: dict, *, arch="chief-ctranspath", dtype: torch.dtype = torch.float32, eps: float = BN_EPS) -> dict:
    """The parameters ``ap_swin_set_param`` takes: every key but the stem's BatchNorms, with each folded into the convolution
    in front of it in float32 (W' = W g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)).  A folded weight that is not
    finite in ``dtype`` is refused."""
    bn_keys = {f"{bn}.{p}" for bn in _STEM_BN.values() for p in _BN}
    out = {k: canonical[k] for k in canonical_keys(arch) if k not in bn_keys}
    for conv, bn in _STEM_BN.items():
        out[f"{conv}.weight"], out[f"{conv}.bias"] = convbn.fold_conv_bn(canonical, conv, bn, dtype, eps)
    return out


def expand_relative_bias(table: torch.Tensor, window: int = WINDOW) -> torch.Tensor:
    """``relative_position_bias_table`` [(2w-1)^2, heads] -> the bias of every token pair, float32 [heads, w^2, w^2]:
    B_h[i, j] = table[(yi - yj + w - 1) (2w - 1) + (xi - xj + w - 1), h] with token i = w yi + xi."""
    t = torch.arange(window * window)
    y, x = t // window, t % window
    index = (y[:, None] - y[None, :] + window - 1) * (2 * window - 1) + (x[:, None] - x[None, :] + window - 1)
    table = torch.as_tensor(table).to(torch.float32)
    return table[index.reshape(-1)].reshape(window * window, window * window, -1).permute(2, 0, 1).contiguous()


def random_canonical_state_dict(arch="chief-ctranspath", seed: int = 0) -> dict:
    """Seeded, well-conditioned random weights in canonical (timm, unfolded) form.  Every convolution / linear layer is scaled
    to unit output variance for unit input and LayerNorm / BatchNorm gains lie near 1 with small shifts, so every block's two
    branches add a visible share of the residual stream and activations stay O(1), far inside float16's range.  The bias
    tables are N(0, 1) -- a wrong index changes the features -- and the BatchNorm running variances lie in [0.5, 1.5], not 1."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for k, shape in canonical_keys(arch).items():
        if k.endswith("relative_position_bias_table"):
            sd[k] = torch.randn(shape, generator=g)
        elif len(shape) > 1:
            sd[k] = torch.randn(shape, generator=g) / float(np.sqrt(int(np.prod(shape[1:]))))
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith((".bias", "running_mean")):
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        else:                                           # LayerNorm / BatchNorm gains
            sd[k] = 0.8 + 0.4 * torch.rand(shape, generator=g)
    return {k: sd[k].contiguous() for k in canonical_keys(arch)}


# ----------------------------------------------------------------------------- device object
class HipSwin(NativeEncoder):
    """Device-resident Swin behind ``ap_swin_*``."""

    ABI = "swin"
    PROF_KINDS = _lib.SWIN_PROF_KINDS

    def __init__(self, arch, folded: dict, *, device: torch.device, dtype: torch.dtype) -> None:
        self._bind(device, dtype)
        spec = _spec(arch)
        self._open(_lib.SwinConfig((C.c_int * 4)(*spec["depths"]), (C.c_int * 4)(*spec["heads"]), int(spec["embed_dim"]),
                                   int(spec["window"]), _lib.torch_dtype_code(dtype), int(spec["image_size"])), folded)
        self.embed_dim = int(self.lib.ap_swin_embed_dim(self._handle))


# ----------------------------------------------------------------------------- builders
def build_hip_swin_extractor(*, name: str = "chief-ctranspath", arch="chief-ctranspath", device, dtype,
                             state_dict: Optional[dict] = None, source: str = "auto", mean=None, std=None,
                             max_batch: int = MAX_BATCH, random_init_seed: Optional[int] = None) -> HipViTFeatureExtractor:
    """A CTransPath checkpoint (``state_dict``, else ``$ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth}``, else seeded random
    weights when ``random_init_seed`` is given) as an extractor on the HIP kernels, behind the same device front end as the
    ViTs: Pillow-exact device resize (shorter side -> 224, bilinear) for tiles that are not 224 px."""
    sd, seeded = resolve_weights(name, state_dict, random_init_seed, lambda seed: random_canonical_state_dict(arch, seed),
                                 "timm, original CTransPath or transformers SwinModel")
    canonical = sd if seeded else canonical_state_dict(sd, arch=arch, source=source)
    folded = fold_batchnorm(canonical, arch=arch, dtype=dtype)
    net = HipSwin(arch, folded, device=torch.device(device), dtype=dtype)
    return HipViTFeatureExtractor(name=name, vit=net, mean=mean or IMAGENET_MEAN, std=std or IMAGENET_STD,
                                  max_batch=max_batch, resize=TRANSFORM_RESIZE, expect_size=None)


def register_chief_ctranspath(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """chief-ctranspath (models/patch/chief_ctranspath.py): the CHIEF_CTransPath checkpoint from ATLASPATCH_WEIGHTS_DIR (timm,
    original or transformers keys), or ATLASPATCH_RANDOM_INIT=<seed>."""
    dev = torch.device(device)
    for name in ARCHS:
        registry.register(name, lambda n=name: build_hip_swin_extractor(
            name=n, arch=n, device=dev, dtype=dtype, random_init_seed=_env_seed()))
