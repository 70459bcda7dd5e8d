"""ConvNeXt-Tiny / Small / Base / Large encoders on the native HIP kernels (models/patch/convnext.py of the reference).

The reference builds torchvision ``convnext_xxx(weights=IMAGENET1K_V1)`` and replaces the WHOLE ``classifier`` (LayerNorm,
Flatten, Linear) with ``Identity``: the feature is the flattened global average pool of the last stage, without the head's
LayerNorm (768 / 768 / 1024 / 1536-d).  Preprocessing is ``weights.transforms()`` = ``ImageClassification(crop_size=224,
resize_size=R)``: Pillow BILINEAR resize of the shorter side to R (236 / 230 / 232 / 232), centre crop 224, ImageNet
normalisation -- so unlike the ResNets a 256-px tile is always resized (on the device, Pillow-exact).

Here the depthwise 7x7 convolution + LayerNorm of every block runs in ``convnext.hip``, and the stem, the downsampling
convolutions and the pointwise fc1 (GELU) / fc2 (+ residual) in ``conv.hip``'s implicit GEMM, behind ``ap_convnext_*``.
``layer_scale`` is folded into fc2 on the host (f32).  Checkpoints come in torchvision keys (``features.*``; ``classifier.*``
dropped) or transformers ``ConvNextModel`` keys (``embeddings.*``, ``encoder.stages.S.*``; an optional ``convnext.`` prefix
stripped, the top-level ``layernorm.*`` and ``classifier.*`` dropped); both are detected.

These names are not in ``build_default_registry``: they are registered by ``register_convnexts``, which the shipped plugin
``atlaspatch_amd/plugins/torchvision_convnexts.py`` calls (``--feature-plugin``).
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Optional

import numpy as np
import torch

from .. import _lib
from .base import HipViTFeatureExtractor, NativeEncoder
from .checkpoints import IMAGENET_MEAN, IMAGENET_STD, _env_seed, check_canonical, resolve_weights

LN_EPS = 1e-6

# resize: torchvision's ConvNeXt_*_Weights.IMAGENET1K_V1 transforms (ImageClassification(crop_size=224, resize_size=R))
ARCHS = {
    "convnext_tiny": {"depths": (3, 3, 9, 3), "widths": (96, 192, 384, 768), "embed_dim": 768, "resize": 236},
    "convnext_small": {"depths": (3, 3, 27, 3), "widths": (96, 192, 384, 768), "embed_dim": 768, "resize": 230},
    "convnext_base": {"depths": (3, 3, 27, 3), "widths": (128, 256, 512, 1024), "embed_dim": 1024, "resize": 232},
    "convnext_large": {"depths": (3, 3, 27, 3), "widths": (192, 384, 768, 1536), "embed_dim": 1536, "resize": 232},
}
DEFAULTS = {"image_size": 224}
MAX_BATCH = 256         # device batch: convnext_large's workspace at 256 tiles is 3.7 GB in float16


def _spec(arch) -> dict:
    spec = dict(DEFAULTS)
    spec.update(ARCHS[arch] if isinstance(arch, str) else arch)
    return spec


def canonical_keys(arch) -> dict:
    """{torchvision key: shape} of the checkpoint without the classifier, in forward order."""
    spec = _spec(arch)
    w = spec["widths"]
    keys = {"features.0.0.weight": (w[0], 3, 4, 4), "features.0.0.bias": (w[0],),
            "features.0.1.weight": (w[0],), "features.0.1.bias": (w[0],)}
    for s, depth in enumerate(spec["depths"]):
        c = w[s]
        if s > 0:
            d = f"features.{2 * s}."
            keys.update({d + "0.weight": (w[s - 1],), d + "0.bias": (w[s - 1],),
                         d + "1.weight": (c, w[s - 1], 2, 2), d + "1.bias": (c,)})
        for j in range(depth):
            p = f"features.{2 * s + 1}.{j}."
            keys.update({p + "layer_scale": (c, 1, 1),
                         p + "block.0.weight": (c, 1, 7, 7), p + "block.0.bias": (c,),
                         p + "block.2.weight": (c,), p + "block.2.bias": (c,),
                         p + "block.3.weight": (4 * c, c), p + "block.3.bias": (4 * c,),
                         p + "block.5.weight": (c, 4 * c), p + "block.5.bias": (c,)})
    return keys


_HF_LAYER = {"dwconv": "block.0", "layernorm": "block.2", "pwconv1": "block.3", "pwconv2": "block.5"}
_HF_STAGE = re.compile(r"^encoder\.stages\.(\d+)\.(?:downsampling_layer\.(\d+)\.(weight|bias)|"
                       r"layers\.(\d+)\.(?:(dwconv|layernorm|pwconv1|pwconv2)\.(weight|bias)|(layer_scale_parameter)))$")


def _hf_to_torchvision(key: str) -> Optional[str]:
    for hf, tv in (("embeddings.patch_embeddings.", "features.0.0."), ("embeddings.layernorm.", "features.0.1.")):
        if key.startswith(hf) and key[len(hf):] in ("weight", "bias"):
            return tv + key[len(hf):]
    m = _HF_STAGE.match(key)
    if m is None:
        return None
    stage, ds_idx, ds_param, layer, part, param, ls = m.groups()
    s = int(stage)
    if ds_idx is not None:
        return f"features.{2 * s}.{ds_idx}.{ds_param}" if s > 0 else None
    pre = f"features.{2 * s + 1}.{int(layer)}."
    if ls is not None:
        return pre + "layer_scale"
    return pre + _HF_LAYER[part] + "." + param


def detect_source(sd: dict) -> str:
    keys = list(sd)
    if any(k.startswith(("embeddings.", "encoder.stages.", "convnext.embeddings.", "convnext.encoder.")) for k in keys):
        return "hf"
    if any(k.startswith("features.") for k in keys):
        return "torchvision"
    raise ValueError("ConvNeXt checkpoint: neither torchvision keys (features.*) nor transformers ConvNextModel keys "
                     f"(embeddings.*, encoder.stages.*) found; first keys: {keys[:5]}")


def canonical_state_dict(sd: dict, *, arch, source: str = "auto") -> dict:
    """The checkpoint as float32 tensors under torchvision keys (``canonical_keys``, layer_scale unfolded, shape [C, 1, 1]).
    ``source``: "torchvision", "hf" (transformers ``ConvNextModel``; a ``ConvNextForImageClassification`` dict's
    ``convnext.`` prefix is stripped) or "auto".  The classifier (and transformers' final ``layernorm``) is dropped; any other
    unknown key, a missing key or a wrong shape is a ``ValueError``."""
    if source == "auto":
        source = detect_source(sd)
    if source not in ("torchvision", "hf"):
        raise ValueError(f"unknown ConvNeXt checkpoint layout {source!r}")
    want = canonical_keys(arch)
    out, unknown = {}, []
    for key, value in sd.items():
        if source == "hf":
            k = key[len("convnext."):] if key.startswith("convnext.") else key
            if k.startswith(("classifier.", "layernorm.")):
                continue
            name = _hf_to_torchvision(k)
        else:
            name = key[len("module."):] if key.startswith("module.") else key
            if name.startswith("classifier."):
                continue
        if name is None or name not in want:
            unknown.append(key)
            continue
        t = torch.as_tensor(value).detach().to(torch.float32).cpu()
        if name.endswith("layer_scale") and t.dim() == 1:
            t = t.view(-1, 1, 1)                        # transformers keeps it as [C]
        out[name] = t.contiguous()
    return check_canonical(out, want, unknown, family="ConvNeXt", source=source)


def fold_layer_scale(canonical: dict, *, arch, dtype: torch.dtype = torch.float32) -> dict:
    """The parameters ``ap_convnext_set_param`` takes: every key but ``layer_scale``, with gamma folded into fc2 in float32
    (W2'[o] = gamma_o W2[o], b2'[o] = gamma_o b2[o]: exact up to one f32 rounding per element).  A folded weight that is not
    finite in ``dtype`` is refused."""
    out = {}
    for k in canonical_keys(arch):
        if k.endswith("layer_scale"):
            continue
        out[k] = canonical[k]
    for k in canonical_keys(arch):
        if not k.endswith("layer_scale"):
            continue
        pre = k[:-len("layer_scale")]
        g = canonical[k].reshape(-1)
        w = canonical[pre + "block.5.weight"] * g.view(-1, 1)
        b = canonical[pre + "block.5.bias"] * g
        if not bool(torch.isfinite(w.to(dtype)).all()) or not bool(torch.isfinite(b).all()):
            raise ValueError(f"{pre}block.5: the layer_scale-folded weights are not finite in {dtype}")
        out[pre + "block.5.weight"] = w.contiguous()
        out[pre + "block.5.bias"] = b.contiguous()
    return out


def random_canonical_state_dict(arch, seed: int = 0) -> dict:
    """Seeded, well-conditioned random weights in canonical (torchvision, unfolded) form.  Every convolution / linear layer
    is scaled to unit output variance for unit input, LayerNorm gains near 1 with small shifts, and layer_scale in
    [0.3, 0.8] (NOT the 1e-6 of a fresh torchvision model): every block's branch adds a visible share of the residual
    stream, so a wrong block changes the features, and activations stay O(1), far inside float16's range."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for k, shape in canonical_keys(arch).items():
        if k.endswith("layer_scale"):
            sd[k] = 0.3 + 0.5 * torch.rand(shape, generator=g)
        elif len(shape) > 1:
            fan_in = int(np.prod(shape[1:]))
            sd[k] = torch.randn(shape, generator=g) / float(np.sqrt(fan_in))
        elif k.endswith(".bias"):
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        else:                                           # LayerNorm gains
            sd[k] = 0.8 + 0.4 * torch.rand(shape, generator=g)
    return {k: sd[k].contiguous() for k in canonical_keys(arch)}


# ----------------------------------------------------------------------------- device object
class HipConvNeXt(NativeEncoder):
    """Device-resident ConvNeXt behind ``ap_convnext_*``."""

    ABI = "convnext"
    PROF_KINDS = _lib.CONVNEXT_PROF_KINDS

    def __init__(self, arch, folded: dict, *, device: torch.device, dtype: torch.dtype) -> None:
        self._bind(device, dtype)
        spec = _spec(arch)
        self._open(_lib.ConvnextConfig((C.c_int * 4)(*spec["depths"]), (C.c_int * 4)(*spec["widths"]),
                                       _lib.torch_dtype_code(dtype), int(spec["image_size"])), folded)
        self.embed_dim = int(self.lib.ap_convnext_embed_dim(self._handle))


# ----------------------------------------------------------------------------- builders
def build_hip_convnext_extractor(*, name: str, arch, device, dtype, state_dict: Optional[dict] = None, source: str = "auto",
                                 mean=None, std=None, max_batch: int = MAX_BATCH,
                                 random_init_seed: Optional[int] = None) -> HipViTFeatureExtractor:
    """A ConvNeXt checkpoint (``state_dict``, else ``$ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth}``, else seeded random
    weights when ``random_init_seed`` is given) as an extractor on the HIP kernels, behind the same device front end as the
    ViTs: Pillow-exact device resize (shorter side -> the variant's resize size, bilinear), then centre crop 224."""
    spec = _spec(arch)
    sd, seeded = resolve_weights(name, state_dict, random_init_seed, lambda seed: random_canonical_state_dict(arch, seed),
                                 "torchvision or transformers ConvNextModel")
    canonical = sd if seeded else canonical_state_dict(sd, arch=arch, source=source)
    folded = fold_layer_scale(canonical, arch=arch, dtype=dtype)
    net = HipConvNeXt(arch, folded, device=torch.device(device), dtype=dtype)
    return HipViTFeatureExtractor(name=name, vit=net, mean=mean or IMAGENET_MEAN, std=std or IMAGENET_STD,
                                  max_batch=max_batch, resize=(int(spec["resize"]), "bilinear"), expect_size=None)


def register_convnexts(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """convnext_tiny / small / base / large (models/patch/convnext.py): torchvision ImageNet weights from
    ATLASPATCH_WEIGHTS_DIR (torchvision or transformers keys), or ATLASPATCH_RANDOM_INIT=<seed>."""
    dev = torch.device(device)
    for name in ARCHS:
        registry.register(name, lambda n=name: build_hip_convnext_extractor(
            name=n, arch=n, device=dev, dtype=dtype, random_init_seed=_env_seed()))
