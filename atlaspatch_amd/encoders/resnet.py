"""ResNet-18 / 34 / 50 / 101 / 152 encoders on the native HIP convolution kernels (models/patch/resnet.py of the reference).

The reference builds torchvision ``resnetXX(weights=IMAGENET1K_V1)`` with ``fc = Identity``: the feature is the flattened
global average pool (512-d for 18 / 34, 2048-d for 50 / 101 / 152), preprocessing ``weights.transforms()`` =
``ImageClassification(crop_size=224)`` -- Pillow BILINEAR resize of the shorter side to 256, centre crop 224, ImageNet
normalisation.  On the default 256-px tiles that is a pure centre crop (the transform of ``vit_b_16``).

Here every convolution, both pools and the preprocess run in the kernels of ``conv.hip`` behind ``ap_resnet_*``, with
BatchNorm folded into the convolutions on the host (f32).  Checkpoints come in torchvision keys (``conv1``, ``bn1``,
``layerX.Y.convK`` / ``bnK``, ``downsample.0/1``; ``fc.*`` dropped) or transformers ``ResNetModel`` keys
(``embedder.embedder.*``, ``encoder.stages.S.layers.L.{layer.K,shortcut}.*``); both are detected.

These names are not in ``build_default_registry``: they are registered by ``register_resnets``, which the shipped plugin
``atlaspatch_amd/plugins/torchvision_resnets.py`` calls (``--feature-plugin``).
"""
from __future__ import annotations

import ctypes as C
import functools
import re
from typing import Optional

import torch
import torch.nn.functional as F

from .. import _lib
from . import convbn
from .base import HipViTFeatureExtractor, NativeEncoder
from .checkpoints import IMAGENET_MEAN, IMAGENET_STD, _env_seed, check_canonical, resolve_weights

BN_EPS = convbn.BN_EPS
TRANSFORM_RESIZE = (256, "bilinear")      # ImageClassification(crop_size=224): resize 256 (Pillow BILINEAR), crop 224

ARCHS = {
    "resnet18": {"block": "basic", "depths": (2, 2, 2, 2), "embed_dim": 512},
    "resnet34": {"block": "basic", "depths": (3, 4, 6, 3), "embed_dim": 512},
    "resnet50": {"block": "bottleneck", "depths": (3, 4, 6, 3), "embed_dim": 2048},
    "resnet101": {"block": "bottleneck", "depths": (3, 4, 23, 3), "embed_dim": 2048},
    "resnet152": {"block": "bottleneck", "depths": (3, 8, 36, 3), "embed_dim": 2048},
}
DEFAULTS = {"stem_width": 64, "image_size": 224}
MAX_BATCH = 256         # device batch: resnet50's four activation buffers at 256 tiles are 1.6 GB in float16


def _spec(arch) -> dict:
    spec = dict(DEFAULTS)
    spec.update(ARCHS[arch] if isinstance(arch, str) else arch)
    return spec


def conv_layers(arch) -> list:
    """[(name, cout, cin, k, stride, has_bn)] of every convolution in forward order, torchvision names (``downsample`` for
    the projection shortcut).  The order is the one ``ap_resnet_create`` allocates."""
    spec = _spec(arch)
    w = int(spec["stem_width"])
    return [("conv1", w, 3, 7, 2)] + convbn.stage_layers(w, spec["depths"], bottleneck=spec["block"] == "bottleneck",
                                                        stride_in_conv=True)


def canonical_keys(arch) -> dict:
    """{torchvision key: shape} of the unfolded checkpoint (no ``fc``, no ``num_batches_tracked``)."""
    return convbn.conv_bn_keys(conv_layers(arch))


_HF_CONV = re.compile(r"^encoder\.stages\.(\d+)\.layers\.(\d+)\.(layer\.(\d+)|shortcut)\.(convolution|normalization)\.(.+)$")


def _hf_to_torchvision(key: str) -> Optional[str]:
    if key.startswith("embedder.embedder."):
        rest = key[len("embedder.embedder."):]
        if rest.startswith("convolution."):
            return "conv1." + rest[len("convolution."):]
        if rest.startswith("normalization."):
            return "bn1." + rest[len("normalization."):]
        return None
    m = _HF_CONV.match(key)
    if m is None:
        return None
    stage, layer, part, k, kind, param = m.groups()
    pre = f"layer{int(stage) + 1}.{int(layer)}."
    if part == "shortcut":
        return pre + ("downsample.0." if kind == "convolution" else "downsample.1.") + param
    return pre + (f"conv{int(k) + 1}." if kind == "convolution" else f"bn{int(k) + 1}.") + param


def detect_source(sd: dict) -> str:
    keys = list(sd)
    if any(k.startswith(("embedder.", "encoder.stages.", "resnet.embedder.")) for k in keys):
        return "hf"
    if any(k.startswith(("conv1.", "layer1.")) for k in keys):
        return "torchvision"
    raise ValueError("ResNet checkpoint: neither torchvision keys (conv1.*, layerX.Y.*) nor transformers ResNetModel keys "
                     f"(embedder.embedder.*, encoder.stages.*) found; first keys: {keys[:5]}")


def canonical_state_dict(sd: dict, *, arch, source: str = "auto") -> dict:
    """The checkpoint as unfolded float32 tensors under torchvision keys (``canonical_keys``).  ``source``: "torchvision",
    "hf" (transformers ``ResNetModel``; a ``ResNetForImageClassification`` dict's ``resnet.`` prefix is stripped) or "auto".
    The classifier (``fc.*`` / ``classifier.*``) and ``num_batches_tracked`` are dropped; any other unknown key, a missing
    key or a wrong shape is a ``ValueError``."""
    if source == "auto":
        source = detect_source(sd)
    if source not in ("torchvision", "hf"):
        raise ValueError(f"unknown ResNet checkpoint layout {source!r}")
    want = canonical_keys(arch)
    out, unknown = {}, []
    for key, value in sd.items():
        if key.endswith("num_batches_tracked"):
            continue
        if source == "hf":
            k = key[len("resnet."):] if key.startswith("resnet.") else key
            if k.startswith("classifier."):
                continue
            name = _hf_to_torchvision(k)
        else:
            name = key[len("module."):] if key.startswith("module.") else key
            if name.startswith("fc."):
                continue
        if name is None or name not in want:
            unknown.append(key)
            continue
        out[name] = torch.as_tensor(value).detach().to(torch.float32).cpu().contiguous()
    return check_canonical(out, want, unknown, family="ResNet", source=source)


def fold_batchnorm(canonical: dict, *, arch, dtype: torch.dtype = torch.float32, eps: float = BN_EPS) -> dict:
    """Conv + BatchNorm (eval) -> one conv with bias, in float32: W' = W g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps).
    Keys ``<conv>.weight`` / ``<conv>.bias`` (``downsample`` for the projection), what ``ap_resnet_set_param`` takes.  A folded
    weight that is not finite in ``dtype`` (or a bias that is not finite) is refused."""
    return convbn.fold_layers(canonical, conv_layers(arch), dtype, eps)


def _forward_calibrate(sd: dict, arch, x: torch.Tensor) -> None:
    """Seeded random init: one CPU float32 forward that sets every BatchNorm's running statistics to the batch statistics of
    its input (rounded to float16 precision so that they do not depend on the host's summation order)."""
    spec = _spec(arch)

    bn = functools.partial(convbn.calibrate_bn, sd)

    layers = {name: (k, stride) for name, _, _, k, stride in conv_layers(arch)}

    def conv(t, name):
        k, stride = layers[name]
        return F.conv2d(t, sd[convbn.conv_key(name)], stride=stride, padding=k // 2)

    x = F.relu(bn(conv(x, "conv1"), "bn1"))
    x = F.max_pool2d(x, 3, 2, 1)
    n_conv = 3 if spec["block"] == "bottleneck" else 2
    for s, depth in enumerate(spec["depths"]):
        for b in range(depth):
            pre = f"layer{s + 1}.{b}."
            y = x
            for i in range(1, n_conv + 1):
                y = bn(conv(y, f"{pre}conv{i}"), f"{pre}bn{i}")
                if i < n_conv:
                    y = F.relu(y)
            sc = bn(conv(x, pre + "downsample"), pre + "downsample.1") if pre + "downsample" in layers else x
            x = F.relu(y + sc)


def random_canonical_state_dict(arch, seed: int = 0) -> dict:
    """Seeded, well-conditioned random weights in canonical (torchvision, unfolded) form: He-normal convolutions, BatchNorm
    gains near 1 (the last BatchNorm of every block scaled by 1 / sqrt(blocks in its stage), so that the residual sums of a
    stage stay O(1)), small shifts, and running statistics calibrated on a seeded random image batch -- activations stay
    O(1) through all stages, in float16's range with room to spare."""
    spec = _spec(arch)
    g = torch.Generator().manual_seed(int(seed))
    sd = convbn.random_conv_bn(conv_layers(arch), spec["depths"], 3 if spec["block"] == "bottleneck" else 2, g)
    x = torch.randn(2, 3, 128, 128, generator=g)
    with torch.no_grad():
        _forward_calibrate(sd, arch, x)
    return {k: sd[k].contiguous() for k in canonical_keys(arch)}


# ----------------------------------------------------------------------------- device object
class HipResNet(NativeEncoder):
    """Device-resident ResNet behind ``ap_resnet_*``."""

    ABI = "resnet"
    PROF_KINDS = _lib.RESNET_PROF_KINDS

    def __init__(self, arch, folded: dict, *, device: torch.device, dtype: torch.dtype) -> None:
        self._bind(device, dtype)
        spec = _spec(arch)
        self._open(_lib.ResnetConfig(1 if spec["block"] == "bottleneck" else 0, (C.c_int * 4)(*spec["depths"]),
                                     int(spec["stem_width"]), _lib.torch_dtype_code(dtype), int(spec["image_size"])), folded)
        self.embed_dim = int(self.lib.ap_resnet_embed_dim(self._handle))


# ----------------------------------------------------------------------------- builders
def build_hip_resnet_extractor(*, name: str, arch, device, dtype, state_dict: Optional[dict] = None, source: str = "auto",
                               mean=None, std=None, max_batch: int = MAX_BATCH,
                               random_init_seed: Optional[int] = None) -> HipViTFeatureExtractor:
    """A ResNet checkpoint (``state_dict``, else ``$ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth}``, else seeded random
    weights when ``random_init_seed`` is given) as an extractor on the HIP kernels, behind the same device front end as the
    ViTs: Pillow-exact device resize (shorter side -> 256, bilinear) for tiles that are not 256 px, then centre crop 224."""
    sd, seeded = resolve_weights(name, state_dict, random_init_seed, lambda seed: random_canonical_state_dict(arch, seed),
                                 "torchvision or transformers ResNetModel")
    canonical = sd if seeded else canonical_state_dict(sd, arch=arch, source=source)
    folded = fold_batchnorm(canonical, arch=arch, dtype=dtype)
    net = HipResNet(arch, folded, device=torch.device(device), dtype=dtype)
    return HipViTFeatureExtractor(name=name, vit=net, mean=mean or IMAGENET_MEAN, std=std or IMAGENET_STD,
                                  max_batch=max_batch, resize=TRANSFORM_RESIZE, expect_size=None)


def register_resnets(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """resnet18 / 34 / 50 / 101 / 152 (models/patch/resnet.py): torchvision ImageNet weights from ATLASPATCH_WEIGHTS_DIR
    (torchvision or transformers keys), or ATLASPATCH_RANDOM_INIT=<seed>."""
    dev = torch.device(device)
    for name in ARCHS:
        registry.register(name, lambda n=name: build_hip_resnet_extractor(
            name=n, arch=n, device=dev, dtype=dtype, random_init_seed=_env_seed()))
