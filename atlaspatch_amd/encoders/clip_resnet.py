"""OpenAI CLIP ResNet image towers -- clip_rn50 / clip_rn101 / clip_rn50x4 / clip_rn50x16 / clip_rn50x64
(models/patch/clip.py of the reference: open_clip ``RN50`` .. ``RN50x64`` with the ``openai`` weights, ``encode_image``) --
on the native HIP kernels.

The network is CLIP's *modified* ResNet: a stem of three 3x3 convolutions and a 2x2 average pool, bottleneck blocks in which
every stride of 2 is a 2x2 average pool in front of a stride-1 convolution (main path and shortcut), and an attention-pool
head (mean token + positional embedding, the mean token as the one query, heads of 64).  The transform is open_clip's for
the ``openai`` tags: Pillow BICUBIC resize of the shorter side to the model's size, centre crop, CLIP mean / std.

Every convolution, pool, the head and the preprocess run in HIP kernels behind ``ap_clip_resnet_*``, with BatchNorm folded
into the convolutions on the host (f32).  Checkpoints come in open_clip / OpenAI keys (``conv1``, ``bn1``, ``layerX.Y.convK`` /
``bnK``, ``downsample.0/1``, ``attnpool.*``), bare or under ``visual.``; a whole CLIP state dict is accepted and its text tower
dropped.

These names are not in ``build_default_registry``: they are registered by ``register_clip_resnets``, which the shipped plugin
``atlaspatch_amd/plugins/openai_clip_resnets.py`` calls (``--feature-plugin``).
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import torch
import torch.nn.functional as F

from .. import _lib
from . import convbn
from .base import HipViTFeatureExtractor, NativeEncoder
from .checkpoints import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, _env_seed, check_canonical, resolve_weights

BN_EPS = convbn.BN_EPS
HEAD_DIM = 64

ARCHS = {
    "clip_rn50": {"depths": (3, 4, 6, 3), "width": 64, "image_size": 224, "output_dim": 1024},
    "clip_rn101": {"depths": (3, 4, 23, 3), "width": 64, "image_size": 224, "output_dim": 512},
    "clip_rn50x4": {"depths": (4, 6, 10, 6), "width": 80, "image_size": 288, "output_dim": 640},
    "clip_rn50x16": {"depths": (6, 8, 18, 8), "width": 96, "image_size": 384, "output_dim": 768},
    "clip_rn50x64": {"depths": (3, 15, 36, 10), "width": 128, "image_size": 448, "output_dim": 1024},
}
# device batch: four buffers of the largest activation (the stem's third convolution: (S / 2)^2 pixels of the width rounded up to
# 32 channels) stay below 2 GB in float16 -- 1.64 / 1.64 / 1.53 / 1.81 / 1.64 GB
MAX_BATCH = {"clip_rn50": 256, "clip_rn101": 256, "clip_rn50x4": 96, "clip_rn50x16": 64, "clip_rn50x64": 32}


def _spec(arch) -> dict:
    return dict(ARCHS[arch] if isinstance(arch, str) else arch)


def embed_width(arch) -> int:
    """C = 32 x width: the channels of the final map (heads = C / 64)."""
    return 32 * int(_spec(arch)["width"])


def grid_size(arch) -> int:
    return int(_spec(arch)["image_size"]) // 32


def conv_layers(arch) -> list:
    """[(name, cout, cin, k, stride)] of every convolution in forward order, open_clip names (``downsample`` for the shortcut's
    projection).  ``stride`` is the block's (the stem's first convolution's own): inside the blocks it is carried by a 2x2
    average pool, every convolution there has stride 1.  The order is the one ``ap_clip_resnet_create`` allocates."""
    spec = _spec(arch)
    w = int(spec["width"])
    stem = [("conv1", w // 2, 3, 3, 2), ("conv2", w // 2, w // 2, 3, 1), ("conv3", w, w // 2, 3, 1)]
    return stem + convbn.stage_layers(w, spec["depths"], bottleneck=True, stride_in_conv=False)


def canonical_keys(arch) -> dict:
    """{open_clip key: shape} of the unfolded visual tower (no ``num_batches_tracked``)."""
    spec = _spec(arch)
    keys = convbn.conv_bn_keys(conv_layers(arch))
    c, g = embed_width(arch), grid_size(arch)
    keys["attnpool.positional_embedding"] = (g * g + 1, c)
    for proj, rows in (("q_proj", c), ("k_proj", c), ("v_proj", c), ("c_proj", int(spec["output_dim"]))):
        keys[f"attnpool.{proj}.weight"] = (rows, c)
        keys[f"attnpool.{proj}.bias"] = (rows,)
    return keys


def canonical_state_dict(sd: dict, *, arch) -> dict:
    """The checkpoint as unfolded float32 tensors under open_clip's visual keys (``canonical_keys``).  Keys may be bare or carry
    ``visual.`` and / or ``module.`` in front; tensors may be stored in float16.  With ``visual.`` keys present the dict is a whole
    CLIP model: everything outside ``visual.`` (text tower, ``logit_scale``, ``input_resolution``, ``context_length``,
    ``vocab_size``) is dropped.  ``num_batches_tracked`` is dropped.  An unknown visual key, a missing key or a wrong shape --
    a positional embedding of another resolution included: it is not interpolated -- is a ``ValueError``."""
    want = canonical_keys(arch)
    stripped = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    whole_clip = any(k.startswith("visual.") for k in stripped)
    out, unknown = {}, []
    for key, value in stripped.items():
        if whole_clip:
            if not key.startswith("visual."):
                continue                                     # the text tower and the model's scalars
            name = key[len("visual."):]
        else:
            name = key
        if name.endswith("num_batches_tracked"):
            continue
        if name not in want:
            unknown.append(key)
            continue
        out[name] = torch.as_tensor(value).detach().to(torch.float32).cpu().contiguous()
    return check_canonical(out, want, unknown, family="CLIP ResNet", source="open_clip")


def fold_batchnorm(canonical: dict, *, arch, dtype: torch.dtype = torch.float32, eps: float = BN_EPS) -> dict:
    """Conv + BatchNorm (eval) -> one conv with bias, in float32 (W' = W g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)),
    and the head under the engine's names: ``attnpool.pos``, ``attnpool.q``, ``attnpool.kv`` (k_proj's rows, then v_proj's) and
    ``attnpool.c``.  What ``ap_clip_resnet_set_param`` takes.  A folded weight that is not finite in ``dtype`` is refused."""
    out = convbn.fold_layers(canonical, conv_layers(arch), dtype, eps)
    a = "attnpool."
    out["attnpool.pos"] = canonical[a + "positional_embedding"].contiguous()
    out["attnpool.q.weight"] = canonical[a + "q_proj.weight"][:, :, None, None].contiguous()
    out["attnpool.q.bias"] = canonical[a + "q_proj.bias"].contiguous()
    out["attnpool.kv.weight"] = torch.cat([canonical[a + "k_proj.weight"], canonical[a + "v_proj.weight"]])[:, :, None, None].contiguous()
    out["attnpool.kv.bias"] = torch.cat([canonical[a + "k_proj.bias"], canonical[a + "v_proj.bias"]]).contiguous()
    out["attnpool.c.weight"] = canonical[a + "c_proj.weight"][:, :, None, None].contiguous()
    out["attnpool.c.bias"] = canonical[a + "c_proj.bias"].contiguous()
    return out


def stored_channels(c: int) -> int:
    """Channels a map of ``c`` channels is stored with: the next multiple of 32 (the implicit GEMM's granularity in Cout)."""
    return (int(c) + 31) // 32 * 32


def padded_parameters(folded: dict, *, arch) -> dict:
    """The folded convolution parameters as the engine stores them (``ParamStore::add_padded``), in torch layout: output
    channels padded to ``stored_channels`` with zero weight rows and zero bias, input channels padded to the producing map's
    stored count (the image: 8) with zero weights.  A padded output channel is then ReLU(0 + 0) = 0, and stays 0 through the
    average pools; a padded input channel contributes nothing."""
    out = {}
    for name, cout, cin, k, _ in conv_layers(arch):
        cin_p = 8 if name == "conv1" else stored_channels(cin)
        w = torch.zeros(stored_channels(cout), cin_p, k, k, dtype=folded[f"{name}.weight"].dtype)
        w[:cout, :cin] = folded[f"{name}.weight"]
        b = torch.zeros(stored_channels(cout), dtype=folded[f"{name}.bias"].dtype)
        b[:cout] = folded[f"{name}.bias"]
        out[f"{name}.weight"], out[f"{name}.bias"] = w, b
    return out


def _forward_calibrate(sd: dict, arch, x: torch.Tensor) -> None:
    """Seeded random init: one CPU float32 forward of the convolutional part that sets every BatchNorm's running statistics to
    the batch statistics of its input (rounded to float16 precision so that they do not depend on the host's summation order)."""
    spec = _spec(arch)

    bn = functools.partial(convbn.calibrate_bn, sd)

    def conv(t, name, stride=1):
        w = sd[convbn.conv_key(name)]
        return F.conv2d(t, w, stride=stride, padding=w.shape[-1] // 2)

    x = F.relu(bn(conv(x, "conv1", 2), "bn1"))
    x = F.relu(bn(conv(x, "conv2"), "bn2"))
    x = F.relu(bn(conv(x, "conv3"), "bn3"))
    x = F.avg_pool2d(x, 2)
    for s, depth in enumerate(spec["depths"]):
        for b in range(depth):
            pre = f"layer{s + 1}.{b}."
            stride = 2 if (s > 0 and b == 0) else 1
            y = F.relu(bn(conv(x, pre + "conv1"), pre + "bn1"))
            y = F.relu(bn(conv(y, pre + "conv2"), pre + "bn2"))
            if stride == 2:
                y = F.avg_pool2d(y, 2)
            y = bn(conv(y, pre + "conv3"), pre + "bn3")
            sc = x
            if convbn.conv_key(pre + "downsample") in sd:
                sc = bn(conv(F.avg_pool2d(x, 2) if stride == 2 else x, pre + "downsample"), pre + "downsample.1")
            x = F.relu(y + sc)


def calibration_images(size: int, seed: int, count: int = 8) -> torch.Tensor:
    """Seeded images with the spectrum of a photograph rather than of white noise, normalised float32 [count, 3, size, size]:
    stationary random fields of three scales, every image statistically like every other.  The average pools pass low
    frequencies whole and halve white noise, so statistics taken on noise leave a smooth tile's activations growing stage by
    stage; images that each carry a colour or contrast of their own are too few samples for the deep layers, whose units see
    the whole image.  On images drawn like these (another seed) the seeded network's activations stay O(1) and its head's
    softmax soft: what a well-conditioned comparison needs."""
    g = torch.Generator().manual_seed(10007 + int(seed))
    up = lambda t: F.interpolate(t, size=(size, size), mode="bilinear", align_corners=False)
    return (0.8 * up(torch.randn(count, 3, max(size // 16, 2), max(size // 16, 2), generator=g))
            + 0.5 * up(torch.randn(count, 3, max(size // 4, 2), max(size // 4, 2), generator=g))
            + 0.3 * torch.randn(count, 3, size, size, generator=g))


def random_canonical_state_dict(arch, seed: int = 0) -> dict:
    """Seeded, well-conditioned random weights in canonical (open_clip, unfolded) form: He-normal convolutions, BatchNorm gains
    near 1 (the last BatchNorm of every block scaled by 1 / sqrt(blocks in its stage), so that the residual sums of a stage stay
    O(1)), small shifts, running statistics calibrated on seeded smooth random images (``calibration_images``), and the head as CLIP initialises it:
    projections and positional embedding normal with std C^-0.5."""
    spec = _spec(arch)
    g = torch.Generator().manual_seed(int(seed))
    sd = convbn.random_conv_bn(conv_layers(arch), spec["depths"], 3, g)
    c, grid = embed_width(arch), grid_size(arch)
    std = float(c) ** -0.5
    sd["attnpool.positional_embedding"] = torch.randn(grid * grid + 1, c, generator=g) * std
    for proj, rows in (("q_proj", c), ("k_proj", c), ("v_proj", c), ("c_proj", int(spec["output_dim"]))):
        sd[f"attnpool.{proj}.weight"] = torch.randn(rows, c, generator=g) * std
        sd[f"attnpool.{proj}.bias"] = 0.02 * torch.randn(rows, generator=g)
    x = calibration_images(min(int(spec["image_size"]), 224), int(seed), count=6)      # the zero padding's weight in the last maps
    with torch.no_grad():
        _forward_calibrate(sd, arch, x)
    return {k: sd[k].contiguous() for k in canonical_keys(arch)}


# ----------------------------------------------------------------------------- device object
class HipClipResNet(NativeEncoder):
    """Device-resident CLIP ResNet behind ``ap_clip_resnet_*``."""

    ABI = "clip_resnet"
    PROF_KINDS = _lib.CLIP_RESNET_PROF_KINDS

    def __init__(self, arch, folded: dict, *, device: torch.device, dtype: torch.dtype) -> None:
        self._bind(device, dtype)
        spec = _spec(arch)
        self._open(_lib.ClipResnetConfig((C.c_int * 4)(*spec["depths"]), int(spec["width"]), int(spec["image_size"]),
                                         int(spec["output_dim"]), _lib.torch_dtype_code(dtype)), folded)
        self.embed_dim = int(self.lib.ap_clip_resnet_embed_dim(self._handle))


# ----------------------------------------------------------------------------- builders
def build_hip_clip_resnet_extractor(*, name: str, arch, device, dtype, state_dict: Optional[dict] = None, mean=None, std=None,
                                    max_batch: Optional[int] = None,
                                    random_init_seed: Optional[int] = None) -> HipViTFeatureExtractor:
    """A CLIP ResNet checkpoint (``state_dict``, else ``$ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth}``, else seeded random
    weights when ``random_init_seed`` is given) as an extractor on the HIP kernels, behind the same device front end as the
    ViTs: Pillow-exact device resize (shorter side -> the model's size, bicubic) for tiles of another size, then centre crop."""
    sd, seeded = resolve_weights(name, state_dict, random_init_seed, lambda seed: random_canonical_state_dict(arch, seed),
                                 "open_clip / OpenAI CLIP")
    canonical = sd if seeded else canonical_state_dict(sd, arch=arch)
    folded = fold_batchnorm(canonical, arch=arch, dtype=dtype)
    net = HipClipResNet(arch, folded, device=torch.device(device), dtype=dtype)
    if max_batch is None:
        max_batch = MAX_BATCH.get(arch, 32) if isinstance(arch, str) else 32
    return HipViTFeatureExtractor(name=name, vit=net, mean=mean or OPENAI_CLIP_MEAN, std=std or OPENAI_CLIP_STD,
                                  max_batch=max_batch, resize=(int(_spec(arch)["image_size"]), "bicubic"), expect_size=None)


def register_clip_resnets(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """clip_rn50 / clip_rn101 / clip_rn50x4 / clip_rn50x16 / clip_rn50x64 (models/patch/clip.py): OpenAI weights from
    ATLASPATCH_WEIGHTS_DIR (open_clip / OpenAI keys, the visual tower or the whole model), or ATLASPATCH_RANDOM_INIT=<seed>."""
    dev = torch.device(device)
    for name in ARCHS:
        registry.register(name, lambda n=name: build_hip_clip_resnet_extractor(
            name=n, arch=n, device=dev, dtype=dtype, random_init_seed=_env_seed()))
