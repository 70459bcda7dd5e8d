"""Plugin API (reference: models/patch/custom.py:19-146), kept verbatim at the boundary:

* a plugin file defines ``register_feature_extractors(registry, device, dtype, num_workers)``;
  it is loaded by path and the hook is invoked WITH KEYWORD ARGUMENTS (custom.py:146);
* inside, the plugin calls ``register_custom_encoder(registry=..., name=..., embedding_dim=...,
  loader=..., device=..., dtype=..., num_workers=0, non_blocking=False)`` whose ``loader(device,
  dtype)`` returns ``CustomEncoderComponents(model, preprocess, forward_fn=None)``.

MI355X addition: a loader may also return ``device_transform=DeviceTransform(...)``, its ``preprocess`` restated for the
device (encoders/device_transform.py).  The module then runs from the tile ring like a native encoder
(``DeviceTorchFeatureExtractor``); without it nothing changes.

MI355X addition: ``register_hip_vit_encoder`` / ``register_hip_resnet_encoder`` let a plugin hand over a ViT / ResNet
state dict and have it run in the native HIP kernels instead of as a torch module.
"""
from __future__ import annotations

import dataclasses as _dc
import importlib.util
import logging
from pathlib import Path
from types import ModuleType
from typing import Callable, Optional, Protocol

import torch
from PIL import Image

from .base import DeviceTorchFeatureExtractor, PatchFeatureExtractor
from .device_transform import DeviceTransform
from .registry import PatchFeatureExtractorRegistry

logger = logging.getLogger("atlaspatch_amd.encoders.custom")


class CustomEncoderLoader(Protocol):
    def __call__(self, device: torch.device, dtype: torch.dtype) -> "CustomEncoderComponents": ...


@_dc.dataclass
class CustomEncoderComponents:
    model: torch.nn.Module
    preprocess: Callable[[Image.Image], torch.Tensor]
    forward_fn: Optional[Callable[[torch.Tensor], torch.Tensor]] = None
    device_transform: Optional[DeviceTransform] = None        # ``preprocess`` restated for the device; None = the host route


def register_custom_encoder(*, registry: PatchFeatureExtractorRegistry, name: str, embedding_dim: int,
                            loader: CustomEncoderLoader, device: torch.device, dtype: torch.dtype,
                            num_workers: int = 0, non_blocking: bool = False, device_batch: int = 256) -> None:
    """``device_batch``: tiles per model call when the loader returns a ``device_transform`` (the ring's own batch stays
    capped at 2048 as for every encoder).  A memory knob for a model of unknown size, not a tuned value: lower it when the
    model's activations do not fit, raise it for a small model."""
    def build() -> PatchFeatureExtractor:
        parts = loader(device, dtype)
        if not isinstance(parts, CustomEncoderComponents):
            raise TypeError(f"Custom encoder loader for '{name}' must return CustomEncoderComponents, "
                            f"got {type(parts)}.")
        kw = dict(name=name, model=parts.model, embedding_dim=embedding_dim, preprocess=parts.preprocess, device=device,
                  dtype=dtype, num_workers=num_workers, non_blocking=non_blocking, forward_fn=parts.forward_fn)
        if parts.device_transform is not None and torch.device(device).type == "cuda":
            if not isinstance(parts.device_transform, DeviceTransform):
                raise TypeError(f"Custom encoder loader for '{name}': device_transform must be a DeviceTransform, "
                                f"got {type(parts.device_transform)}.")
            return DeviceTorchFeatureExtractor(device_transform=parts.device_transform, max_batch=device_batch, **kw)
        return PatchFeatureExtractor(**kw)

    registry.register(name, build)


def register_hip_vit_encoder(*, registry: PatchFeatureExtractorRegistry, name: str,
                             state_dict_loader: Callable[[], dict], arch: str,
                             device: torch.device, dtype: torch.dtype, mean=None, std=None,
                             source: str = "auto", **arch_overrides) -> None:
    """Register a ViT checkpoint to run in the native HIP kernels (lazy, like every builder)."""
    from .vit import build_hip_vit_extractor

    def build():
        return build_hip_vit_extractor(name=name, arch=arch, state_dict=state_dict_loader(),
                                       device=device, dtype=dtype, mean=mean, std=std, source=source,
                                       **arch_overrides)

    registry.register(name, build)


def register_hip_resnet_encoder(*, registry: PatchFeatureExtractorRegistry, name: str,
                                state_dict_loader: Callable[[], dict], arch, device: torch.device,
                                dtype: torch.dtype, mean=None, std=None, source: str = "auto") -> None:
    """Register a ResNet checkpoint (torchvision or transformers ResNetModel keys; ``arch`` one of resnet18 .. resnet152 or
    a dict ``{"block": "basic" | "bottleneck", "depths": (d1, d2, d3, d4)}``) to run in the native HIP kernels (lazy)."""
    from .resnet import build_hip_resnet_extractor

    def build():
        return build_hip_resnet_extractor(name=name, arch=arch, state_dict=state_dict_loader(), device=device,
                                          dtype=dtype, mean=mean, std=std, source=source)

    registry.register(name, build)


class CustomRegistryHook(Protocol):
    def __call__(self, registry: PatchFeatureExtractorRegistry, device: torch.device,
                 dtype: torch.dtype, num_workers: int) -> None: ...


def _load_module(path: Path) -> ModuleType:
    spec = importlib.util.spec_from_file_location(path.stem, path)
    if spec is None or spec.loader is None:
        raise RuntimeError(f"Failed to load module spec from {path}")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def register_feature_extractors_from_module(module_path, registry: PatchFeatureExtractorRegistry, *,
                                            device: torch.device, dtype: torch.dtype,
                                            num_workers: int = 0) -> None:
    path = Path(module_path).expanduser().resolve()
    hook = getattr(_load_module(path), "register_feature_extractors", None)
    if not callable(hook):
        raise AttributeError(f"Custom encoder module {path} must define a callable "
                             "'register_feature_extractors(registry, device, dtype, num_workers)'.")
    logger.info("Registering custom feature extractors from %s", path)
    hook(registry=registry, device=device, dtype=dtype, num_workers=num_workers)


__all__ = ["CustomEncoderComponents", "DeviceTransform", "CustomEncoderLoader", "CustomRegistryHook",
           "register_custom_encoder", "register_hip_vit_encoder", "register_hip_resnet_encoder",
           "register_feature_extractors_from_module"]
