"""Where an encoder's weights come from, shared by every family: the weights directory, checkpoint files, the seeded
random fall-back, the check of a canonical state dict against its key table, and the two normalisation constants."""
from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import Optional

import torch

logger = logging.getLogger(__name__)

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def weights_path(name: str) -> Optional[Path]:
    """``$ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth}`` if present."""
    root = os.environ.get("ATLASPATCH_WEIGHTS_DIR")
    if not root:
        return None
    for ext in (".safetensors", ".pt", ".pth"):
        candidate = Path(root) / f"{name}{ext}"
        if candidate.exists():
            return candidate
    return None


def load_checkpoint(path: Path) -> dict:
    if path.suffix == ".safetensors":
        from safetensors.torch import load_file
        return load_file(str(path))
    obj = torch.load(str(path), map_location="cpu", weights_only=True)
    for key in ("model", "state_dict"):
        if isinstance(obj, dict) and key in obj and isinstance(obj[key], dict):
            obj = obj[key]
    return obj


def resolve_weights(name: str, state_dict: Optional[dict], random_init_seed: Optional[int], random_init,
                    key_families: str) -> tuple[dict, bool]:
    """(checkpoint, seeded) for the model ``name``: ``state_dict`` if given, else ``$ATLASPATCH_WEIGHTS_DIR/<name>.*``, else
    ``random_init(random_init_seed)`` -- seeded random weights in canonical form (``seeded`` True) -- when a seed is given.
    ``key_families``: the checkpoint layouts the model takes, named in the error when there is none of the three."""
    if state_dict is not None:
        return state_dict, False
    path = weights_path(name)
    if path is not None:
        return load_checkpoint(path), False
    if random_init_seed is not None:
        logger.warning("%s: using seeded RANDOM weights (seed %d); features are not meaningful", name, random_init_seed)
        return random_init(random_init_seed), True
    raise FileNotFoundError(
        f"No weights for '{name}': set ATLASPATCH_WEIGHTS_DIR to a directory holding {name}.safetensors/.pt "
        f"({key_families} key names), or set ATLASPATCH_RANDOM_INIT=<seed> for seeded random weights (benchmarks/tests).")


def check_canonical(out: dict, want: dict, unknown: list, *, family: str, source: str) -> dict:
    """``out`` (canonical key -> tensor) against ``want`` (canonical key -> shape): a ``ValueError`` for checkpoint keys that
    mapped to no canonical key (``unknown``), then for missing keys, then for wrong shapes; else ``out``."""
    if unknown:
        raise ValueError(f"{family} checkpoint ({source} layout): {len(unknown)} unknown key(s) for this architecture, e.g. "
                         f"{unknown[:5]}")
    missing = [k for k in want if k not in out]
    if missing:
        raise ValueError(f"{family} checkpoint ({source} layout): {len(missing)} missing key(s), e.g. {missing[:5]}")
    for k, shape in want.items():
        if tuple(out[k].shape) != shape:
            raise ValueError(f"{family} checkpoint: {k} has shape {tuple(out[k].shape)}, expected {shape}")
    return out


def _env_seed() -> Optional[int]:
    raw = os.environ.get("ATLASPATCH_RANDOM_INIT")
    return int(raw) if raw not in (None, "") else None
