"""Backend registry keyed by file extension (reference: core/wsi/wsi_factory.py:12-141), with the
synthetic backend mapped to ``.synth``.

``ATLASPATCH_TIFF_NATIVE=1`` (opt-in) sends ``.svs`` / ``.tif`` / ``.tiff`` files that ``ap_host_tiff_open`` accepts -- tiled TIFF
with JPEG tiles -- to the native ``tiff`` backend (tiff_wsi.py); a file it refuses, and every file with the switch unset, goes
to ``openslide`` as before.  ``backend="tiff"`` works either way."""
from __future__ import annotations

import os
from pathlib import Path
from typing import Optional

from .image_wsi import ImageWSI
from .iwsi import IWSI
from .openslide_wsi import OpenSlideWSI
from .synth_wsi import SynthWSI
from .tiff_wsi import TiffWSI

_OPENSLIDE_EXT = (".svs", ".tif", ".tiff", ".ndpi", ".vms", ".vmu", ".scn", ".mrxs", ".bif", ".biff",
                  ".dcm", ".dicom")
_IMAGE_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".webp", ".gif")
_TIFF_NATIVE_EXT = (".svs", ".tif", ".tiff")


class WSIFactory:
    _registry = {"openslide": OpenSlideWSI, "image": ImageWSI, "synth": SynthWSI}
    # backends that are reached by name (or by detect() under their switch) and are NOT tried by try_load's default sweep, so that
    # the registry's contents -- and with them every default path -- stay what they were
    _by_name = {"tiff": TiffWSI}
    _formats = {**{e: "openslide" for e in _OPENSLIDE_EXT}, **{e: "image" for e in _IMAGE_EXT},
                ".synth": "synth"}

    @classmethod
    def register(cls, name: str, impl_class) -> None:
        cls._registry[name] = impl_class

    @classmethod
    def map_extension(cls, ext: str, backend: str) -> None:
        if backend not in cls._registry:
            raise ValueError(f"Unknown backend: {backend}")
        cls._formats[(ext if ext.startswith(".") else "." + ext).lower()] = backend

    @classmethod
    def detect(cls, path: str) -> Optional[str]:
        ext = Path(path).suffix.lower()
        backend = cls._formats.get(ext)
        if backend == "openslide" and ext in _TIFF_NATIVE_EXT and cls._tiff_native(path):
            return "tiff"
        return backend

    @staticmethod
    def _tiff_native(path: str) -> bool:
        """ATLASPATCH_TIFF_NATIVE=1 and ``ap_host_tiff_open`` accepts the file."""
        from ...utils.env import env_flag
        if not env_flag("ATLASPATCH_TIFF_NATIVE") or not os.path.isfile(path):
            return False
        from ... import _lib
        from .tiff_wsi import open_native
        handle, _ = open_native(path)
        if handle is None:
            return False
        _lib.load().ap_host_tiff_close(handle)
        return True

    @classmethod
    def load(cls, path: str, backend: Optional[str] = None, mpp: Optional[float] = None, **kwargs) -> IWSI:
        if not os.path.exists(path):
            raise FileNotFoundError(f"File not found: {path}")
        if backend is None:
            backend = cls.detect(path)
            if backend is None:
                raise ValueError(f"No backend found for: {path}")
        elif backend not in cls._registry and backend not in cls._by_name:
            raise ValueError(f"Unknown backend: {backend}")
        impl = cls._registry.get(backend) or cls._by_name[backend]
        return impl(path=path, mpp=mpp, **kwargs)

    @classmethod
    def try_load(cls, path: str, backends: Optional[list] = None, mpp: Optional[float] = None, **kwargs) -> IWSI:
        if not os.path.exists(path):
            raise FileNotFoundError(f"File not found: {path}")
        problems = []
        for name in (backends if backends is not None else list(cls._registry)):
            if name not in cls._registry and name not in cls._by_name:
                problems.append(f"{name}: not registered")
                continue
            try:
                return cls.load(path, backend=name, mpp=mpp, **kwargs)
            except Exception as exc:  # noqa: BLE001
                problems.append(f"{name}: {exc}")
        raise RuntimeError(f"All backends failed for {path}:\n" + "\n".join(problems))
