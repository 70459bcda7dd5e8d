"""The transform of a plugin's torch module, described so that the device can run it.

``DeviceTransform`` states the chain ``Resize -> CenterCrop -> ToTensor -> Normalize`` on a PIL RGB image, the chain every
torchvision-style ``preprocess`` of the reference's encoders is built from, and runs it on a device batch of uint8 tiles:
``ap_resample_u8`` gives Pillow's bytes for the resize, ``ap_preproc_u8hwc_to_chw`` (``_any`` for a width that is no
multiple of 8) takes the crop window and does ToTensor + Normalize in torchvision's arithmetic.  The result equals the host
chain bit for bit in float32, and its ``.to(dtype)`` in float16 / bfloat16.

torchvision is not a dependency; its rules are restated here (torchvision 0.15 - 0.20, transforms/functional.py and
transforms/_functional_pil.py):

* ``Resize(int)``: ``_compute_resized_output_size`` -- shorter side -> ``size``, the other side ``int(size * long / short)``;
  ``resize`` returns the image untouched when the shorter side already equals ``size``.  ``Resize((h, w))``: exactly that size.
  On a PIL image the resize is ``Image.resize((w, h), interpolation)``; ``antialias`` has no effect there.
* ``CenterCrop``: ``center_crop`` -- ``crop_top = int(round((H - h) / 2.0))``, ``crop_left = int(round((W - w) / 2.0))`` with
  Python's ``round`` (half to even).  A crop larger than the image pads in torchvision; here it is refused.
* ``ToTensor``: uint8 HWC -> float32 CHW, ``/ 255``.  ``Normalize``: ``(x - mean[c]) / std[c]``.
"""
from __future__ import annotations

from typing import Optional

PILLOW_FILTERS = {0: "nearest", 1: "lanczos", 2: "bilinear", 3: "bicubic", 4: "box", 5: "hamming"}      # Image.Resampling
_DEVICE_FILTERS = ("bilinear", "bicubic", "lanczos", "box", "hamming")


def _filter_name(interpolation) -> str:
    """A Pillow code, a name, or an object whose ``.value`` is a name (torchvision's InterpolationMode) -> the table's name."""
    raw = interpolation
    if not isinstance(raw, (int, str)) and hasattr(raw, "value"):
        raw = raw.value
    if isinstance(raw, bool):
        raise ValueError(f"DeviceTransform: interpolation {interpolation!r} is not a Pillow filter")
    name = PILLOW_FILTERS.get(raw) if isinstance(raw, int) else (raw.lower() if isinstance(raw, str) else None)
    if name in ("nearest", "nearest-exact"):
        raise ValueError(f"DeviceTransform: interpolation '{name}' is not a coefficient table (Pillow's nearest picks "
                         "pixels); the device resampler runs bilinear, bicubic, lanczos, box and hamming")
    if name not in _DEVICE_FILTERS:
        raise ValueError(f"DeviceTransform: interpolation {interpolation!r} is not a Pillow filter "
                         f"(codes 1-5, or one of {', '.join(_DEVICE_FILTERS)})")
    return name


def _pair(value, what: str) -> tuple:
    """int or 1-sequence -> (v, v); (h, w) -> (h, w)."""
    if isinstance(value, bool):
        raise ValueError(f"DeviceTransform: {what} {value!r} is not a size")
    if isinstance(value, int):
        pair = (value, value)
    else:
        seq = tuple(int(v) for v in value)
        if len(seq) not in (1, 2):
            raise ValueError(f"DeviceTransform: {what} {value!r} must be an int or (h, w)")
        pair = (seq[0], seq[-1])
    if pair[0] <= 0 or pair[1] <= 0:
        raise ValueError(f"DeviceTransform: {what} {value!r} must be positive")
    return pair


def _triple(value, what: str) -> tuple:
    if hasattr(value, "tolist"):
        value = value.tolist()
    seq = tuple(float(v) for v in value) if isinstance(value, (tuple, list)) else (float(value),)
    if len(seq) == 1:
        seq = seq * 3
    if len(seq) != 3:
        raise ValueError(f"DeviceTransform: {what} must have one value or three, got {len(seq)}")
    return seq


class DeviceTransform:
    """``Resize(resize, interpolation) -> CenterCrop(crop) -> ToTensor() -> Normalize(mean, std)`` on RGB tiles.

    resize : ``None`` (no resize), an int (shorter side -> size, aspect kept) or ``(h, w)``.
    interpolation : a Pillow code (2 bilinear, 3 bicubic, 1 lanczos, 4 box, 5 hamming), one of those names, or an object whose
        ``.value`` is one (``InterpolationMode``).  ``nearest`` is refused.
    crop : ``None``, an int or ``(h, w)``: the centre crop after the resize.
    mean, std : per channel (or one value for all three).
    """

    def __init__(self, resize=None, interpolation="bilinear", crop=None, mean=(0, 0, 0), std=(1, 1, 1)) -> None:
        if resize is None or (isinstance(resize, int) and not isinstance(resize, bool)):
            self.resize = resize
            if resize is not None and resize <= 0:
                raise ValueError(f"DeviceTransform: resize {resize!r} must be positive")
        else:
            seq = tuple(resize)
            self.resize = int(seq[0]) if len(seq) == 1 else _pair(seq, "resize")     # Resize([s]) is Resize(s)
        self.filter = _filter_name(interpolation)
        self.crop = None if crop is None else _pair(crop, "crop")
        self.mean, self.std = _triple(mean, "mean"), _triple(std, "std")
        if any(s == 0 for s in self.std):
            raise ValueError(f"DeviceTransform: std {self.std} has a zero (Normalize would divide by it)")
        self._plans: dict = {}
        self._resamplers: dict = {}

    def __repr__(self) -> str:
        return (f"DeviceTransform(resize={self.resize}, interpolation='{self.filter}', crop={self.crop}, "
                f"mean={self.mean}, std={self.std})")

    # ------------------------------------------------------------------ pure Python
    def plan(self, in_hw) -> tuple:
        """``(resized_hw, crop_top, crop_left, out_hw)`` for tiles of ``in_hw = (H, W)``; ``ValueError`` when the crop is
        larger than the resized image."""
        key = (int(in_hw[0]), int(in_hw[1]))
        hit = self._plans.get(key)
        if hit is not None:
            return hit
        if key[0] <= 0 or key[1] <= 0:
            raise ValueError(f"DeviceTransform: tile size {key} must be positive")
        if self.resize is None:
            rh, rw = key
        elif isinstance(self.resize, int):
            from ..utils.resample import shorter_side_hw
            rh, rw = shorter_side_hw(key, self.resize)
        else:
            rh, rw = self.resize
        if self.crop is None:
            top, left, oh, ow = 0, 0, rh, rw
        else:
            oh, ow = self.crop
            if oh > rh or ow > rw:
                raise ValueError(f"DeviceTransform: crop {oh}x{ow} (h x w) is larger than the resized image {rh}x{rw} "
                                 f"(tiles of {key[0]}x{key[1]}); torchvision would pad, the device transform does not")
            top, left = int(round((rh - oh) / 2.0)), int(round((rw - ow) / 2.0))
        if len(self._plans) > 64:
            self._plans.clear()
        self._plans[key] = out = ((rh, rw), top, left, (oh, ow))
        return out

    def host(self, image):
        """The same chain on one PIL image (or uint8 HWC array) with Pillow and torch on the CPU -> float32 [3, oh, ow]: a
        ``preprocess`` for plugins whose environment has no torchvision, and the statement the device route is tested against."""
        import numpy as np
        import torch
        from PIL import Image
        if not isinstance(image, Image.Image):
            image = Image.fromarray(np.asarray(image))
        image = image.convert("RGB")
        (rh, rw), top, left, (oh, ow) = self.plan((image.height, image.width))
        if (rh, rw) != (image.height, image.width):
            code = {v: k for k, v in PILLOW_FILTERS.items()}[self.filter]
            image = image.resize((rw, rh), code)
        arr = np.asarray(image)[top:top + oh, left:left + ow]
        x = torch.from_numpy(np.array(arr, order="C")).permute(2, 0, 1).to(torch.float32) / 255
        mean = torch.tensor(self.mean, dtype=torch.float32).view(3, 1, 1)
        std = torch.tensor(self.std, dtype=torch.float32).view(3, 1, 1)
        return ((x - mean) / std).contiguous()

    # ------------------------------------------------------------------ device
    def __call__(self, tiles_u8, dtype):
        """uint8 [n, H, W, 3] on the device -> ``dtype`` [n, 3, oh, ow] on the same device; enqueued on the current stream."""
        import torch
        from .. import _lib
        if not (tiles_u8.is_cuda and tiles_u8.dtype == torch.uint8 and tiles_u8.dim() == 4 and tiles_u8.shape[3] == 3):
            raise ValueError(f"DeviceTransform: tiles must be uint8 [n, H, W, 3] on the device, got {tiles_u8.dtype} "
                             f"{tuple(tiles_u8.shape)} on {tiles_u8.device}")
        n, h, w = int(tiles_u8.shape[0]), int(tiles_u8.shape[1]), int(tiles_u8.shape[2])
        (rh, rw), top, left, (oh, ow) = self.plan((h, w))
        code = _lib.torch_dtype_code(dtype)
        out = torch.empty((n, 3, oh, ow), dtype=dtype, device=tiles_u8.device)
        if n == 0:
            return out
        x = tiles_u8.contiguous()
        if (rh, rw) != (h, w):
            key = (h, w, str(x.device))
            rs = self._resamplers.get(key)
            if rs is None:
                from ..utils.resample import DeviceResampler
                rs = self._resamplers[key] = DeviceResampler((h, w), (rh, rw), self.filter, x.device)
            x = rs(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().ap_preproc_u8hwc_to_chw_any(x.data_ptr(), n, rh, rw, top, left, oh, ow, _lib.f3(self.mean),
                                                               _lib.f3(self.std), out.data_ptr(), code,
                                                               _lib.current_stream_ptr(x.device)), "ap_preproc_u8hwc_to_chw_any")
        return out

    # ------------------------------------------------------------------ from a torchvision Compose
    @classmethod
    def from_torchvision(cls, compose) -> "DeviceTransform":
        """Read a ``Compose``-like object by duck typing (class names and attributes; torchvision is not imported):
        ``[Resize] -> [CenterCrop] -> ToTensor -> [Normalize]``.  ``ValueError`` names the first thing the device cannot
        reproduce.  Nothing calls this implicitly: a plugin author does, and passes the result as ``device_transform``."""
        ops = getattr(compose, "transforms", None)
        if ops is None:
            raise ValueError(f"DeviceTransform.from_torchvision: {type(compose).__name__} has no .transforms (a Compose is expected)")
        order = ("Resize", "CenterCrop", "ToTensor", "Normalize")
        kw: dict = {}
        stage = -1
        seen_tensor = False
        for op in ops:
            name = type(op).__name__
            if name not in order:
                raise ValueError(f"DeviceTransform.from_torchvision: {name} is not one of Resize, CenterCrop, ToTensor, "
                                 "Normalize; the device cannot reproduce it")
            at = order.index(name)
            if at <= stage:
                raise ValueError(f"DeviceTransform.from_torchvision: {name} after {order[stage]}: the device runs "
                                 "Resize -> CenterCrop -> ToTensor -> Normalize, each at most once, in this order")
            if name == "Normalize" and not seen_tensor:
                raise ValueError("DeviceTransform.from_torchvision: Normalize before ToTensor (ToTensor is missing or comes later)")
            stage = at
            if name == "Resize":
                if getattr(op, "max_size", None) is not None:
                    raise ValueError(f"DeviceTransform.from_torchvision: Resize(max_size={op.max_size}) is not supported")
                if getattr(op, "antialias", True) is False:
                    raise ValueError("DeviceTransform.from_torchvision: Resize(antialias=False) is not supported "
                                     "(Pillow's resize, which the device reproduces, always antialiases)")
                kw["resize"] = op.size
                kw["interpolation"] = getattr(op, "interpolation", "bilinear")
            elif name == "CenterCrop":
                kw["crop"] = op.size
            elif name == "ToTensor":
                seen_tensor = True
            else:
                kw["mean"], kw["std"] = op.mean, op.std
        if not seen_tensor:
            raise ValueError("DeviceTransform.from_torchvision: ToTensor is missing (the chain must turn the image into a tensor)")
        return cls(**kw)


__all__ = ["DeviceTransform", "PILLOW_FILTERS"]
