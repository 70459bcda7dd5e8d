"""ViT-family encoders on the native HIP path.  ``HipViT`` owns the ``ap_vit`` handle and its HBM workspace (``forward_u8`` /
``forward_chw`` launch on torch's current stream); ``vit_config`` is the structure it is created from.  ``build_hip_vit_extractor``
and the ``register_*`` functions go from a name of ``vit_archs`` and a checkpoint (``vit_checkpoints.to_canonical``) to a feature
extractor.  What those two modules define is importable from here as well."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .. import _lib
from .base import HipViTFeatureExtractor, NativeEncoder
from .checkpoints import (IMAGENET_MEAN, IMAGENET_STD, OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, _env_seed,  # noqa: F401 (re-exported)
                          check_canonical, load_checkpoint, resolve_weights, weights_path)
from .vit_archs import ARCHS, MAX_BATCH, TRANSFORM_NORM, TRANSFORM_RESIZE
from .vit_checkpoints import (LAYOUTS, POOLER_KEYS, _detect_source, attn_pool_canonical, attn_tower_canonical_shapes,  # noqa: F401
                              canonical_shapes, canonical_state_dict, coca_canonical_state_dict, conch_state_dicts,
                              conch_v15_canonical_state_dict, dinov3_rope_tables, pad_heads, pad_mlp, random_attn_pool,
                              random_canonical_state_dict, resample_position_grid, siglip_canonical_shapes,
                              siglip_canonical_state_dict, stored_head_dim, stored_mlp_dim, to_canonical)

POOL_CODES = {"attn": 1, "cls_mean": 2, "map": 3}      # attentional pooler | [class token | mean of the patch tokens] | SigLIP's head
ACT_CODES = {"quick_gelu": 1, "gelu_tanh": 2}          # 0 = erf GELU


def vit_config(arch: dict, dtype: torch.dtype):
    """The structure ``ap_vit_create`` takes for ``arch``.  Heads and MLP are given as the device stores them (``stored_head_dim``,
    ``stored_mlp_dim``); ``attn_scale`` is 1 / sqrt(true head width) where the stored width differs, else 0 (= the default); the
    true width is dim / heads unless ``arch`` has a "head_dim" (attention narrower than the stream: no model of the zoo).  The
    fields appended since ABI v20 travel in the longer structures only when one of them is set: ``VitConfigEx`` (96 bytes) for
    ``no_class_token``, ``VitConfigEx2`` (112 bytes) for the CoCa / CONCH v1.5 pooler's; every other model hands over the 92 bytes
    of ``VitConfig``, as before."""
    flag = lambda key: 1 if arch.get(key) else 0
    hd_true = int(arch.get("head_dim") or arch["dim"] // arch["heads"])        # "head_dim": heads narrower than dim / heads
    hd_stored = stored_head_dim(arch["dim"], arch["heads"], hd_true)
    fields = dict(
        image_size=arch["image_size"], patch_size=arch["patch_size"], dim=arch["dim"], depth=arch["depth"], heads=arch["heads"],
        mlp_dim=stored_mlp_dim(arch["mlp_dim"]), ln_eps=float(arch["ln_eps"]), layer_scale=flag("layer_scale"),
        compute_dtype=_lib.torch_dtype_code(dtype), pool=POOL_CODES.get(arch.get("pool"), 0), pool_dim=int(arch.get("pool_dim", 0)),
        pool_heads=int(arch.get("pool_heads", 0)), pool_ln_eps=float(arch.get("pool_ln_eps", 1e-5)),
        reg_tokens=int(arch.get("reg_tokens", 0)), no_embed_class=flag("no_embed_class"),
        mlp_type=1 if arch.get("mlp") == "swiglu" else 0, head_dim=hd_stored,
        attn_scale=0.0 if hd_stored == hd_true else float(1.0 / np.sqrt(np.float32(hd_true))),
        pre_norm=flag("pre_norm"), act=ACT_CODES.get(arch.get("act"), 0), proj_dim=int(arch.get("proj_dim", 0)), rope=flag("rope"))
    ex2 = dict(pool_head_dim=int(arch.get("pool_head_dim", 0)), pool_skip_final_norm=flag("pool_skip_final_norm"),
               pool_proj_dim=int(arch.get("pool_proj_dim", 0)), out_normalize=flag("out_normalize"))
    if any(ex2.values()):
        return _lib.VitConfigEx2(**fields, no_class_token=flag("no_class_token"), **ex2)
    if arch.get("no_class_token"):
        return _lib.VitConfigEx(**fields, no_class_token=1)
    return _lib.VitConfig(**fields)


# ----------------------------------------------------------------------------- device object
class HipViT(NativeEncoder):
    """Device-resident ViT encoder behind ``ap_vit_*``."""

    ABI = "vit"
    PROF_KINDS = _lib.PROF_KINDS

    def __init__(self, arch: dict, state: dict, *, device: torch.device, dtype: torch.dtype) -> None:
        self._bind(device, dtype)
        self.arch = dict(arch)
        # features: the pooler's (attn), [class token | mean patch token] (cls_mean), else dim floats; a projection's output if any
        self.embed_dim = int(arch.get("pool_proj_dim") or arch.get("proj_dim") or
                             {"attn": arch.get("pool_dim"), "cls_mean": 2 * arch["dim"]}.get(arch.get("pool"), arch["dim"]))
        state = pad_heads(state, dim=arch["dim"], heads=arch["heads"], depth=arch["depth"], head_dim=arch.get("head_dim"))
        state = pad_mlp(state, mlp_dim=arch["mlp_dim"], depth=arch["depth"], swiglu=arch.get("mlp") == "swiglu")
        self._open(vit_config(arch, dtype), state)

    def _upload(self, arrs: dict) -> None:
        # one native call for the whole checkpoint: the uploads run outside the interpreter lock (the encoder is built on a
        # side thread while the CLI's phase 1 runs)
        n = len(arrs)
        names = (C.c_char_p * n)(*[k.encode() for k in arrs])
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs.values()])
        counts = (C.c_size_t * n)(*[a.size for a in arrs.values()])
        _lib.check(self.lib.ap_vit_set_params(self._handle, names, ptrs, counts, n), "ap_vit_set_params")

    def forward_chw(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x: [n, 3, S, S] float32 or compute dtype, already normalised."""
        self._live()
        assert x.is_contiguous() and x.dim() == 4
        n = x.shape[0]
        if out is None:
            out = torch.empty((n, self.embed_dim), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        ws = self._ws(n)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ap_vit_forward_chw(self._handle, x.data_ptr(), _lib.torch_dtype_code(x.dtype), n,
                                                   out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _lib.current_stream_ptr(self.device)), "ap_vit_forward_chw")
        return out

    OPTIONS = {"full_last_block": 0, "two_half_overlap": 1, "f32_stream": 2, "exact_cls": 3, "split_f16": 4}

    def set_option(self, name: str, on: bool) -> None:
        """``full_last_block``: the last block for every token instead of the CLS row only; ``two_half_overlap``: a
        batch >= 512 as two halves on two streams.  Both leave the features unchanged (tested).  ``f32_stream``
        (f16 / bf16): float32 residual stream with standalone add+LayerNorm launches instead of the fused-LayerNorm
        dataflow (slower).  ``exact_cls`` (default ON; f16 / bf16 fused dataflow with a class-token pooling): the class rows'
        residual stream is additionally carried in float32, which removes most of the 16-bit stream's error from the features
        (ViT-B/16 float16: 1.26e-3 -> 8.0e-4 against the CPU fp32 path, 1.5 % of the step); off = the plain 16-bit stream.
        ``split_f16`` (float32 only): the GEMMs' inner products as three f16 MFMA passes on hi / lo halves with f32
        accumulation instead of the exact f32 MFMA -- every buffer, LayerNorm, softmax and the stream stay float32."""
        value = int(on) if not isinstance(on, bool) else (1 if on else 0)
        _lib.check(self.lib.ap_vit_set_option(self._handle, self.OPTIONS[name], value), "ap_vit_set_option")


# ----------------------------------------------------------------------------- builders
def build_hip_vit_extractor(*, name: str, arch, device, dtype, state_dict: Optional[dict] = None,
                            mean=None, std=None, source: str = "auto", max_batch: int = 1024,
                            random_init_seed: Optional[int] = None, resize=None,
                            expect_size: Optional[int] = 256, **arch_overrides) -> HipViTFeatureExtractor:
    spec = dict(ARCHS[arch]) if isinstance(arch, str) else dict(arch)
    spec.update(arch_overrides)
    state_dict, seeded = resolve_weights(name, state_dict, random_init_seed, lambda seed: random_canonical_state_dict(spec, seed),
                                         "torchvision, timm or HF ViT")
    state, layer_scale = to_canonical(state_dict, spec, "canonical" if seeded else source)
    if layer_scale != bool(spec.get("layer_scale")):                 # conch_v15: the checkpoint decides
        spec["layer_scale"] = layer_scale
    vit = HipViT(spec, state, device=torch.device(device), dtype=dtype)
    extractor = SquareResizeFeatureExtractor if spec.get("square_resize") else HipViTFeatureExtractor
    return extractor(name=name, vit=vit, mean=mean or IMAGENET_MEAN, std=std or IMAGENET_STD,
                     max_batch=max_batch, resize=resize, expect_size=expect_size)


class SquareResizeFeatureExtractor(HipViTFeatureExtractor):
    """``resize`` = (S, filter) means S x S whatever the tile's aspect -- transformers' SiglipImageProcessor (``size: {height, width}``,
    no crop) -- instead of torchvision's shorter-side ``Resize(S)``.  Square tiles, the usual case, come out the same."""

    def resized(self, tiles_u8: torch.Tensor) -> torch.Tensor:
        size, filt = self.resize
        h, w = int(tiles_u8.shape[1]), int(tiles_u8.shape[2])
        if h == size and w == size:
            return tiles_u8
        rs = self._resamplers.get((h, w))
        if rs is None:
            from ..utils.resample import DeviceResampler
            rs = self._resamplers[(h, w)] = DeviceResampler((h, w), (size, size), filt, self.device)
        return rs(tiles_u8)


PIL_RESAMPLE_NAMES = {0: "nearest", 2: "bilinear", 3: "bicubic"}     # PIL.Image.Resampling codes a preprocessor_config.json holds


def medsiglip_transform(weights_dir: Optional[str] = None) -> tuple:
    """(size, filter, mean, std) of the medsiglip preprocess: ``TRANSFORM_RESIZE`` / ``TRANSFORM_NORM`` (the public model card's
    values, unverifiable offline) unless ``<weights_dir>/medsiglip.preprocessor_config.json`` -- the processor config published
    with the checkpoint -- is there, whose ``size``, ``resample``, ``image_mean`` and ``image_std`` then win."""
    import json
    size, filt = TRANSFORM_RESIZE["medsiglip"]
    mean, std = TRANSFORM_NORM["medsiglip"]
    root = weights_dir if weights_dir is not None else os.environ.get("ATLASPATCH_WEIGHTS_DIR")
    path = Path(root) / "medsiglip.preprocessor_config.json" if root else None
    if path is not None and path.exists():
        cfg = json.loads(path.read_text())
        if "size" in cfg:
            sz = cfg["size"]
            h, w = (sz["height"], sz["width"]) if isinstance(sz, dict) else (sz, sz)
            if int(h) != int(w):
                raise ValueError(f"{path}: size {sz} is not square")
            size = int(h)
        if "resample" in cfg:
            if int(cfg["resample"]) not in PIL_RESAMPLE_NAMES or PIL_RESAMPLE_NAMES[int(cfg["resample"])] == "nearest":
                raise ValueError(f"{path}: resample {cfg['resample']} is not a filter of the device resize (2 bilinear, 3 bicubic)")
            filt = PIL_RESAMPLE_NAMES[int(cfg["resample"])]
        if "image_mean" in cfg:
            mean = tuple(float(v) for v in cfg["image_mean"])
        if "image_std" in cfg:
            std = tuple(float(v) for v in cfg["image_std"])
    return size, filt, mean, std


def fit_max_batch(vit: "HipViT", cap: int, budget_bytes: int = 16 << 30) -> int:
    """The largest batch <= cap whose ``ap_vit_workspace_bytes`` fits the budget (medsiglip, 1024 tokens of 1152: ~90 MB per image
    in float16)."""
    n = cap
    while n > 1 and int(vit.lib.ap_vit_workspace_bytes(vit._handle, n)) > budget_bytes:
        n //= 2
    return n


def refuse_float32(name: str, spec: dict, dtype: torch.dtype) -> None:
    """The float32 attention kernel takes 288 tokens and 64-wide heads: a larger model says so before any device work."""
    tokens = (0 if spec.get("no_class_token") else 1) + (spec["image_size"] // spec["patch_size"]) ** 2
    if dtype == torch.float32 and (tokens > 288 or stored_head_dim(spec["dim"], spec["heads"]) != 64):
        raise ValueError(f"{name}: --feature-precision float32 is not available: {tokens} tokens with heads stored "
                         f"{stored_head_dim(spec['dim'], spec['heads'])} wide exceed the float32 attention kernel's limits (288 "
                         "tokens, 64 wide); use float16 or bfloat16")


def _register(registry, names, *, device, dtype, tower: bool = False, extra=None, **arch_overrides) -> None:
    """Register ``names``, each built from what the four tables of ``vit_archs`` hold for it.  ``tower`` (the plugins' pooled
    towers): the architecture takes ``arch_overrides``, float32 is refused where the attention kernel has no float32 form, and
    ``MAX_BATCH`` is a cap that ``fit_max_batch`` lowers to the workspace budget; ``extra(name, spec)`` gives builder arguments
    that replace the tables'."""
    def build(name):
        mean, std = TRANSFORM_NORM.get(name, (IMAGENET_MEAN, IMAGENET_STD))
        kw = dict(name=name, arch=name, device=device, dtype=dtype, random_init_seed=_env_seed(), mean=mean, std=std,
                  resize=TRANSFORM_RESIZE[name], expect_size=None, max_batch=MAX_BATCH[name])
        if not tower:
            return build_hip_vit_extractor(**kw)
        spec = kw["arch"] = dict(ARCHS[name], **arch_overrides)
        refuse_float32(name, spec, dtype)
        kw.update(extra(name, spec) if extra else {})
        ex = build_hip_vit_extractor(**kw)
        ex.max_batch = fit_max_batch(ex.vit, MAX_BATCH[name])
        return ex
    for name in names:
        registry.register(name, lambda n=name: build(n))


def register_medsiglip(registry, *, device, dtype=torch.float32, num_workers: int = 0, **arch_overrides) -> None:
    """medsiglip (models/patch/medsiglip.py): transformers' SiglipVisionModel of google/medsiglip-448, features =
    ``get_image_features`` = ``pooler_output`` of the vision tower (the attention-pooling head's 1152 floats).  Transform: the
    processor's resize to 448 x 448 (bilinear), rescale, Normalize(0.5, 0.5) -- resize and normalisation on the device.  float16 /
    bfloat16 only: 1024 tokens and 72-wide heads are outside the float32 attention kernel's limits.  HF state dict (vision tower
    alone or the whole SiglipModel) as ``$ATLASPATCH_WEIGHTS_DIR/medsiglip.safetensors``."""
    def transform(name, spec):
        size, filt, mean, std = medsiglip_transform()
        if size != spec["image_size"]:
            raise ValueError(f"medsiglip: the preprocessor config resizes to {size}, the model takes {spec['image_size']}")
        return dict(mean=mean, std=std, resize=(size, filt), square_resize=True)
    _register(registry, ["medsiglip"], device=device, dtype=dtype, tower=True, extra=transform, **arch_overrides)


def register_coca_towers(registry, *, device, dtype=torch.float32, num_workers: int = 0, **arch_overrides) -> None:
    """omiclip (models/patch/omiclip.py: open_clip ``coca_ViT-L-14``, ``encode_image``) and conch_v15 (models/patch/conch.py:67-112:
    ``build_conch(ConchConfig())`` of the TITAN repository): ViT-L trunks whose features come from an attentional pooler with eight
    96-wide heads over the 1024-wide tokens.  Both architectures are restated from the public packages, unverified offline (see
    ``ARCHS``).  Transform: Pillow-exact bicubic resize of the shorter side to 224 / 448 and the centre crop on the device, OpenAI
    CLIP / ImageNet constants.  Weights: ``$ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth}`` (omiclip: ``visual.*`` bare or
    prefixed, or the whole CoCa model; conch_v15: ``trunk.*`` / ``attn_pool_contrast.*`` / ``ln_contrast.*``, bare or under
    ``visual.`` / ``vision_encoder.``) or ``ATLASPATCH_RANDOM_INIT=<seed>``.  omiclip runs in float32 too (257 tokens); conch_v15
    (785 tokens) in float16 / bfloat16 only.  Not in the default registry: ``plugins/coca_towers.py`` ships them."""
    layout = {"omiclip": "open_clip_coca", "conch_v15": "conch_v15"}     # neither is auto-detected
    _register(registry, ["omiclip", "conch_v15"], device=device, dtype=dtype, tower=True,
              extra=lambda name, spec: dict(source=layout[name]), **arch_overrides)


def register_conch(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """conch_v1 (models/patch/conch.py:20-64): open_clip image transform = Resize(448, bicubic) + CenterCrop(448)
    + ToTensor + Normalize(OpenAI CLIP mean / std) [3P]; all of it on the device (the resize is Pillow-exact,
    ap_resample_u8).  float16 / bfloat16 only (the reference's config 5 runs it in fp16)."""
    _register(registry, ["conch_v1"], device=device, dtype=dtype)


def register_vits(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """vit_b_16 / vit_l_16 with torchvision's transform semantics: ImageClassification(crop 224, resize R, bilinear)
    on the PIL tile (models/patch/base.py:42-45 hands the transform a PIL image, so the resize is Pillow's BILINEAR),
    R = 256 for vit_b_16 and 242 for vit_l_16 (``TRANSFORM_RESIZE``).  vit_b_16 on the default 256-px tiles is a pure
    centre crop; vit_l_16 resamples every 256-px tile to 242 first; any other --patch-size goes through the same
    Pillow-exact device resize (shorter side -> R)."""
    # ... and vit_b_32 / vit_l_32 / vit_h_14, the other three names of models/patch/vit.py:9-15 (see ``ARCHS``, ``TRANSFORM_RESIZE``)
    _register(registry, ["vit_b_16", "vit_l_16", "vit_b_32", "vit_l_32", "vit_h_14"], device=device, dtype=dtype)


def register_uni(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """uni_v1: timm ViT-L/16 + LayerScale; timm transform Resize(224, bicubic) + CenterCrop(224):
    the resize runs on the device bit-identically to Pillow (ap_resample_u8), the crop in the preprocess kernel."""
    # uni_v2 = UNI2-h (uni.py:62-125): same timm transform; checkpoint: timm key names (pytorch_model.bin of MahmoodLab/UNI2-h)
    _register(registry, ["uni_v1", "uni_v2"], device=device, dtype=dtype)


def register_dinov2(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """dinov2_small / base / large / giant (models/patch/dinov2.py:12-17): the reference runs transformers' Dinov2Model on the
    processor's output and returns the class token of ``last_hidden_state``.  Same device kernels as the other encoders (LayerScale
    folded, giant: SwiGLU gate in the fc1 epilogue); checkpoints: the HF state dict (model.safetensors of facebook/dinov2-*) as
    ``$ATLASPATCH_WEIGHTS_DIR/<name>.safetensors``."""
    _register(registry, ["dinov2_small", "dinov2_base", "dinov2_large", "dinov2_giant"], device=device, dtype=dtype)


def register_phikon(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """phikon_v1 (transformers ViTModel, ViT-B/16, LayerNorm eps 1e-12) and phikon_v2 (Dinov2Model ViT-L/16), models/patch/phikon.py:
    class token of ``last_hidden_state``.  HF state dicts in ATLASPATCH_WEIGHTS_DIR."""
    _register(registry, ["phikon_v1", "phikon_v2"], device=device, dtype=dtype)


def register_more_vits(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """The other loader files whose model is a plain ViT this engine runs: midnight (models/patch/midnight.py, transformers
    Dinov2Model giant, class token + mean patch token), h_optimus_0 / h_optimus_1 (hoptimus.py), prov_gigapath (gigapath.py),
    virchow_v1 / virchow_v2 (virchow.py: 80-wide heads and a 3416-wide SwiGLU stored zero-padded, class | mean patch token),
    the two Lunit ViT-S (lunit.py) and pathorchestra (pathorchestra.py).  Checkpoints: HF (midnight) or timm key names in
    ATLASPATCH_WEIGHTS_DIR; each with the transform its loader file writes out (``TRANSFORM_RESIZE`` / ``TRANSFORM_NORM``)."""
    _register(registry, ["midnight", "h_optimus_0", "h_optimus_1", "prov_gigapath", "virchow_v1", "virchow_v2", "h0_mini",
                         "lunit_vit_small_patch16_dino", "lunit_vit_small_patch8_dino", "pathorchestra"], device=device, dtype=dtype)


def register_clip(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """The CLIP vision towers with a plain ViT: clip_vit_b_32 / b_16 / l_14 / l_14_336 (models/patch/clip.py, open_clip, OpenAI
    weights), plip (plip.py) and quilt_b_32 / quilt_b_16 (quilt.py), both transformers CLIPModel; features = encode_image /
    get_image_features (projected, not normalised); biomedclip (biomedclip.py: timm ViT-B/16 trunk + linear projection).  Checkpoints: open_clip or HF CLIP state dicts in ATLASPATCH_WEIGHTS_DIR.
    (The ResNet CLIPs, quilt_b_16_pmb and omiclip are other architectures.)"""
    _register(registry, ["clip_vit_b_32", "clip_vit_b_16", "clip_vit_l_14", "clip_vit_l_14_336", "plip", "quilt_b_32", "quilt_b_16",
                         "biomedclip"], device=device, dtype=dtype)


def register_dinov3(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """dinov3_vits16 / vits16_plus / vitb16 / vitl16 / vitl16_sat / vith16_plus / vit7b16 / vit7b16_sat (models/patch/dinov3.py:12-21):
    transformers' DINOv3ViTModel, ``pooler_output``.  Rotary position embedding applied in place on q / k after the qkv GEMM (``ap::launch_rope``);
    HF state dicts in ATLASPATCH_WEIGHTS_DIR."""
    _register(registry, ["dinov3_vits16", "dinov3_vits16_plus", "dinov3_vitb16", "dinov3_vitl16", "dinov3_vitl16_sat",
                         "dinov3_vith16_plus", "dinov3_vit7b16", "dinov3_vit7b16_sat"], device=device, dtype=dtype)
