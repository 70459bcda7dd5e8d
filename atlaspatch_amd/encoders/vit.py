"""ViT-family encoders on the native HIP path.

* ``ARCHS``: the shapes the reference registers as ``vit_b_16`` / ``vit_l_16``
  (/root/reference/atlas_patch/models/patch/vit.py:9-15, torchvision) and ``uni_v1``
  (models/patch/uni.py:13-60, timm ViT-L/16 with LayerScale).
* ``canonical_state_dict``: adapters from torchvision / timm / HF ``ViTModel`` key names to the
  parameter names of ``ap_vit_set_param``.  QKV is packed ``[q; k; v]`` rows.
* ``HipViT``: owns the ``ap_vit`` handle and its HBM workspace; ``forward_u8`` / ``forward_chw``
  launch on torch's current stream.
"""
from __future__ import annotations

import ctypes as C
import re
import os
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .. import _lib
from .base import HipViTFeatureExtractor, NativeEncoder
from .checkpoints import (IMAGENET_MEAN, IMAGENET_STD, OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, _env_seed,  # noqa: F401 (re-exported)
                          check_canonical, load_checkpoint, resolve_weights, weights_path)

# Leading Resize of the reference transform per registered name: (shorter side, Pillow filter).
# torchvision (models/patch/base.py:126-145 prefers <enum>.IMAGENET1K_V1, base.py:170 takes weights.transforms()) [3P]:
#   ViT_B_16_Weights.IMAGENET1K_V1 = ImageClassification(crop_size=224)                  -> resize_size 256 (default), bilinear
#   ViT_L_16_Weights.IMAGENET1K_V1 = ImageClassification(crop_size=224, resize_size=242) -> 256-px tiles ARE resampled to 242
# timm / open_clip: uni_v1 Resize(224, bicubic), conch_v1 Resize(448, bicubic).
#   ViT_B_32 / ViT_L_32 IMAGENET1K_V1 = ImageClassification(crop_size=224)               -> resize 256, bilinear
#   ViT_H_14 has no IMAGENET1K_V1: base.py:131-137 falls back to DEFAULT = IMAGENET1K_SWAG_E2E_V1 =
#     ImageClassification(crop_size=518, resize_size=518, interpolation=BICUBIC), model image_size 518 (1370 tokens)
# uni_v2 (uni.py:62-125): timm create_transform of the hub config = Resize(224, bicubic) + CenterCrop(224) (unverifiable offline)
TRANSFORM_RESIZE = {
    "vit_b_16": (256, "bilinear"),
    "vit_b_32": (256, "bilinear"),
    "vit_l_16": (242, "bilinear"),
    "vit_l_32": (256, "bilinear"),
    "vit_h_14": (518, "bicubic"),
    "uni_v1": (224, "bicubic"),
    "uni_v2": (224, "bicubic"),
    "conch_v1": (448, "bicubic"),
    # transformers image processors (dinov2.py:20-25, phikon.py:16-21: AutoImageProcessor(use_fast=True), configs from the public
    # model cards, unverifiable offline): facebook/dinov2-* = BitImageProcessor(shortest_edge 256, bicubic, crop 224);
    # owkin/phikon = ViTImageProcessor(224 x 224, bilinear, no crop); owkin/phikon-v2 = BitImageProcessor(224, bicubic, crop 224).
    # Deviation, stated: the fast processors resample with torchvision's tensor kernels (antialias on), this path with the
    # Pillow-exact device resize; on the default 256-px tiles the dinov2 resize is a no-op.
    "dinov2_small": (256, "bicubic"), "dinov2_base": (256, "bicubic"), "dinov2_large": (256, "bicubic"),
    "dinov2_giant": (256, "bicubic"),
    "phikon_v1": (224, "bilinear"), "phikon_v2": (224, "bicubic"),
    # torchvision transforms written out in the loader files (PIL input -> Pillow filters):
    #   midnight.py:14-24 Resize(224) + CenterCrop(224), Normalize(0.5, 0.5); hoptimus.py:15-30 Resize((224, 224)) + its own
    #   mean / std; gigapath.py:15-26 Resize(256, BICUBIC) + CenterCrop(224); pathorchestra.py:52-58 Resize(224)
    "midnight": (224, "bilinear"), "h_optimus_0": (224, "bilinear"), "h_optimus_1": (224, "bilinear"),
    # virchow.py:14-19: timm create_transform of the hub config (expected: Resize(224, bicubic) + CenterCrop(224), ImageNet
    # mean / std; unverifiable offline)
    "virchow_v1": (224, "bicubic"), "virchow_v2": (224, "bicubic"), "h0_mini": (224, "bicubic"),
    "prov_gigapath": (256, "bicubic"), "pathorchestra": (224, "bilinear"),
    # lunit.py:58-59: timm create_transform of the hub data config (expected: Resize(256, bicubic) + CenterCrop(224), the
    # checkpoints' own mean / std; unverifiable offline)
    "lunit_vit_small_patch16_dino": (256, "bicubic"), "lunit_vit_small_patch8_dino": (256, "bicubic"),
    # open_clip image transform (clip.py:38-40) / transformers CLIPProcessor (plip.py:35, quilt.py): Resize(S, bicubic) +
    # CenterCrop(S), OpenAI CLIP mean / std
    "clip_vit_b_32": (224, "bicubic"), "clip_vit_b_16": (224, "bicubic"), "clip_vit_l_14": (224, "bicubic"),
    "clip_vit_l_14_336": (336, "bicubic"), "plip": (224, "bicubic"), "quilt_b_32": (224, "bicubic"), "quilt_b_16": (224, "bicubic"),
    "biomedclip": (224, "bicubic"),
    # dinov3.py:52 AutoImageProcessor of facebook/dinov3-*: 224 x 224, bilinear, no crop (public model cards, unverifiable offline)
    "dinov3_vits16": (224, "bilinear"), "dinov3_vits16_plus": (224, "bilinear"), "dinov3_vitb16": (224, "bilinear"),
    "dinov3_vitl16": (224, "bilinear"), "dinov3_vitl16_sat": (224, "bilinear"), "dinov3_vith16_plus": (224, "bilinear"),
    "dinov3_vit7b16": (224, "bilinear"), "dinov3_vit7b16_sat": (224, "bilinear"),
    # medsiglip.py:38 AutoProcessor(use_fast=True) of google/medsiglip-448 = SiglipImageProcessor: resize to 448 x 448 (both sides,
    # no crop), `resample: 2` = bilinear, rescale 1 / 255, mean = std = 0.5 (public model card, unverifiable offline)
    "medsiglip": (448, "bilinear"),
    # open_clip image transforms (omiclip.py:59-61: create_model_and_transforms of coca_ViT-L-14; conch.py:97-100: CONCH v1.5's own
    # 448-px transform; the packages are absent offline, unverified): Resize(S, bicubic) + CenterCrop(S)
    "omiclip": (224, "bicubic"), "conch_v15": (448, "bicubic"),
}

# Normalize() constants per registered name (default: ImageNet)
TRANSFORM_NORM = {
    "conch_v1": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD),
    "clip_vit_b_32": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD), "clip_vit_b_16": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD),
    "clip_vit_l_14": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD), "clip_vit_l_14_336": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD),
    "plip": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD), "quilt_b_32": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD),
    "quilt_b_16": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD), "biomedclip": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD),
    "dinov3_vitl16_sat": ((0.430, 0.411, 0.296), (0.213, 0.156, 0.143)),        # the satellite (SAT-493M) checkpoints' statistics
    "dinov3_vit7b16_sat": ((0.430, 0.411, 0.296), (0.213, 0.156, 0.143)),       # (their AutoImageProcessor config, dinov3.py:39-41)
    "midnight": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),                                                   # midnight.py:22
    "medsiglip": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),                          # the processor config's image_mean / image_std
    "h_optimus_0": ((0.707223, 0.578729, 0.703617), (0.211883, 0.230117, 0.177517)),                  # hoptimus.py:24-27
    "h_optimus_1": ((0.707223, 0.578729, 0.703617), (0.211883, 0.230117, 0.177517)),
    "h0_mini": ((0.707223, 0.578729, 0.703617), (0.211883, 0.230117, 0.177517)),          # the hub config's (H-optimus statistics)
    "lunit_vit_small_patch16_dino": ((0.70322989, 0.53606487, 0.66096631), (0.21716536, 0.26081574, 0.20723464)),
    "lunit_vit_small_patch8_dino": ((0.70322989, 0.53606487, 0.66096631), (0.21716536, 0.26081574, 0.20723464)),
    "omiclip": (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD),            # open_clip's default constants (unverified offline)
    "conch_v15": (IMAGENET_MEAN, IMAGENET_STD),                # CONCH v1.5's transform (unverified offline)
}

ARCHS = {
    # name: image, patch, dim, depth, heads, mlp, eps, layer_scale
    "vit_b_16": dict(image_size=224, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072,
                     ln_eps=1e-6, layer_scale=False),
    "vit_l_16": dict(image_size=224, patch_size=16, dim=1024, depth=24, heads=16, mlp_dim=4096,
                     ln_eps=1e-6, layer_scale=False),
    "uni_v1": dict(image_size=224, patch_size=16, dim=1024, depth=24, heads=16, mlp_dim=4096,
                   ln_eps=1e-6, layer_scale=True),
    # the rest of models/patch/vit.py:9-15 (torchvision): patch 32 (50 tokens); ViT-H/14 at the SWAG end-to-end weights'
    # 518 px (37 x 37 + 1 = 1370 tokens), heads 80 wide (stored zero-padded to 96 on the device, softmax scale 1/sqrt(80))
    "vit_b_32": dict(image_size=224, patch_size=32, dim=768, depth=12, heads=12, mlp_dim=3072,
                     ln_eps=1e-6, layer_scale=False),
    "vit_l_32": dict(image_size=224, patch_size=32, dim=1024, depth=24, heads=16, mlp_dim=4096,
                     ln_eps=1e-6, layer_scale=False),
    "vit_h_14": dict(image_size=518, patch_size=14, dim=1280, depth=32, heads=16, mlp_dim=5120,
                     ln_eps=1e-6, layer_scale=False),
    # UNI2-h (models/patch/uni.py:62-125, timm kwargs :82-96): ViT-H/14 at 224 px, 8 register tokens, no_embed_class (the
    # position embedding covers the 256 patch tokens only), SwiGLUPacked MLP (fc1 1536 -> 2 x 4096, silu(x1) * x2, fc2
    # 4096 -> 1536; mlp_ratio 2.66667 * 2 -> int(1536 * 5.33334) = 8192 packed), LayerScale 1e-5, class-token pooling
    "uni_v2": dict(image_size=224, patch_size=14, dim=1536, depth=24, heads=24, mlp_dim=4096,
                   ln_eps=1e-6, layer_scale=True, reg_tokens=8, no_embed_class=True, mlp="swiglu"),
    # CONCH v1 visual tower (models/patch/conch.py:20-64 -> conch.open_clip_custom "conch_ViT-B-16" [3P, package
    # absent offline]): timm ViT-B/16 trunk at 448 px (785 tokens) + open_clip AttentionalPooler with ONE
    # contrastive query (d_model 512, 8 heads, context 768) + LayerNorm; encode_image(proj_contrast=False,
    # normalize=False) returns that 512-vector.
    "conch_v1": dict(image_size=448, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072,
                     ln_eps=1e-6, layer_scale=False, pool="attn", pool_dim=512, pool_heads=8, pool_ln_eps=1e-5),
    # transformers Dinov2Model (models/patch/dinov2.py:12-17,46-60: AutoModel.from_pretrained(facebook/dinov2-*),
    # last_hidden_state[:, 0]): patch 14 at the processor's 224-px crop = 256 + 1 tokens, LayerScale, LayerNorm 1e-6; the
    # checkpoints hold a 37 x 37 position grid (518 px) that the model resamples to the input's 16 x 16 with torch's bicubic
    # interpolate in every forward (Dinov2Embeddings.interpolate_pos_encoding) -- done once at load here, with the same call.
    # Canonical form: no_embed_class with the class position row folded into the class token (the hf_dinov2 adapter).
    # giant: SwiGLUFFN, hidden = (int(1536 * 4 * 2 / 3) + 7) // 8 * 8 = 4096, silu(x1) * x2 on the two halves of weights_in
    "dinov2_small": dict(image_size=224, patch_size=14, dim=384, depth=12, heads=6, mlp_dim=1536, ln_eps=1e-6,
                         layer_scale=True, no_embed_class=True),
    "dinov2_base": dict(image_size=224, patch_size=14, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-6,
                        layer_scale=True, no_embed_class=True),
    "dinov2_large": dict(image_size=224, patch_size=14, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-6,
                         layer_scale=True, no_embed_class=True),
    "dinov2_giant": dict(image_size=224, patch_size=14, dim=1536, depth=40, heads=24, mlp_dim=4096, ln_eps=1e-6,
                         layer_scale=True, no_embed_class=True, mlp="swiglu"),
    # models/patch/phikon.py: phikon_v1 = transformers ViTModel(owkin/phikon, add_pooling_layer=False) = ViT-B/16, LayerNorm
    # 1e-12 (ViTConfig default), last_hidden_state[:, 0] (after the final LayerNorm); phikon_v2 = AutoModel(owkin/phikon-v2) =
    # Dinov2Model ViT-L/16 at 224 px (197 tokens)
    "phikon_v1": dict(image_size=224, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-12, layer_scale=False),
    "phikon_v2": dict(image_size=224, patch_size=16, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-6,
                      layer_scale=True, no_embed_class=True),
    # models/patch/midnight.py: transformers AutoModel(kaiko-ai/midnight) = Dinov2Model ViT-g/14 (the loader's emb_dim 3072 = 2 x
    # 1536), features = cat(last_hidden_state[:, 0], last_hidden_state[:, 1:].mean(1))
    "midnight": dict(image_size=224, patch_size=14, dim=1536, depth=40, heads=24, mlp_dim=4096, ln_eps=1e-6,
                     layer_scale=True, no_embed_class=True, mlp="swiglu", pool="cls_mean"),
    # timm hub models; the architecture comes from the hub's config.json, not from the reference's text (public model cards,
    # unverifiable offline -- same standing as uni_v1 / uni_v2).  hoptimus.py:53-58 (init_values 1e-5): H-optimus-0 / -1 =
    # vit_giant_patch14_reg4_dinov2 at 224 px (1536 / 40 / 24, SwiGLUPacked 4096, 4 register tokens, no_embed_class);
    # gigapath.py:46: vit_giant_patch14_dinov2 with patch 16 (1536 / 40 / 24, SwiGLUPacked 4096, class position row);
    # lunit.py:10-16: timm vit_small patch 16 / 8 (384 / 12 / 6); pathorchestra.py:38-43: ViT-L/16 with LayerScale
    "h_optimus_0": dict(image_size=224, patch_size=14, dim=1536, depth=40, heads=24, mlp_dim=4096, ln_eps=1e-6,
                        layer_scale=True, reg_tokens=4, no_embed_class=True, mlp="swiglu"),
    "h_optimus_1": dict(image_size=224, patch_size=14, dim=1536, depth=40, heads=24, mlp_dim=4096, ln_eps=1e-6,
                        layer_scale=True, reg_tokens=4, no_embed_class=True, mlp="swiglu"),
    "prov_gigapath": dict(image_size=224, patch_size=16, dim=1536, depth=40, heads=24, mlp_dim=4096, ln_eps=1e-6,
                          layer_scale=True, mlp="swiglu"),
    # virchow.py:41-46,94-99 (mlp_layer=SwiGLUPacked, act_layer=SiLU; hub config: ViT-H/14, 1280 / 32 / 16 -> 80-wide heads,
    # mlp_ratio 5.3375 -> packed 6832 = 2 x 3416, init_values 1e-5; Virchow2: 4 register tokens).  Features: class token |
    # mean of the patch tokens (virchow.py:58-61; Virchow2 skips its registers, :111-114) = 2560-d
    # hoptimus.py:141-146,158-161: H0-mini = vit_base_patch14_reg4_dinov2 with SwiGLUPacked (768 / 12 / 12, packed 3072 = 2 x
    # 1536, 4 register tokens, no_embed_class), features = class token | mean of the patch tokens (1536-d)
    "h0_mini": dict(image_size=224, patch_size=14, dim=768, depth=12, heads=12, mlp_dim=1536, ln_eps=1e-6, layer_scale=True,
                    reg_tokens=4, no_embed_class=True, mlp="swiglu", pool="cls_mean"),
    "virchow_v1": dict(image_size=224, patch_size=14, dim=1280, depth=32, heads=16, mlp_dim=3416, ln_eps=1e-6, layer_scale=True,
                       mlp="swiglu", pool="cls_mean"),
    "virchow_v2": dict(image_size=224, patch_size=14, dim=1280, depth=32, heads=16, mlp_dim=3416, ln_eps=1e-6, layer_scale=True,
                       mlp="swiglu", pool="cls_mean", reg_tokens=4),
    "lunit_vit_small_patch16_dino": dict(image_size=224, patch_size=16, dim=384, depth=12, heads=6, mlp_dim=1536, ln_eps=1e-6,
                                         layer_scale=False),
    "lunit_vit_small_patch8_dino": dict(image_size=224, patch_size=8, dim=384, depth=12, heads=6, mlp_dim=1536, ln_eps=1e-6,
                                        layer_scale=False),
    "pathorchestra": dict(image_size=224, patch_size=16, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-6,
                          layer_scale=True),
    # CLIP vision towers: models/patch/clip.py:16-19 (open_clip ViT-B-32 / ViT-B-16 / ViT-L-14 / ViT-L-14-336, "openai"),
    # plip.py (transformers CLIPModel vinid/plip = ViT-B/32), quilt.py (CLIPModel wisdomik/QuiltNet-B-32 / B-16).  No
    # patch-embedding bias, LayerNorm on the embedded tokens before the blocks (ln_pre), QuickGELU, LayerNorm 1e-5, final
    # LayerNorm of the class token times the bias-free visual projection = encode_image / get_image_features
    "clip_vit_b_32": dict(image_size=224, patch_size=32, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-5, layer_scale=False,
                          pre_norm=True, act="quick_gelu", proj_dim=512),
    "clip_vit_b_16": dict(image_size=224, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-5, layer_scale=False,
                          pre_norm=True, act="quick_gelu", proj_dim=512),
    "clip_vit_l_14": dict(image_size=224, patch_size=14, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-5, layer_scale=False,
                          pre_norm=True, act="quick_gelu", proj_dim=768),
    "clip_vit_l_14_336": dict(image_size=336, patch_size=14, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-5,
                              layer_scale=False, pre_norm=True, act="quick_gelu", proj_dim=768),
    "plip": dict(image_size=224, patch_size=32, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-5, layer_scale=False,
                 pre_norm=True, act="quick_gelu", proj_dim=512),
    "quilt_b_32": dict(image_size=224, patch_size=32, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-5, layer_scale=False,
                       pre_norm=True, act="quick_gelu", proj_dim=512),
    "quilt_b_16": dict(image_size=224, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-5, layer_scale=False,
                       pre_norm=True, act="quick_gelu", proj_dim=512),
    # biomedclip.py: open_clip TimmModel = timm vit_base_patch16_224 (erf GELU, LayerNorm 1e-6, class token) + linear projection
    # 768 -> 512 without bias; encode_image (not normalised)
    "biomedclip": dict(image_size=224, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-6, layer_scale=False,
                       proj_dim=512),
    # models/patch/dinov3.py:12-21: transformers DINOv3ViTModel, pooler_output.  Class + 4 register tokens, no position embedding,
    # rotary embedding (theta 100) on q / k of the patch tokens, LayerScale, LayerNorm 1e-5; "plus" = gated MLP.  The two
    # dinov3_vit7b16 names (dinov3.py:20-21): dim 4096, 40 blocks, 32 heads of 128, gated MLP 8192 (6.7 G parameters, 13.4 GB in
    # float16; public hub config, unverifiable offline) -- the rows wider than 2048 take the LayerNorm kernels' 16-vector form.
    "dinov3_vits16": dict(image_size=224, patch_size=16, dim=384, depth=12, heads=6, mlp_dim=1536, ln_eps=1e-5, layer_scale=True,
                          reg_tokens=4, no_embed_class=True, rope=True),
    "dinov3_vits16_plus": dict(image_size=224, patch_size=16, dim=384, depth=12, heads=6, mlp_dim=1536, ln_eps=1e-5, layer_scale=True,
                               reg_tokens=4, no_embed_class=True, rope=True, mlp="swiglu"),
    "dinov3_vitb16": dict(image_size=224, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-5, layer_scale=True,
                          reg_tokens=4, no_embed_class=True, rope=True),
    "dinov3_vitl16": dict(image_size=224, patch_size=16, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-5, layer_scale=True,
                          reg_tokens=4, no_embed_class=True, rope=True),
    "dinov3_vitl16_sat": dict(image_size=224, patch_size=16, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-5, layer_scale=True,
                              reg_tokens=4, no_embed_class=True, rope=True),
    "dinov3_vith16_plus": dict(image_size=224, patch_size=16, dim=1280, depth=32, heads=20, mlp_dim=5120, ln_eps=1e-5, layer_scale=True,
                               reg_tokens=4, no_embed_class=True, rope=True, mlp="swiglu"),
    "dinov3_vit7b16": dict(image_size=224, patch_size=16, dim=4096, depth=40, heads=32, mlp_dim=8192, ln_eps=1e-5, layer_scale=True,
                           reg_tokens=4, no_embed_class=True, rope=True, mlp="swiglu"),
    "dinov3_vit7b16_sat": dict(image_size=224, patch_size=16, dim=4096, depth=40, heads=32, mlp_dim=8192, ln_eps=1e-5, layer_scale=True,
                               reg_tokens=4, no_embed_class=True, rope=True, mlp="swiglu"),
    # models/patch/medsiglip.py: transformers SiglipVisionModel of google/medsiglip-448 (SigLIP so400m/14 at 448 px; public hub
    # config, unverifiable offline), get_image_features = pooler_output.  No class token (1024 patch tokens with a learned position
    # row each), tanh GELU, LayerNorm 1e-6, and the attention-pooling head (a learned probe attends over the tokens of the final
    # LayerNorm, then LayerNorm + MLP with a residual).  Heads 72 wide, stored zero-padded to 96; MLP 4304, stored as 4352.
    "medsiglip": dict(image_size=448, patch_size=14, dim=1152, depth=27, heads=16, mlp_dim=4304, ln_eps=1e-6, layer_scale=False,
                      act="gelu_tanh", pool="map", no_class_token=True),
    # The two ViT-L towers behind a 96-wide attentional pooler (open_clip AttentionalPooler(d_model 768, context 1024, 8 heads)).
    # The reference only calls open_clip and the TITAN repository's conch_v1_5.py: both architectures are restated here from the
    # public packages [3P], UNVERIFIED OFFLINE, and parity is claimed against the restatement in tests/coca_reference.py only.
    # omiclip (models/patch/omiclip.py:14,46,59-61): open_clip "coca_ViT-L-14" visual tower, CoCa.encode_image(x).  ViT-L/14 at 224
    # px (257 tokens), no patch-embedding bias, ln_pre, erf GELU, LayerNorm 1e-5, NO LayerNorm after the last block; the pooler has
    # 256 queries of which row 0 is the pooled vector (rows 1 .. 255 are the caption tokens), then ln_post, `proj` [768, 768]
    # without bias and L2 normalisation (normalize=True, encode_image's default).
    "omiclip": dict(image_size=224, patch_size=14, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-5, layer_scale=False,
                    pre_norm=True, pool="attn", pool_dim=768, pool_heads=8, pool_ln_eps=1e-5, pool_head_dim=96,
                    pool_skip_final_norm=True, pool_proj_dim=768, out_normalize=True),
    # conch_v15 (models/patch/conch.py:82-85,97-100): build_conch(ConchConfig()) of the TITAN repository, model(x).  timm ViT-L/16
    # trunk at 448 px (785 tokens) with LayerScale, LayerNorm 1e-6, the trunk's final norm on all tokens, a ONE-query pooler
    # (attn_pool_contrast) and ln_contrast; no projection, not normalised: 768 floats.
    "conch_v15": dict(image_size=448, patch_size=16, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-6, layer_scale=True,
                      pool="attn", pool_dim=768, pool_heads=8, pool_ln_eps=1e-5, pool_head_dim=96),
}


# ----------------------------------------------------------------------------- adapters
def _detect_source(sd: dict) -> str:
    keys = sd.keys()
    if "conv_proj.weight" in keys:
        return "torchvision"
    if "visual.trunk.patch_embed.proj.weight" in keys and "visual.head.proj.weight" in keys:
        return "open_clip_timm"
    if "patch_embed.proj.weight" in keys:
        return "timm"
    if "vision_model.pre_layrnorm.weight" in keys or "pre_layrnorm.weight" in keys:
        return "hf_clip"
    if ("vision_model.head.probe" in keys or "head.probe" in keys) and \
            ("vision_model.embeddings.patch_embedding.weight" in keys or "embeddings.patch_embedding.weight" in keys):
        return "hf_siglip"
    if "visual.ln_pre.weight" in keys or "ln_pre.weight" in keys:
        return "open_clip"
    # DINOv3ViTModel: `model.layer.<i>.` in memory (transformers 5), `layer.<i>.` in the published model.safetensors
    # (transformers renames on load: conversion_mapping `(?<!model\.)layer.` -> `model.layer.`); accept both
    if any(re.match(r"(model\.)?layer\.\d+\.attention\.q_proj\.weight$", k) for k in keys) and "embeddings.cls_token" in keys:
        return "hf_dinov3"
    if "embeddings.register_tokens" in keys or any(".layer_scale1.lambda1" in k for k in keys):
        return "hf_dinov2"
    if any(k.startswith("embeddings.patch_embeddings") for k in keys):
        return "hf"
    if "patch_embed.weight" in keys:
        return "canonical"
    raise ValueError("unrecognised ViT state dict (expected torchvision, timm, HF ViTModel or canonical keys)")


def resample_position_grid(pos: torch.Tensor, grid: int) -> torch.Tensor:
    """Patch position rows [g0 * g0, D] -> [grid * grid, D] exactly as transformers' ``interpolate_pos_encoding`` does it
    (Dinov2Embeddings: float32, ``F.interpolate(mode="bicubic", align_corners=False)`` on the [1, D, g0, g0] view)."""
    g0 = int(round(pos.shape[0] ** 0.5))
    if g0 * g0 != pos.shape[0]:
        raise ValueError(f"position embedding with {pos.shape[0]} patch rows is not a square grid")
    if g0 == grid:
        return pos
    x = pos.detach().to(torch.float32).reshape(1, g0, g0, -1).permute(0, 3, 1, 2)
    y = torch.nn.functional.interpolate(x, size=(grid, grid), mode="bicubic", align_corners=False)
    return y.permute(0, 2, 3, 1).reshape(grid * grid, -1).contiguous()


def dinov3_rope_tables(grid: int, head_dim: int, theta: float = 100.0) -> tuple[torch.Tensor, torch.Tensor]:
    """cos / sin [grid * grid, head_dim] of transformers' DINOv3ViTRopePositionEmbedding in eval mode (float32, as the module forces):
    patch centres (i + 0.5) / grid mapped to [-1, 1], angles = 2 pi * coord * inv_freq with inv_freq = theta ** -arange(0, 1,
    4 / head_dim), (y | x) blocks flattened to head_dim / 2 and tiled twice."""
    import math
    c = torch.arange(0.5, grid, dtype=torch.float32) / grid
    coords = torch.stack(torch.meshgrid(c, c, indexing="ij"), dim=-1).flatten(0, 1)
    coords = 2.0 * coords - 1.0
    inv_freq = 1 / theta ** torch.arange(0, 1, 4 / head_dim, dtype=torch.float32)
    angles = 2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]
    angles = angles.flatten(1, 2).tile(2)
    return torch.cos(angles).contiguous(), torch.sin(angles).contiguous()


def canonical_state_dict(sd: dict, *, depth: int, layer_scale: bool, source: str = "auto", grid: Optional[int] = None,
                         heads: Optional[int] = None, rope_theta: float = 100.0) -> dict:
    """Return ``{canonical name: float32 CPU tensor}`` for ``ap_vit_set_param``.  ``grid``: patches per side of the input the
    encoder will see; an HF DINOv2 checkpoint trained on another grid has its position rows resampled to it (as the model
    itself does in every forward)."""
    sd = {k: v for k, v in sd.items()}
    if source == "auto":
        source = _detect_source(sd)
    out: dict[str, torch.Tensor] = {}

    def put(name, tensor):
        out[name] = tensor.detach().to(dtype=torch.float32, device="cpu").contiguous()

    if source == "canonical":
        for k, v in sd.items():
            put(k, v)
    elif source == "torchvision":
        put("patch_embed.weight", sd["conv_proj.weight"]); put("patch_embed.bias", sd["conv_proj.bias"])
        put("cls_token", sd["class_token"].reshape(-1)); put("pos_embed", sd["encoder.pos_embedding"][0])
        put("norm.weight", sd["encoder.ln.weight"]); put("norm.bias", sd["encoder.ln.bias"])
        for i in range(depth):
            p, b = f"encoder.layers.encoder_layer_{i}.", f"blocks.{i}."
            put(b + "ln1.weight", sd[p + "ln_1.weight"]); put(b + "ln1.bias", sd[p + "ln_1.bias"])
            put(b + "qkv.weight", sd[p + "self_attention.in_proj_weight"])
            put(b + "qkv.bias", sd[p + "self_attention.in_proj_bias"])
            put(b + "proj.weight", sd[p + "self_attention.out_proj.weight"])
            put(b + "proj.bias", sd[p + "self_attention.out_proj.bias"])
            put(b + "ln2.weight", sd[p + "ln_2.weight"]); put(b + "ln2.bias", sd[p + "ln_2.bias"])
            f1 = "mlp.0" if p + "mlp.0.weight" in sd else "mlp.linear_1"
            f2 = "mlp.3" if p + "mlp.3.weight" in sd else "mlp.linear_2"
            put(b + "fc1.weight", sd[p + f1 + ".weight"]); put(b + "fc1.bias", sd[p + f1 + ".bias"])
            put(b + "fc2.weight", sd[p + f2 + ".weight"]); put(b + "fc2.bias", sd[p + f2 + ".bias"])
    elif source == "open_clip_timm":
        # open_clip TimmModel (biomedclip.py:40: hf-hub:microsoft/BiomedCLIP-...-vit_base_patch16_224): visual.trunk = a timm ViT
        # (class-token pooling), visual.head.proj = the bias-free linear projection [embed_dim, width] [3P, unverified offline]
        trunk = {k[len("visual.trunk."):]: v for k, v in sd.items() if k.startswith("visual.trunk.")}
        out.update(canonical_state_dict(trunk, depth=depth, layer_scale=layer_scale, source="timm", grid=grid))
        put("head_proj.weight", sd["visual.head.proj.weight"])
    elif source == "timm":
        put("patch_embed.weight", sd["patch_embed.proj.weight"]); put("patch_embed.bias", sd["patch_embed.proj.bias"])
        put("cls_token", sd["cls_token"].reshape(-1)); put("pos_embed", sd["pos_embed"][0])
        if "reg_token" in sd:                                         # timm reg_tokens > 0: [1, R, D]
            put("reg_tokens", sd["reg_token"][0])
        put("norm.weight", sd["norm.weight"]); put("norm.bias", sd["norm.bias"])
        for i in range(depth):
            p, b = f"blocks.{i}.", f"blocks.{i}."
            put(b + "ln1.weight", sd[p + "norm1.weight"]); put(b + "ln1.bias", sd[p + "norm1.bias"])
            put(b + "qkv.weight", sd[p + "attn.qkv.weight"]); put(b + "qkv.bias", sd[p + "attn.qkv.bias"])
            put(b + "proj.weight", sd[p + "attn.proj.weight"]); put(b + "proj.bias", sd[p + "attn.proj.bias"])
            put(b + "ln2.weight", sd[p + "norm2.weight"]); put(b + "ln2.bias", sd[p + "norm2.bias"])
            put(b + "fc1.weight", sd[p + "mlp.fc1.weight"]); put(b + "fc1.bias", sd[p + "mlp.fc1.bias"])
            put(b + "fc2.weight", sd[p + "mlp.fc2.weight"]); put(b + "fc2.bias", sd[p + "mlp.fc2.bias"])
            if layer_scale:
                put(b + "ls1", sd[p + "ls1.gamma"]); put(b + "ls2", sd[p + "ls2.gamma"])
    elif source == "hf":
        put("patch_embed.weight", sd["embeddings.patch_embeddings.projection.weight"])
        put("patch_embed.bias", sd["embeddings.patch_embeddings.projection.bias"])
        put("cls_token", sd["embeddings.cls_token"].reshape(-1))
        put("pos_embed", sd["embeddings.position_embeddings"][0])
        put("norm.weight", sd["layernorm.weight"]); put("norm.bias", sd["layernorm.bias"])
        for i in range(depth):
            b = f"blocks.{i}."
            if f"layers.{i}.layernorm_before.weight" in sd:          # transformers >= 5
                p = f"layers.{i}."
                q, k, v, o = (p + "attention." + n for n in ("q_proj", "k_proj", "v_proj", "o_proj"))
                f1, f2 = p + "mlp.fc1", p + "mlp.fc2"
            else:                                                    # transformers 4.x
                p = f"encoder.layer.{i}."
                q, k, v = (p + "attention.attention." + n for n in ("query", "key", "value"))
                o, f1, f2 = p + "attention.output.dense", p + "intermediate.dense", p + "output.dense"
            put(b + "ln1.weight", sd[p + "layernorm_before.weight"]); put(b + "ln1.bias", sd[p + "layernorm_before.bias"])
            put(b + "qkv.weight", torch.cat([sd[q + ".weight"], sd[k + ".weight"], sd[v + ".weight"]], 0))
            put(b + "qkv.bias", torch.cat([sd[q + ".bias"], sd[k + ".bias"], sd[v + ".bias"]], 0))
            put(b + "proj.weight", sd[o + ".weight"]); put(b + "proj.bias", sd[o + ".bias"])
            put(b + "ln2.weight", sd[p + "layernorm_after.weight"]); put(b + "ln2.bias", sd[p + "layernorm_after.bias"])
            put(b + "fc1.weight", sd[f1 + ".weight"]); put(b + "fc1.bias", sd[f1 + ".bias"])
            put(b + "fc2.weight", sd[f2 + ".weight"]); put(b + "fc2.bias", sd[f2 + ".bias"])
    elif source == "hf_clip":
        # transformers CLIPModel / CLIPVisionModelWithProjection (plip.py:34, quilt.py: CLIPModel.from_pretrained): the vision
        # tower + visual_projection.  No patch-embedding bias; class_embedding + position_embedding rows; pre_layrnorm (sic)
        v = "vision_model." if "vision_model.pre_layrnorm.weight" in sd else ""
        d = sd[v + "embeddings.class_embedding"].shape[0]
        put("patch_embed.weight", sd[v + "embeddings.patch_embedding.weight"]); put("patch_embed.bias", torch.zeros(d))
        put("cls_token", sd[v + "embeddings.class_embedding"].reshape(-1))
        put("pos_embed", sd[v + "embeddings.position_embedding.weight"])
        put("pre_norm.weight", sd[v + "pre_layrnorm.weight"]); put("pre_norm.bias", sd[v + "pre_layrnorm.bias"])
        put("norm.weight", sd[v + "post_layernorm.weight"]); put("norm.bias", sd[v + "post_layernorm.bias"])
        if "visual_projection.weight" in sd:
            put("head_proj.weight", sd["visual_projection.weight"])
        for i in range(depth):
            p, b = f"{v}encoder.layers.{i}.", f"blocks.{i}."
            a = p + "self_attn."
            put(b + "ln1.weight", sd[p + "layer_norm1.weight"]); put(b + "ln1.bias", sd[p + "layer_norm1.bias"])
            put(b + "qkv.weight", torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]], 0))
            put(b + "qkv.bias", torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"], sd[a + "v_proj.bias"]], 0))
            put(b + "proj.weight", sd[a + "out_proj.weight"]); put(b + "proj.bias", sd[a + "out_proj.bias"])
            put(b + "ln2.weight", sd[p + "layer_norm2.weight"]); put(b + "ln2.bias", sd[p + "layer_norm2.bias"])
            put(b + "fc1.weight", sd[p + "mlp.fc1.weight"]); put(b + "fc1.bias", sd[p + "mlp.fc1.bias"])
            put(b + "fc2.weight", sd[p + "mlp.fc2.weight"]); put(b + "fc2.bias", sd[p + "mlp.fc2.bias"])
    elif source == "open_clip":
        # open_clip VisionTransformer (clip.py:38-40, the OpenAI checkpoints; key names of the public package [3P], unverified
        # offline): visual.conv1 (no bias), class_embedding, positional_embedding, ln_pre, transformer.resblocks.<i>.{ln_1,
        # attn.in_proj_weight | in_proj_bias | out_proj, ln_2, mlp.c_fc, mlp.c_proj}, ln_post, proj [width, output_dim]
        v = "visual." if "visual.ln_pre.weight" in sd else ""
        d = sd[v + "class_embedding"].shape[0]
        put("patch_embed.weight", sd[v + "conv1.weight"]); put("patch_embed.bias", torch.zeros(d))
        put("cls_token", sd[v + "class_embedding"].reshape(-1)); put("pos_embed", sd[v + "positional_embedding"])
        put("pre_norm.weight", sd[v + "ln_pre.weight"]); put("pre_norm.bias", sd[v + "ln_pre.bias"])
        put("norm.weight", sd[v + "ln_post.weight"]); put("norm.bias", sd[v + "ln_post.bias"])
        if v + "proj" in sd:
            put("head_proj.weight", sd[v + "proj"].t())
        for i in range(depth):
            p, b = f"{v}transformer.resblocks.{i}.", f"blocks.{i}."
            put(b + "ln1.weight", sd[p + "ln_1.weight"]); put(b + "ln1.bias", sd[p + "ln_1.bias"])
            put(b + "qkv.weight", sd[p + "attn.in_proj_weight"]); put(b + "qkv.bias", sd[p + "attn.in_proj_bias"])
            put(b + "proj.weight", sd[p + "attn.out_proj.weight"]); put(b + "proj.bias", sd[p + "attn.out_proj.bias"])
            put(b + "ln2.weight", sd[p + "ln_2.weight"]); put(b + "ln2.bias", sd[p + "ln_2.bias"])
            put(b + "fc1.weight", sd[p + "mlp.c_fc.weight"]); put(b + "fc1.bias", sd[p + "mlp.c_fc.bias"])
            put(b + "fc2.weight", sd[p + "mlp.c_proj.weight"]); put(b + "fc2.bias", sd[p + "mlp.c_proj.bias"])
    elif source == "hf_dinov3":
        # transformers DINOv3ViTModel (dinov3.py:52-67): class + register tokens, NO position embedding (zeros here; the rotary
        # tables rope.cos | rope.sin carry the positions), k_proj without bias, LayerScale, plain or gated (silu(gate) * up = the
        # packed SwiGLU layout [gate; up]) MLP, LayerNorm 1e-5, pooler_output = final LayerNorm of the class token
        if grid is None or heads is None:
            raise ValueError("hf_dinov3: the patch grid and the head count are needed for the rotary tables")
        d = sd["embeddings.cls_token"].shape[-1]
        put("patch_embed.weight", sd["embeddings.patch_embeddings.weight"]); put("patch_embed.bias", sd["embeddings.patch_embeddings.bias"])
        put("cls_token", sd["embeddings.cls_token"].reshape(-1))
        if sd["embeddings.register_tokens"].shape[1] > 0:
            put("reg_tokens", sd["embeddings.register_tokens"][0])
        put("pos_embed", torch.zeros(int(grid) * int(grid), d))
        put("norm.weight", sd["norm.weight"]); put("norm.bias", sd["norm.bias"])
        cos, sin = dinov3_rope_tables(int(grid), d // int(heads), rope_theta)
        put("rope.cos", cos); put("rope.sin", sin)
        root = "model.layer." if any(k.startswith("model.layer.") for k in sd) else "layer."      # in-memory / on-disk names
        for i in range(depth):
            p, b = f"{root}{i}.", f"blocks.{i}."
            a = p + "attention."
            zeros = torch.zeros(d)
            bias = lambda n: sd[a + n + ".bias"] if a + n + ".bias" in sd else zeros
            put(b + "ln1.weight", sd[p + "norm1.weight"]); put(b + "ln1.bias", sd[p + "norm1.bias"])
            put(b + "qkv.weight", torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]], 0))
            put(b + "qkv.bias", torch.cat([bias("q_proj"), bias("k_proj"), bias("v_proj")], 0))
            put(b + "proj.weight", sd[a + "o_proj.weight"]); put(b + "proj.bias", sd[a + "o_proj.bias"])
            put(b + "ln2.weight", sd[p + "norm2.weight"]); put(b + "ln2.bias", sd[p + "norm2.bias"])
            if p + "mlp.gate_proj.weight" in sd:
                put(b + "fc1.weight", torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], 0))
                put(b + "fc1.bias", torch.cat([sd[p + "mlp.gate_proj.bias"], sd[p + "mlp.up_proj.bias"]], 0))
            else:
                put(b + "fc1.weight", sd[p + "mlp.up_proj.weight"]); put(b + "fc1.bias", sd[p + "mlp.up_proj.bias"])
            put(b + "fc2.weight", sd[p + "mlp.down_proj.weight"]); put(b + "fc2.bias", sd[p + "mlp.down_proj.bias"])
            if layer_scale:
                put(b + "ls1", sd[p + "layer_scale1.lambda1"]); put(b + "ls2", sd[p + "layer_scale2.lambda1"])
    elif source == "hf_dinov2":
        # transformers Dinov2Model / Dinov2WithRegistersModel: the position embedding has a class row and patch rows but none
        # for the register tokens, which are inserted AFTER it is added -> canonical no_embed_class form with the class row
        # folded into the class token (one f32 add, the same one the model performs)
        pos = sd["embeddings.position_embeddings"][0]
        put("patch_embed.weight", sd["embeddings.patch_embeddings.projection.weight"])
        put("patch_embed.bias", sd["embeddings.patch_embeddings.projection.bias"])
        put("cls_token", (sd["embeddings.cls_token"].reshape(-1).float() + pos[0].float()))
        if "embeddings.register_tokens" in sd:
            put("reg_tokens", sd["embeddings.register_tokens"][0])
        put("pos_embed", pos[1:] if grid is None else resample_position_grid(pos[1:], int(grid)))
        put("norm.weight", sd["layernorm.weight"]); put("norm.bias", sd["layernorm.bias"])
        for i in range(depth):
            p, b = f"encoder.layer.{i}.", f"blocks.{i}."
            a = p + "attention.attention."
            put(b + "ln1.weight", sd[p + "norm1.weight"]); put(b + "ln1.bias", sd[p + "norm1.bias"])
            put(b + "qkv.weight", torch.cat([sd[a + "query.weight"], sd[a + "key.weight"], sd[a + "value.weight"]], 0))
            put(b + "qkv.bias", torch.cat([sd[a + "query.bias"], sd[a + "key.bias"], sd[a + "value.bias"]], 0))
            put(b + "proj.weight", sd[p + "attention.output.dense.weight"]); put(b + "proj.bias", sd[p + "attention.output.dense.bias"])
            put(b + "ln2.weight", sd[p + "norm2.weight"]); put(b + "ln2.bias", sd[p + "norm2.bias"])
            f1, f2 = (("mlp.weights_in", "mlp.weights_out") if p + "mlp.weights_in.weight" in sd else ("mlp.fc1", "mlp.fc2"))
            put(b + "fc1.weight", sd[p + f1 + ".weight"]); put(b + "fc1.bias", sd[p + f1 + ".bias"])
            put(b + "fc2.weight", sd[p + f2 + ".weight"]); put(b + "fc2.bias", sd[p + f2 + ".bias"])
            if layer_scale:
                put(b + "ls1", sd[p + "layer_scale1.lambda1"]); put(b + "ls2", sd[p + "layer_scale2.lambda1"])
    elif source == "hf_siglip":
        raise ValueError("hf_siglip checkpoints go through siglip_canonical_state_dict (it needs the architecture for its checks)")
    else:
        raise ValueError(f"unknown state-dict source '{source}'")
    return out


def siglip_canonical_shapes(arch: dict) -> dict:
    """Canonical key -> shape of a SigLIP vision tower BEFORE head / MLP padding (``arch``: an ``ARCHS`` entry with ``pool="map"``)."""
    d, mlp, ps = arch["dim"], arch["mlp_dim"], arch["patch_size"]
    patches = (arch["image_size"] // ps) ** 2
    want = {"patch_embed.weight": (d, 3, ps, ps), "patch_embed.bias": (d,), "pos_embed": (patches, d),
            "norm.weight": (d,), "norm.bias": (d,),
            "map.q": (d,), "map.kv.weight": (2 * d, d), "map.kv.bias": (2 * d,), "map.out.weight": (d, d), "map.out.bias": (d,),
            "map.ln.weight": (d,), "map.ln.bias": (d,), "map.fc1.weight": (mlp, d), "map.fc1.bias": (mlp,),
            "map.fc2.weight": (d, mlp), "map.fc2.bias": (d,)}
    for i in range(arch["depth"]):
        b = f"blocks.{i}."
        want.update({b + "ln1.weight": (d,), b + "ln1.bias": (d,), b + "qkv.weight": (3 * d, d), b + "qkv.bias": (3 * d,),
                     b + "proj.weight": (d, d), b + "proj.bias": (d,), b + "ln2.weight": (d,), b + "ln2.bias": (d,),
                     b + "fc1.weight": (mlp, d), b + "fc1.bias": (mlp,), b + "fc2.weight": (d, mlp), b + "fc2.bias": (d,)})
    return want


def siglip_canonical_state_dict(sd: dict, arch: dict) -> dict:
    """transformers' SigLIP vision tower -> canonical names (unpadded; ``HipViT`` pads heads and MLP).  Takes the three layouts that
    occur: ``SiglipVisionModel.state_dict()`` of transformers 5 (bare keys), the same prefixed ``vision_model.`` (older versions
    and the published ``model.safetensors``), and a whole ``SiglipModel`` checkpoint, whose ``text_model.*``, ``logit_scale`` and
    ``logit_bias`` are dropped.  ``map.q`` = W_q probe + b_q, the query third of ``head.attention.in_proj`` applied to the probe
    (input independent; float64 on the host, as for CONCH's pooler).  Every other unknown key, missing key or wrong shape is a
    ``ValueError`` naming it (``check_canonical``)."""
    src = {k: v for k, v in sd.items() if not (k.startswith("text_model.") or k in ("logit_scale", "logit_bias"))}
    if any(k.startswith("vision_model.") for k in src):
        src = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in src.items()}
    d, depth = arch["dim"], arch["depth"]
    out: dict[str, torch.Tensor] = {}
    used = set()

    def take(key):
        used.add(key)
        return src.get(key)

    def put(name, tensor):
        if tensor is not None:
            out[name] = tensor.detach().to(dtype=torch.float32, device="cpu").contiguous()

    def cat(*keys):
        parts = [take(k) for k in keys]
        if any(p is None for p in parts):
            return None
        if any(p.shape[1:] != parts[0].shape[1:] for p in parts):
            raise ValueError(f"SigLIP checkpoint: {list(keys)} have shapes {[tuple(p.shape) for p in parts]}, which do not stack")
        return torch.cat(parts, 0)

    put("patch_embed.weight", take("embeddings.patch_embedding.weight")); put("patch_embed.bias", take("embeddings.patch_embedding.bias"))
    put("pos_embed", take("embeddings.position_embedding.weight"))
    put("norm.weight", take("post_layernorm.weight")); put("norm.bias", take("post_layernorm.bias"))
    for i in range(depth):
        p, b = f"encoder.layers.{i}.", f"blocks.{i}."
        a = p + "self_attn."
        put(b + "ln1.weight", take(p + "layer_norm1.weight")); put(b + "ln1.bias", take(p + "layer_norm1.bias"))
        put(b + "qkv.weight", cat(a + "q_proj.weight", a + "k_proj.weight", a + "v_proj.weight"))
        put(b + "qkv.bias", cat(a + "q_proj.bias", a + "k_proj.bias", a + "v_proj.bias"))
        put(b + "proj.weight", take(a + "out_proj.weight")); put(b + "proj.bias", take(a + "out_proj.bias"))
        put(b + "ln2.weight", take(p + "layer_norm2.weight")); put(b + "ln2.bias", take(p + "layer_norm2.bias"))
        put(b + "fc1.weight", take(p + "mlp.fc1.weight")); put(b + "fc1.bias", take(p + "mlp.fc1.bias"))
        put(b + "fc2.weight", take(p + "mlp.fc2.weight")); put(b + "fc2.bias", take(p + "mlp.fc2.bias"))
    probe, w_in, b_in = take("head.probe"), take("head.attention.in_proj_weight"), take("head.attention.in_proj_bias")
    if probe is not None and w_in is not None and b_in is not None and tuple(w_in.shape) == (3 * d, d) and \
            tuple(b_in.shape) == (3 * d,) and probe.numel() == d:
        f = lambda t: t.detach().to(torch.float64, copy=True).cpu()
        put("map.q", f(w_in)[:d] @ f(probe).reshape(d) + f(b_in)[:d])
        put("map.kv.weight", w_in[d:]); put("map.kv.bias", b_in[d:])
    elif w_in is not None and b_in is not None:
        put("map.kv.weight", w_in); put("map.kv.bias", b_in)          # wrong shapes: check_canonical names them
    put("map.out.weight", take("head.attention.out_proj.weight")); put("map.out.bias", take("head.attention.out_proj.bias"))
    put("map.ln.weight", take("head.layernorm.weight")); put("map.ln.bias", take("head.layernorm.bias"))
    put("map.fc1.weight", take("head.mlp.fc1.weight")); put("map.fc1.bias", take("head.mlp.fc1.bias"))
    put("map.fc2.weight", take("head.mlp.fc2.weight")); put("map.fc2.bias", take("head.mlp.fc2.bias"))
    unknown = sorted(k for k in src if k not in used)
    absent = sorted(k for k in used if k not in src)
    try:
        return check_canonical(out, siglip_canonical_shapes(arch), unknown, family="SigLIP", source="hf_siglip")
    except ValueError as exc:
        if unknown or not absent:
            raise
        raise ValueError(f"{exc}; the checkpoint lacks {absent[:5]}") from None


def stored_head_dim(dim: int, heads: int) -> int:
    """Width of one q / k / v head as the device stores it: 64, 96 or 128 (other true widths are zero-padded up; 96 -- the 80-wide
    heads of ViT-H/14 and Virchow -- exists in the float16 / bfloat16 attention kernels only, like 128)."""
    hd = dim // heads
    if hd <= 64:
        return 64
    if hd <= 96:
        return 96
    if hd <= 128:
        return 128
    raise ValueError(f"head width {hd} (dim {dim} / heads {heads}) exceeds 128")


def pad_heads(state: dict, *, dim: int, heads: int, depth: int) -> dict:
    """Canonical state dict -> the same model with every attention head zero-padded from dim / heads to
    ``stored_head_dim`` channels: qkv rows [3, heads, hd, :] -> [3, heads, hdp, :], proj columns likewise.  Zero q / k
    channels add nothing to q.k, zero v channels give zero outputs that meet zero proj columns: the function is unchanged
    as long as the softmax scale stays 1 / sqrt(hd) (``attn_scale``)."""
    hd, hdp = dim // heads, stored_head_dim(dim, heads)
    if hd == hdp:
        return state
    out = dict(state)
    for i in range(depth):
        b = f"blocks.{i}."
        w = state[b + "qkv.weight"].reshape(3, heads, hd, -1)
        wp = torch.zeros((3, heads, hdp, w.shape[-1]), dtype=w.dtype); wp[:, :, :hd] = w
        out[b + "qkv.weight"] = wp.reshape(3 * heads * hdp, -1).contiguous()
        bb = state[b + "qkv.bias"].reshape(3, heads, hd)
        bp = torch.zeros((3, heads, hdp), dtype=bb.dtype); bp[:, :, :hd] = bb
        out[b + "qkv.bias"] = bp.reshape(-1).contiguous()
        pw = state[b + "proj.weight"].reshape(-1, heads, hd)
        pp = torch.zeros((pw.shape[0], heads, hdp), dtype=pw.dtype); pp[:, :, :hd] = pw
        out[b + "proj.weight"] = pp.reshape(pw.shape[0], heads * hdp).contiguous()
    if "map.kv.weight" in state:                                     # SigLIP's pooling head: q [heads, hd], kv rows [2, heads, hd, :], out columns
        q = state["map.q"].reshape(heads, hd)
        qp = torch.zeros((heads, hdp), dtype=q.dtype); qp[:, :hd] = q
        out["map.q"] = qp.reshape(-1).contiguous()
        w = state["map.kv.weight"].reshape(2, heads, hd, -1)
        wp = torch.zeros((2, heads, hdp, w.shape[-1]), dtype=w.dtype); wp[:, :, :hd] = w
        out["map.kv.weight"] = wp.reshape(2 * heads * hdp, -1).contiguous()
        bb = state["map.kv.bias"].reshape(2, heads, hd)
        bp = torch.zeros((2, heads, hdp), dtype=bb.dtype); bp[:, :, :hd] = bb
        out["map.kv.bias"] = bp.reshape(-1).contiguous()
        pw = state["map.out.weight"].reshape(-1, heads, hd)
        pp = torch.zeros((pw.shape[0], heads, hdp), dtype=pw.dtype); pp[:, :, :hd] = pw
        out["map.out.weight"] = pp.reshape(pw.shape[0], heads * hdp).contiguous()
    return out


def stored_mlp_dim(mlp_dim: int) -> int:
    """Hidden width of the MLP as the device stores it: the next multiple of 128 (the GEMM kernels' N / K granularity)."""
    return (int(mlp_dim) + 127) // 128 * 128


def pad_mlp(state: dict, *, mlp_dim: int, depth: int, swiglu: bool) -> dict:
    """Canonical state dict -> the same model with the MLP's hidden width zero-padded to ``stored_mlp_dim`` (Virchow: timm
    ``mlp_ratio=5.3375`` on dim 1280 gives a packed width of 6832 = 2 x 3416, and 3416 is no multiple of 64).  Padded fc1 rows have
    zero weights and biases, so their activations are gelu(0) = 0 (or silu(0) * 0 = 0) and meet zero fc2 columns: the function
    is unchanged.  SwiGLU: the two halves x1 | x2 are padded separately."""
    hp = stored_mlp_dim(mlp_dim)
    if hp == mlp_dim:
        return state
    out = dict(state)
    prefixes = [f"blocks.{i}." for i in range(depth)] + (["map."] if "map.fc1.weight" in state else [])   # (gelu_tanh(0) = 0 too)
    for b in prefixes:
        w1, b1, w2 = state[b + "fc1.weight"], state[b + "fc1.bias"], state[b + "fc2.weight"]
        halves = 2 if swiglu else 1
        w1p = torch.zeros((halves, hp, w1.shape[1]), dtype=w1.dtype); w1p[:, :mlp_dim] = w1.reshape(halves, mlp_dim, -1)
        b1p = torch.zeros((halves, hp), dtype=b1.dtype); b1p[:, :mlp_dim] = b1.reshape(halves, mlp_dim)
        w2p = torch.zeros((w2.shape[0], hp), dtype=w2.dtype); w2p[:, :mlp_dim] = w2
        out[b + "fc1.weight"] = w1p.reshape(halves * hp, -1).contiguous()
        out[b + "fc1.bias"] = b1p.reshape(-1).contiguous()
        out[b + "fc2.weight"] = w2p.contiguous()
    return out


def attn_pool_canonical(pool: dict, *, pool_eps: float = 1e-5) -> dict:
    """open_clip ``AttentionalPooler`` (+ the LayerNorm after it) -> ``attn_pool.*`` parameters.

    ``pool`` holds the module's own tensors: ``query`` [Q, P], ``ln_q.weight|bias``, ``ln_k.weight|bias``,
    ``attn.q_proj_weight`` [P, P], ``attn.k_proj_weight`` / ``attn.v_proj_weight`` [P, C], ``attn.in_proj_bias``
    [3P], ``attn.out_proj.weight|bias`` and ``ln_out.weight|bias`` (CONCH: ``visual.ln_contrast``; CoCa: ``visual.ln_post``),
    and optionally ``proj`` [P, P2] (CoCa's projection, stored transposed as ``attn_pool.proj.weight``).
    The projected query is input independent and is folded here (float64 on the host).  Of Q queries only row 0 is the pooled
    vector (CoCa: rows 1 .. 255 are the caption tokens, which ``encode_image`` drops); the head width plays no part here."""
    f = lambda k: pool[k].detach().to(torch.float64, copy=True).cpu()
    P = pool["attn.q_proj_weight"].shape[0]
    q = torch.nn.functional.layer_norm(f("query").reshape(-1, P)[:1], (P,), f("ln_q.weight"), f("ln_q.bias"), pool_eps)
    q = q @ f("attn.q_proj_weight").T + f("attn.in_proj_bias")[:P]
    extra = {"attn_pool.proj.weight": f("proj").T} if "proj" in pool else {}
    out = {"attn_pool.q": q.reshape(-1), **extra,
           "attn_pool.ln_k.weight": f("ln_k.weight"), "attn_pool.ln_k.bias": f("ln_k.bias"),
           "attn_pool.kv.weight": torch.cat([f("attn.k_proj_weight"), f("attn.v_proj_weight")], 0),
           "attn_pool.kv.bias": f("attn.in_proj_bias")[P:],
           "attn_pool.out.weight": f("attn.out_proj.weight"), "attn_pool.out.bias": f("attn.out_proj.bias"),
           "attn_pool.ln_out.weight": f("ln_out.weight"), "attn_pool.ln_out.bias": f("ln_out.bias")}
    return {k: v.to(torch.float32).contiguous() for k, v in out.items()}


def conch_state_dicts(sd: dict) -> tuple[dict, dict]:
    """Split a CONCH v1 checkpoint (open_clip_custom CoCa; key names from the public package [3P], unverified
    offline) into the timm trunk state dict and the pooler tensors ``attn_pool_canonical`` expects.  The tower's keys
    (``trunk.*``, ``attn_pool_contrast.*``, ``ln_contrast.*``) may stand under ``visual.`` (CONCH v1), under ``vision_encoder.``
    or bare (CONCH v1.5)."""
    root = next((r for r in ("visual.", "vision_encoder.", "") if any(k.startswith(r + "trunk.") for k in sd)), "visual.")
    trunk = {k[len(root + "trunk."):]: v for k, v in sd.items() if k.startswith(root + "trunk.")}
    pre = root + "attn_pool_contrast."
    pool = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    pool["ln_out.weight"] = sd[root + "ln_contrast.weight"]
    pool["ln_out.bias"] = sd[root + "ln_contrast.bias"]
    return trunk, pool


POOLER_KEYS = ("query", "ln_q.weight", "ln_q.bias", "ln_k.weight", "ln_k.bias", "attn.q_proj_weight", "attn.k_proj_weight",
               "attn.v_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias")


def attn_tower_canonical_shapes(arch: dict) -> dict:
    """Canonical key -> shape of a class-token ViT with the attentional pooler (``arch``: an ``ARCHS`` entry with ``pool="attn"``)."""
    d, mlp, ps, P = arch["dim"], arch["mlp_dim"], arch["patch_size"], arch["pool_dim"]
    tokens = 1 + (arch["image_size"] // ps) ** 2
    want = {"patch_embed.weight": (d, 3, ps, ps), "patch_embed.bias": (d,), "cls_token": (d,), "pos_embed": (tokens, d),
            "attn_pool.q": (P,), "attn_pool.ln_k.weight": (d,), "attn_pool.ln_k.bias": (d,), "attn_pool.kv.weight": (2 * P, d),
            "attn_pool.kv.bias": (2 * P,), "attn_pool.out.weight": (P, P), "attn_pool.out.bias": (P,),
            "attn_pool.ln_out.weight": (P,), "attn_pool.ln_out.bias": (P,)}
    if not arch.get("pool_skip_final_norm"):
        want.update({"norm.weight": (d,), "norm.bias": (d,)})
    if arch.get("pre_norm"):
        want.update({"pre_norm.weight": (d,), "pre_norm.bias": (d,)})
    if arch.get("pool_proj_dim"):
        want["attn_pool.proj.weight"] = (arch["pool_proj_dim"], P)
    for i in range(arch["depth"]):
        b = f"blocks.{i}."
        want.update({b + "ln1.weight": (d,), b + "ln1.bias": (d,), b + "qkv.weight": (3 * d, d), b + "qkv.bias": (3 * d,),
                     b + "proj.weight": (d, d), b + "proj.bias": (d,), b + "ln2.weight": (d,), b + "ln2.bias": (d,),
                     b + "fc1.weight": (mlp, d), b + "fc1.bias": (mlp,), b + "fc2.weight": (d, mlp), b + "fc2.bias": (d,)})
        if arch.get("layer_scale"):
            want.update({b + "ls1": (d,), b + "ls2": (d,)})
    return want


def _mapped_canonical(src: dict, table: dict, pool_prefix: str, ln_out: str, arch: dict, *, family: str, source: str) -> dict:
    """The body both pooler-tower adapters share: ``table`` (canonical name -> checkpoint key, or a callable on the checkpoint)
    plus the pooler under ``pool_prefix`` with ``ln_out`` as its closing LayerNorm, checked against ``attn_tower_canonical_shapes``.
    A checkpoint key nothing reads, a key the architecture needs and a wrong shape are each a ``ValueError`` naming it."""
    used: set = set()
    out: dict[str, torch.Tensor] = {}

    def take(key):
        used.add(key)
        return src.get(key)

    for name, key in table.items():
        t = take(key)
        if t is not None:
            out[name] = t.detach().to(dtype=torch.float32, device="cpu").contiguous()
    pool = {k: take(pool_prefix + k) for k in POOLER_KEYS}
    pool["ln_out.weight"], pool["ln_out.bias"] = take(ln_out + ".weight"), take(ln_out + ".bias")
    if arch.get("pool_proj_dim"):
        pool["proj"] = take("proj")
    P, d = arch["pool_dim"], arch["dim"]
    shapes = {"query": None, "ln_q.weight": (P,), "ln_q.bias": (P,), "ln_k.weight": (d,), "ln_k.bias": (d,),
              "attn.q_proj_weight": (P, P), "attn.k_proj_weight": (P, d), "attn.v_proj_weight": (P, d), "attn.in_proj_bias": (3 * P,),
              "attn.out_proj.weight": (P, P), "attn.out_proj.bias": (P,), "ln_out.weight": (P,), "ln_out.bias": (P,),
              "proj": (P, arch.get("pool_proj_dim") or 0)}
    for k, t in pool.items():                                          # what the float64 fold below multiplies must fit first
        want = shapes[k]
        if t is not None and (tuple(t.shape) != want if want else (t.dim() != 2 or t.shape[1] != P)):
            key = {"ln_out.weight": ln_out + ".weight", "ln_out.bias": ln_out + ".bias", "proj": "proj"}.get(k, pool_prefix + k)
            raise ValueError(f"{family} checkpoint: {key} has shape {tuple(t.shape)}, expected {want or ('Q', P)}")
    if all(t is not None for k, t in pool.items() if k != "proj"):
        out.update(attn_pool_canonical({k: t for k, t in pool.items() if t is not None}, pool_eps=arch.get("pool_ln_eps", 1e-5)))
    unknown = sorted(k for k in src if k not in used)
    absent = sorted(k for k in used if k not in src)
    try:
        return check_canonical(out, attn_tower_canonical_shapes(arch), unknown, family=family, source=source)
    except ValueError as exc:
        if unknown or not absent:
            raise
        raise ValueError(f"{exc}; the checkpoint lacks {absent[:5]}") from None


def coca_canonical_state_dict(sd: dict, arch: dict) -> dict:
    """The ``open_clip_coca`` adapter: open_clip's CoCa visual tower (``coca_ViT-L-14``; key names from the public package [3P],
    unverified offline) -> canonical names.  Takes ``visual.*`` bare or prefixed, or the whole CoCa model, whose ``text.*``,
    ``text_decoder.*`` and ``logit_scale`` are dropped.  ``conv1`` has no bias (zeros are uploaded, as for the CLIP towers); there
    is no LayerNorm after the last block; query row 0 is folded through ``ln_q`` and ``q_proj`` in float64 (``attn_pool_canonical``);
    ``ln_post`` closes the pooler and ``proj`` is stored transposed as ``attn_pool.proj.weight``."""
    src = {k: v for k, v in sd.items() if not (k.startswith("text.") or k.startswith("text_decoder.") or k == "logit_scale")}
    if any(k.startswith("visual.") for k in src):
        src = {(k[len("visual."):] if k.startswith("visual.") else k): v for k, v in src.items()}
    d = arch["dim"]
    table = {"patch_embed.weight": "conv1.weight", "cls_token": "class_embedding", "pos_embed": "positional_embedding",
             "pre_norm.weight": "ln_pre.weight", "pre_norm.bias": "ln_pre.bias"}
    for i in range(arch["depth"]):
        p, b = f"transformer.resblocks.{i}.", f"blocks.{i}."
        table.update({b + "ln1.weight": p + "ln_1.weight", b + "ln1.bias": p + "ln_1.bias",
                      b + "qkv.weight": p + "attn.in_proj_weight", b + "qkv.bias": p + "attn.in_proj_bias",
                      b + "proj.weight": p + "attn.out_proj.weight", b + "proj.bias": p + "attn.out_proj.bias",
                      b + "ln2.weight": p + "ln_2.weight", b + "ln2.bias": p + "ln_2.bias",
                      b + "fc1.weight": p + "mlp.c_fc.weight", b + "fc1.bias": p + "mlp.c_fc.bias",
                      b + "fc2.weight": p + "mlp.c_proj.weight", b + "fc2.bias": p + "mlp.c_proj.bias"})
    src = dict(src)
    src["<zero patch-embedding bias>"] = torch.zeros(d)
    table["patch_embed.bias"] = "<zero patch-embedding bias>"
    return _mapped_canonical(src, table, "attn_pool.", "ln_post", arch, family="CoCa", source="open_clip_coca")


def conch_v15_canonical_state_dict(sd: dict, arch: dict) -> tuple[dict, bool]:
    """CONCH v1.5 (``conch_v1_5.py`` of the TITAN repository; key names from the public package [3P], unverified offline) ->
    (canonical names, layer_scale).  ``trunk.*`` (timm ViT-L/16), ``attn_pool_contrast.*`` and ``ln_contrast.*``, bare or under
    ``visual.`` / ``vision_encoder.``.  LayerScale is taken from the checkpoint when ``trunk.blocks.<i>.ls1.gamma`` is there; a
    checkpoint without it gives a model without it (the second value)."""
    root = next((r for r in ("visual.", "vision_encoder.", "") if any(k.startswith(r + "trunk.") for k in sd)), "")
    src = {(k[len(root):] if k.startswith(root) else k): v for k, v in sd.items()}
    layer_scale = "trunk.blocks.0.ls1.gamma" in src
    if "trunk.cls_token" in src:                                       # timm keeps a leading batch axis on both
        src["trunk.cls_token"] = src["trunk.cls_token"].reshape(-1)
    if "trunk.pos_embed" in src and src["trunk.pos_embed"].dim() == 3:
        src["trunk.pos_embed"] = src["trunk.pos_embed"][0]
    table = {"patch_embed.weight": "trunk.patch_embed.proj.weight", "patch_embed.bias": "trunk.patch_embed.proj.bias",
             "cls_token": "trunk.cls_token", "pos_embed": "trunk.pos_embed", "norm.weight": "trunk.norm.weight",
             "norm.bias": "trunk.norm.bias"}
    for i in range(arch["depth"]):
        p, b = f"trunk.blocks.{i}.", f"blocks.{i}."
        table.update({b + "ln1.weight": p + "norm1.weight", b + "ln1.bias": p + "norm1.bias",
                      b + "qkv.weight": p + "attn.qkv.weight", b + "qkv.bias": p + "attn.qkv.bias",
                      b + "proj.weight": p + "attn.proj.weight", b + "proj.bias": p + "attn.proj.bias",
                      b + "ln2.weight": p + "norm2.weight", b + "ln2.bias": p + "norm2.bias",
                      b + "fc1.weight": p + "mlp.fc1.weight", b + "fc1.bias": p + "mlp.fc1.bias",
                      b + "fc2.weight": p + "mlp.fc2.weight", b + "fc2.bias": p + "mlp.fc2.bias"})
        if layer_scale:
            table.update({b + "ls1": p + "ls1.gamma", b + "ls2": p + "ls2.gamma"})
    spec = dict(arch, layer_scale=layer_scale)
    return _mapped_canonical(src, table, "attn_pool_contrast.", "ln_contrast", spec, family="CONCH v1.5", source="conch_v15"), layer_scale


def random_attn_pool(arch: dict, seed: int = 0) -> dict:
    """Seeded AttentionalPooler tensors (module-style names) for tests / benchmarks."""
    g = torch.Generator().manual_seed(seed + 7919)
    P, C = arch["pool_dim"], arch["dim"]
    w = lambda *shape, s=0.02: torch.randn(*shape, generator=g) * s
    return {"query": torch.randn(1, P, generator=g), "ln_q.weight": 1.0 + w(P, s=0.1), "ln_q.bias": w(P),
            "ln_k.weight": 1.0 + w(C, s=0.1), "ln_k.bias": w(C),
            "attn.q_proj_weight": w(P, P, s=0.05), "attn.k_proj_weight": w(P, C, s=0.05),
            "attn.v_proj_weight": w(P, C, s=0.05), "attn.in_proj_bias": w(3 * P),
            "attn.out_proj.weight": w(P, P, s=0.05), "attn.out_proj.bias": w(P),
            "ln_out.weight": 1.0 + w(P, s=0.1), "ln_out.bias": w(P)}


def random_canonical_state_dict(arch: dict, seed: int = 0) -> dict:
    """Seeded random-init weights (trunc-normal-ish sigma 0.02, LN gamma ~ 1): there are no
    pretrained checkpoints offline."""
    g = torch.Generator().manual_seed(seed)
    d, mlp, ps = arch["dim"], arch["mlp_dim"], arch["patch_size"]
    reg = int(arch.get("reg_tokens", 0))
    patches = (arch["image_size"] // ps) ** 2
    tokens = patches if (arch.get("no_embed_class") or arch.get("no_class_token")) else 1 + reg + patches   # rows of the position embedding
    f1 = 2 * mlp if arch.get("mlp") == "swiglu" else mlp

    def w(*shape, s=0.02):
        return torch.randn(*shape, generator=g) * s

    sd = {"patch_embed.weight": w(d, 3, ps, ps), "patch_embed.bias": w(d), "cls_token": w(d),
          "pos_embed": w(tokens, d), "norm.weight": 1.0 + w(d, s=0.1), "norm.bias": w(d)}
    if reg:
        sd["reg_tokens"] = w(reg, d)
    for i in range(arch["depth"]):
        b = f"blocks.{i}."
        sd[b + "ln1.weight"] = 1.0 + w(d, s=0.1); sd[b + "ln1.bias"] = w(d)
        sd[b + "qkv.weight"] = w(3 * d, d); sd[b + "qkv.bias"] = w(3 * d)
        sd[b + "proj.weight"] = w(d, d); sd[b + "proj.bias"] = w(d)
        sd[b + "ln2.weight"] = 1.0 + w(d, s=0.1); sd[b + "ln2.bias"] = w(d)
        sd[b + "fc1.weight"] = w(f1, d); sd[b + "fc1.bias"] = w(f1)
        sd[b + "fc2.weight"] = w(d, mlp); sd[b + "fc2.bias"] = w(d)
        if arch.get("layer_scale"):
            sd[b + "ls1"] = torch.full((d,), 1e-5) + w(d, s=1e-6)
            sd[b + "ls2"] = torch.full((d,), 1e-5) + w(d, s=1e-6)
    if arch.get("no_class_token"):
        del sd["cls_token"]
    if arch.get("pool") == "map":                                    # SigLIP's head, unpadded (map.q as the adapter folds it)
        sd.update({"map.q": w(d, s=0.5), "map.kv.weight": w(2 * d, d), "map.kv.bias": w(2 * d), "map.out.weight": w(d, d),
                   "map.out.bias": w(d), "map.ln.weight": 1.0 + w(d, s=0.1), "map.ln.bias": w(d), "map.fc1.weight": w(mlp, d),
                   "map.fc1.bias": w(mlp), "map.fc2.weight": w(d, mlp), "map.fc2.bias": w(d)})
    if arch.get("pool") == "attn":
        sd.update(attn_pool_canonical(random_attn_pool(arch, seed), pool_eps=arch.get("pool_ln_eps", 1e-5)))
    if arch.get("rope"):
        sd["pos_embed"] = torch.zeros_like(sd["pos_embed"])
        sd["rope.cos"], sd["rope.sin"] = dinov3_rope_tables(arch["image_size"] // ps, d // arch["heads"], float(arch.get("rope_theta", 100.0)))
    if arch.get("pre_norm"):
        sd["pre_norm.weight"] = 1.0 + w(d, s=0.1); sd["pre_norm.bias"] = w(d)
    if arch.get("proj_dim"):
        sd["head_proj.weight"] = w(arch["proj_dim"], d, s=d ** -0.5)
    if arch.get("pool_proj_dim"):                                     # CoCa's `proj`, as the adapter stores it: [P2, P]
        sd["attn_pool.proj.weight"] = w(arch["pool_proj_dim"], arch["pool_dim"], s=arch["pool_dim"] ** -0.5)
    if arch.get("pool_skip_final_norm"):                              # no LayerNorm after the last block: no norm.* parameters
        del sd["norm.weight"], sd["norm.bias"]
    return sd


# ----------------------------------------------------------------------------- device object
class HipViT(NativeEncoder):
    """Device-resident ViT encoder behind ``ap_vit_*``."""

    ABI = "vit"
    PROF_KINDS = _lib.PROF_KINDS

    def __init__(self, arch: dict, state: dict, *, device: torch.device, dtype: torch.dtype) -> None:
        self._bind(device, dtype)
        self.arch = dict(arch)
        attn_pool = arch.get("pool") == "attn"
        cls_mean = arch.get("pool") == "cls_mean"          # [class token | mean of the patch tokens] (midnight.py:58-61)
        map_head = arch.get("pool") == "map"               # SigLIP's attention-pooling head (medsiglip.py:63): dim floats
        self.embed_dim = int(arch["pool_dim"] if attn_pool else (2 * arch["dim"] if cls_mean else arch["dim"]))
        if arch.get("proj_dim"):                           # CLIP visual projection
            self.embed_dim = int(arch["proj_dim"])
        hd_true = arch["dim"] // arch["heads"]
        hd_stored = stored_head_dim(arch["dim"], arch["heads"])
        if arch.get("pool_proj_dim"):                      # CoCa's projection after the pooler
            self.embed_dim = int(arch["pool_proj_dim"])
        # the fields appended since ABI v20 travel in the longer structures; every other model hands over the v20 one, as before
        ex2 = [int(arch.get("pool_head_dim", 0)), 1 if arch.get("pool_skip_final_norm") else 0, int(arch.get("pool_proj_dim", 0)),
               1 if arch.get("out_normalize") else 0]
        tail = [1 if arch.get("no_class_token") else 0] + ex2 if any(ex2) else ([1] if arch.get("no_class_token") else [])
        config = _lib.VitConfigEx2 if any(ex2) else (_lib.VitConfigEx if arch.get("no_class_token") else _lib.VitConfig)
        cfg = config(arch["image_size"], arch["patch_size"], arch["dim"], arch["depth"],
                             arch["heads"], stored_mlp_dim(arch["mlp_dim"]), float(arch["ln_eps"]),
                             1 if arch.get("layer_scale") else 0, _lib.torch_dtype_code(dtype),
                             1 if attn_pool else (2 if cls_mean else (3 if map_head else 0)), int(arch.get("pool_dim", 0)), int(arch.get("pool_heads", 0)),
                             float(arch.get("pool_ln_eps", 1e-5)),
                             int(arch.get("reg_tokens", 0)), 1 if arch.get("no_embed_class") else 0,
                             1 if arch.get("mlp") == "swiglu" else 0, hd_stored,
                             0.0 if hd_stored == hd_true else float(1.0 / np.sqrt(np.float32(hd_true))),
                             1 if arch.get("pre_norm") else 0, {"quick_gelu": 1, "gelu_tanh": 2}.get(arch.get("act"), 0),
                             int(arch.get("proj_dim", 0)), 1 if arch.get("rope") else 0,
                     *tail)
        state = pad_heads(state, dim=arch["dim"], heads=arch["heads"], depth=arch["depth"])
        state = pad_mlp(state, mlp_dim=arch["mlp_dim"], depth=arch["depth"], swiglu=arch.get("mlp") == "swiglu")
        self._open(cfg, state)

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
    if seeded:
        source = "canonical"
    if spec.get("pool") == "map" and source == "auto" and _detect_source(state_dict) == "hf_siglip":
        source = "hf_siglip"
    if source == "hf_siglip":
        state_dict, source = siglip_canonical_state_dict(state_dict, spec), "canonical"
    pool_state = None
    if spec.get("pool") == "attn" and source != "canonical":
        if any(k.startswith("visual.trunk.") for k in state_dict):          # a CONCH checkpoint
            state_dict, pool = conch_state_dicts(state_dict)
            pool_state = attn_pool_canonical(pool, pool_eps=spec.get("pool_ln_eps", 1e-5))
        else:                                                                # trunk dict + "attn_pool.*" tensors
            pool_state = {k: v for k, v in state_dict.items() if k.startswith("attn_pool.")}
            state_dict = {k: v for k, v in state_dict.items() if not k.startswith("attn_pool.")}
    state = canonical_state_dict(state_dict, depth=spec["depth"], layer_scale=bool(spec.get("layer_scale")),
                                 source=source, grid=spec["image_size"] // spec["patch_size"], heads=spec["heads"],
                                 rope_theta=float(spec.get("rope_theta", 100.0)))
    if pool_state:
        state.update({k: v.detach().to(torch.float32).cpu().contiguous() for k, v in pool_state.items()})
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


def medsiglip_max_batch(vit: "HipViT", cap: int = 128, budget_bytes: int = 16 << 30) -> int:
    """The largest batch <= cap whose ``ap_vit_workspace_bytes`` fits the budget (1024 tokens of 1152: ~90 MB per image in float16)."""
    n = cap
    while n > 1 and int(vit.lib.ap_vit_workspace_bytes(vit._handle, n)) > budget_bytes:
        n //= 2
    return n


def register_medsiglip(registry, *, device, dtype=torch.float32, num_workers: int = 0, **arch_overrides) -> None:
    """medsiglip (models/patch/medsiglip.py): transformers' SiglipVisionModel of google/medsiglip-448, features =
    ``get_image_features`` = ``pooler_output`` of the vision tower (the attention-pooling head's 1152 floats).  Transform: the
    processor's resize to 448 x 448 (bilinear), rescale, Normalize(0.5, 0.5) -- resize and normalisation on the device.  float16 /
    bfloat16 only: 1024 tokens and 72-wide heads are outside the float32 attention kernel's limits.  HF state dict (vision tower
    alone or the whole SiglipModel) as ``$ATLASPATCH_WEIGHTS_DIR/medsiglip.safetensors``."""
    def build():
        spec = dict(ARCHS["medsiglip"]); spec.update(arch_overrides)
        tokens = (spec["image_size"] // spec["patch_size"]) ** 2
        if dtype == torch.float32 and (tokens > 288 or stored_head_dim(spec["dim"], spec["heads"]) != 64):
            raise ValueError(f"medsiglip: --feature-precision float32 is not available: {tokens} tokens with heads stored "
                             f"{stored_head_dim(spec['dim'], spec['heads'])} wide exceed the float32 attention kernel's limits (288 "
                             "tokens, 64 wide); use float16 or bfloat16")
        size, filt, mean, std = medsiglip_transform()
        if size != spec["image_size"]:
            raise ValueError(f"medsiglip: the preprocessor config resizes to {size}, the model takes {spec['image_size']}")
        ex = build_hip_vit_extractor(name="medsiglip", arch=spec, device=device, dtype=dtype, random_init_seed=_env_seed(),
                                     mean=mean, std=std, resize=(size, filt), expect_size=None, max_batch=128, square_resize=True)
        ex.max_batch = medsiglip_max_batch(ex.vit)
        return ex
    registry.register("medsiglip", build)


def register_coca_towers(registry, *, device, dtype=torch.float32, num_workers: int = 0, **arch_overrides) -> None:
    """omiclip (models/patch/omiclip.py: open_clip ``coca_ViT-L-14``, ``encode_image``) and conch_v15 (models/patch/conch.py:67-112:
    ``build_conch(ConchConfig())`` of the TITAN repository): ViT-L trunks whose features come from an attentional pooler with eight
    96-wide heads over the 1024-wide tokens.  Both architectures are restated from the public packages, unverified offline (see
    ``ARCHS``).  Transform: Pillow-exact bicubic resize of the shorter side to 224 / 448 and the centre crop on the device, OpenAI
    CLIP / ImageNet constants.  Weights: ``$ATLASPATCH_WEIGHTS_DIR/<name>.{safetensors,pt,pth}`` (omiclip: ``visual.*`` bare or
    prefixed, or the whole CoCa model; conch_v15: ``trunk.*`` / ``attn_pool_contrast.*`` / ``ln_contrast.*``, bare or under
    ``visual.`` / ``vision_encoder.``) or ``ATLASPATCH_RANDOM_INIT=<seed>``.  omiclip runs in float32 too (257 tokens); conch_v15
    (785 tokens) in float16 / bfloat16 only.  Not in the default registry: ``plugins/coca_towers.py`` ships them."""
    def build(name):
        spec = dict(ARCHS[name]); spec.update(arch_overrides)
        tokens = 1 + (spec["image_size"] // spec["patch_size"]) ** 2
        if dtype == torch.float32 and (tokens > 288 or stored_head_dim(spec["dim"], spec["heads"]) != 64):
            raise ValueError(f"{name}: --feature-precision float32 is not available: {tokens} tokens with heads stored "
                             f"{stored_head_dim(spec['dim'], spec['heads'])} wide exceed the float32 attention kernel's limits (288 "
                             "tokens, 64 wide); use float16 or bfloat16")
        state, path = None, weights_path(name)
        if path is not None:
            if name == "omiclip":
                state = coca_canonical_state_dict(load_checkpoint(path), spec)
            else:
                state, spec["layer_scale"] = conch_v15_canonical_state_dict(load_checkpoint(path), spec)
        mean, std = TRANSFORM_NORM[name]
        ex = build_hip_vit_extractor(name=name, arch=spec, device=device, dtype=dtype, state_dict=state, source="canonical" if state else "auto",
                                     random_init_seed=_env_seed(), mean=mean, std=std, resize=TRANSFORM_RESIZE[name], expect_size=None,
                                     max_batch=256)
        ex.max_batch = medsiglip_max_batch(ex.vit, cap=256)          # ap_vit_workspace_bytes against the byte budget
        return ex
    for name in ("omiclip", "conch_v15"):
        registry.register(name, lambda n=name: build(n))


def register_conch(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """conch_v1 (models/patch/conch.py:20-64): open_clip image transform = Resize(448, bicubic) + CenterCrop(448)
    + ToTensor + Normalize(OpenAI CLIP mean / std) [3P]; all of it on the device (the resize is Pillow-exact,
    ap_resample_u8).  float16 / bfloat16 only (the reference's config 5 runs it in fp16)."""
    registry.register("conch_v1", lambda: build_hip_vit_extractor(
        name="conch_v1", arch="conch_v1", device=device, dtype=dtype, random_init_seed=_env_seed(),
        mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD, resize=TRANSFORM_RESIZE["conch_v1"], expect_size=None,
        max_batch=256))


def register_vits(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """vit_b_16 / vit_l_16 with torchvision's transform semantics: ImageClassification(crop 224, resize R, bilinear)
    on the PIL tile (models/patch/base.py:42-45 hands the transform a PIL image, so the resize is Pillow's BILINEAR),
    R = 256 for vit_b_16 and 242 for vit_l_16 (``TRANSFORM_RESIZE``).  vit_b_16 on the default 256-px tiles is a pure
    centre crop; vit_l_16 resamples every 256-px tile to 242 first; any other --patch-size goes through the same
    Pillow-exact device resize (shorter side -> R)."""
    for name in ("vit_b_16", "vit_l_16"):
        registry.register(name, lambda n=name: build_hip_vit_extractor(
            name=n, arch=n, device=device, dtype=dtype, random_init_seed=_env_seed(), resize=TRANSFORM_RESIZE[n],
            expect_size=None, max_batch=2048))
    # the other three names of models/patch/vit.py:9-15.  vit_b_32 / vit_l_32: 32-px patches, 50 tokens, same transform as
    # vit_b_16.  vit_h_14: torchvision has no IMAGENET1K_V1 entry for it, so the reference (base.py:123-143) takes DEFAULT =
    # IMAGENET1K_SWAG_E2E_V1: 518-px input (Pillow BICUBIC resize of the tile, on the device), 1370 tokens, 80-wide heads
    for name, cap in (("vit_b_32", 4096), ("vit_l_32", 4096), ("vit_h_14", 128)):
        registry.register(name, lambda n=name, c=cap: build_hip_vit_extractor(
            name=n, arch=n, device=device, dtype=dtype, random_init_seed=_env_seed(), resize=TRANSFORM_RESIZE[n],
            expect_size=None, max_batch=c))


def register_uni(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """uni_v1: timm ViT-L/16 + LayerScale; timm transform Resize(224, bicubic) + CenterCrop(224):
    the resize runs on the device bit-identically to Pillow (ap_resample_u8), the crop in the preprocess kernel."""
    registry.register("uni_v1", lambda: build_hip_vit_extractor(
        name="uni_v1", arch="uni_v1", device=device, dtype=dtype, random_init_seed=_env_seed(),
        resize=TRANSFORM_RESIZE["uni_v1"], expect_size=None, max_batch=2048))
    # uni_v2 = UNI2-h (uni.py:62-125): ViT-H/14 at 224 px with 8 register tokens, SwiGLUPacked MLP, LayerScale; same timm
    # transform as uni_v1.  Checkpoint: timm key names (pytorch_model.bin of MahmoodLab/UNI2-h) in ATLASPATCH_WEIGHTS_DIR
    registry.register("uni_v2", lambda: build_hip_vit_extractor(
        name="uni_v2", arch="uni_v2", device=device, dtype=dtype, random_init_seed=_env_seed(),
        resize=TRANSFORM_RESIZE["uni_v2"], expect_size=None, max_batch=1024))


def register_dinov2(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """dinov2_small / base / large / giant (models/patch/dinov2.py:12-17): the reference runs transformers' Dinov2Model on the
    processor's output and returns the class token of ``last_hidden_state``.  Same device kernels as the other encoders (LayerScale
    folded, giant: SwiGLU gate in the fc1 epilogue); checkpoints: the HF state dict (model.safetensors of facebook/dinov2-*) as
    ``$ATLASPATCH_WEIGHTS_DIR/<name>.safetensors``."""
    for name, cap in (("dinov2_small", 4096), ("dinov2_base", 2048), ("dinov2_large", 2048), ("dinov2_giant", 512)):
        registry.register(name, lambda n=name, c=cap: build_hip_vit_extractor(
            name=n, arch=n, device=device, dtype=dtype, random_init_seed=_env_seed(), resize=TRANSFORM_RESIZE[n],
            expect_size=None, max_batch=c))


def register_phikon(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """phikon_v1 (transformers ViTModel, ViT-B/16, LayerNorm eps 1e-12) and phikon_v2 (Dinov2Model ViT-L/16), models/patch/phikon.py:
    class token of ``last_hidden_state``.  HF state dicts in ATLASPATCH_WEIGHTS_DIR."""
    for name in ("phikon_v1", "phikon_v2"):
        registry.register(name, lambda n=name: build_hip_vit_extractor(
            name=n, arch=n, device=device, dtype=dtype, random_init_seed=_env_seed(), resize=TRANSFORM_RESIZE[n],
            expect_size=None, max_batch=2048))


def register_more_vits(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """The other loader files whose model is a plain ViT this engine runs: midnight (models/patch/midnight.py, transformers
    Dinov2Model giant, class token + mean patch token), h_optimus_0 / h_optimus_1 (hoptimus.py), prov_gigapath (gigapath.py),
    virchow_v1 / virchow_v2 (virchow.py: 80-wide heads and a 3416-wide SwiGLU stored zero-padded, class | mean patch token),
    the two Lunit ViT-S (lunit.py) and pathorchestra (pathorchestra.py).  Checkpoints: HF (midnight) or timm key names in
    ATLASPATCH_WEIGHTS_DIR; each with the transform its loader file writes out (``TRANSFORM_RESIZE`` / ``TRANSFORM_NORM``)."""
    for name, cap in (("midnight", 512), ("h_optimus_0", 512), ("h_optimus_1", 512), ("prov_gigapath", 512),
                      ("virchow_v1", 512), ("virchow_v2", 512), ("h0_mini", 2048),
                      ("lunit_vit_small_patch16_dino", 4096), ("lunit_vit_small_patch8_dino", 512), ("pathorchestra", 2048)):
        mean, std = TRANSFORM_NORM.get(name, (IMAGENET_MEAN, IMAGENET_STD))
        registry.register(name, lambda n=name, c=cap, mu=mean, sd=std: build_hip_vit_extractor(
            name=n, arch=n, device=device, dtype=dtype, random_init_seed=_env_seed(), resize=TRANSFORM_RESIZE[n],
            expect_size=None, max_batch=c, mean=mu, std=sd))


def register_clip(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """The CLIP vision towers with a plain ViT: clip_vit_b_32 / b_16 / l_14 / l_14_336 (models/patch/clip.py, open_clip, OpenAI
    weights), plip (plip.py) and quilt_b_32 / quilt_b_16 (quilt.py), both transformers CLIPModel; features = encode_image /
    get_image_features (projected, not normalised); biomedclip (biomedclip.py: timm ViT-B/16 trunk + linear projection).  Checkpoints: open_clip or HF CLIP state dicts in ATLASPATCH_WEIGHTS_DIR.
    (The ResNet CLIPs, quilt_b_16_pmb and omiclip are other architectures.)"""
    for name, cap in (("clip_vit_b_32", 4096), ("clip_vit_b_16", 2048), ("clip_vit_l_14", 1024), ("clip_vit_l_14_336", 256),
                      ("plip", 4096), ("quilt_b_32", 4096), ("quilt_b_16", 2048), ("biomedclip", 2048)):
        mean, std = TRANSFORM_NORM[name]
        registry.register(name, lambda n=name, c=cap, mu=mean, sd=std: build_hip_vit_extractor(
            name=n, arch=n, device=device, dtype=dtype, random_init_seed=_env_seed(), resize=TRANSFORM_RESIZE[n],
            expect_size=None, max_batch=c, mean=mu, std=sd))


def register_dinov3(registry, *, device, dtype=torch.float32, num_workers: int = 0) -> None:
    """dinov3_vits16 / vits16_plus / vitb16 / vitl16 / vitl16_sat / vith16_plus / vit7b16 / vit7b16_sat (models/patch/dinov3.py:12-21):
    transformers' DINOv3ViTModel, ``pooler_output``.  Rotary position embedding applied in place on q / k after the qkv GEMM (``ap::launch_rope``);
    HF state dicts in ATLASPATCH_WEIGHTS_DIR."""
    for name, cap in (("dinov3_vits16", 4096), ("dinov3_vits16_plus", 4096), ("dinov3_vitb16", 2048), ("dinov3_vitl16", 2048),
                      ("dinov3_vitl16_sat", 2048), ("dinov3_vith16_plus", 1024), ("dinov3_vit7b16", 512), ("dinov3_vit7b16_sat", 512)):
        mean, std = TRANSFORM_NORM.get(name, (IMAGENET_MEAN, IMAGENET_STD))
        registry.register(name, lambda n=name, c=cap, mu=mean, sd=std: build_hip_vit_extractor(
            name=n, arch=n, device=device, dtype=dtype, random_init_seed=_env_seed(), resize=TRANSFORM_RESIZE[n],
            expect_size=None, max_batch=c, mean=mu, std=sd))
