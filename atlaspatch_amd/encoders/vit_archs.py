"""The ViT family's tables, keyed by encoder name, and nothing else: ``ARCHS`` (the architecture), ``TRANSFORM_RESIZE`` and
``TRANSFORM_NORM`` (the reference transform) and ``MAX_BATCH`` (the batch cap the extractor is built with).  File names in the
comments are the reference's loader files under ``models/patch/``."""
from __future__ import annotations

from .checkpoints import IMAGENET_MEAN, IMAGENET_STD, OPENAI_CLIP_MEAN, OPENAI_CLIP_STD

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

# Largest batch one forward takes, per registered name (the extractor splits longer runs of tiles).  medsiglip, omiclip and
# conch_v15 are caps: their builders halve them until ``ap_vit_workspace_bytes`` fits the byte budget.
MAX_BATCH = {
    "vit_b_16": 2048, "vit_l_16": 2048, "vit_b_32": 4096, "vit_l_32": 4096, "vit_h_14": 128, "uni_v1": 2048, "uni_v2": 1024, "conch_v1": 256,
    "dinov2_small": 4096, "dinov2_base": 2048, "dinov2_large": 2048, "dinov2_giant": 512, "phikon_v1": 2048, "phikon_v2": 2048,
    "midnight": 512, "h_optimus_0": 512, "h_optimus_1": 512, "prov_gigapath": 512, "virchow_v1": 512, "virchow_v2": 512, "h0_mini": 2048,
    "lunit_vit_small_patch16_dino": 4096, "lunit_vit_small_patch8_dino": 512, "pathorchestra": 2048,
    "clip_vit_b_32": 4096, "clip_vit_b_16": 2048, "clip_vit_l_14": 1024, "clip_vit_l_14_336": 256, "plip": 4096, "quilt_b_32": 4096,
    "quilt_b_16": 2048, "biomedclip": 2048,
    "dinov3_vits16": 4096, "dinov3_vits16_plus": 4096, "dinov3_vitb16": 2048, "dinov3_vitl16": 2048, "dinov3_vitl16_sat": 2048,
    "dinov3_vith16_plus": 1024, "dinov3_vit7b16": 512, "dinov3_vit7b16_sat": 512,
    "medsiglip": 128, "omiclip": 256, "conch_v15": 256,
}
