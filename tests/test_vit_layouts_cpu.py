"""The ViT family's host code off the GPU: every lenient checkpoint layout round-trips (a canonical state dict renamed INTO the
layout, with the renaming written out here, comes back key for key and bit for bit; a missing key is a ``KeyError`` naming
it), ``canonical_shapes`` states the parameter set that ``random_canonical_state_dict`` draws for every architecture, the
``ap_vit_config`` structures of seven architectures field by field, and what each registered name is built with."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

TINY = dict(image_size=32, patch_size=16, dim=128, depth=2, heads=2, mlp_dim=256, ln_eps=1e-6, layer_scale=False)   # grid 2, 5 tokens
IGNORED = {"heads.head.weight": torch.ones(3, 128), "head.weight": torch.ones(3, 128), "head.bias": torch.ones(3),
           "text.transformer.resblocks.0.ln_1.weight": torch.ones(8), "text_model.embeddings.token_embedding.weight": torch.ones(4, 8),
           "text_projection.weight": torch.ones(8, 8), "logit_scale": torch.ones(())}


def _canon(seed=0, **flags):
    from atlaspatch_amd.encoders.vit import random_canonical_state_dict
    arch = dict(TINY, **flags)
    return arch, random_canonical_state_dict(arch, seed)


def _rename(canon, top, block, depth=2):
    """``top``: canonical name -> checkpoint name; ``block``: canonical part -> checkpoint part with ``{i}``."""
    out = {ck: canon[name] for name, ck in top.items()}
    for i in range(depth):
        for part, ck in block.items():
            out[ck.format(i=i)] = canon[f"blocks.{i}.{part}"]
    return out


def _split(sd, key, names):
    """Replace the stacked tensor ``key`` by its equal parts under ``names`` (q | k | v, gate | up)."""
    for name, part in zip(names, sd.pop(key).chunk(len(names), 0)):
        sd[name] = part.clone()


def torchvision(f1="mlp.0", f2="mlp.3"):
    arch, canon = _canon(1)
    p = "encoder.layers.encoder_layer_{i}."
    sd = _rename(canon, {"patch_embed.weight": "conv_proj.weight", "patch_embed.bias": "conv_proj.bias", "norm.weight": "encoder.ln.weight",
                         "norm.bias": "encoder.ln.bias"},
                 {"ln1.weight": p + "ln_1.weight", "ln1.bias": p + "ln_1.bias", "qkv.weight": p + "self_attention.in_proj_weight",
                  "qkv.bias": p + "self_attention.in_proj_bias", "proj.weight": p + "self_attention.out_proj.weight",
                  "proj.bias": p + "self_attention.out_proj.bias", "ln2.weight": p + "ln_2.weight", "ln2.bias": p + "ln_2.bias",
                  "fc1.weight": p + f1 + ".weight", "fc1.bias": p + f1 + ".bias", "fc2.weight": p + f2 + ".weight", "fc2.bias": p + f2 + ".bias"})
    sd["class_token"] = canon["cls_token"].reshape(1, 1, -1)
    sd["encoder.pos_embedding"] = canon["pos_embed"][None]
    return arch, canon, sd, "torchvision", f"encoder.layers.encoder_layer_1.{f2}.bias"


TIMM_BLOCK = {"ln1.weight": "blocks.{i}.norm1.weight", "ln1.bias": "blocks.{i}.norm1.bias", "qkv.weight": "blocks.{i}.attn.qkv.weight",
              "qkv.bias": "blocks.{i}.attn.qkv.bias", "proj.weight": "blocks.{i}.attn.proj.weight", "proj.bias": "blocks.{i}.attn.proj.bias",
              "ln2.weight": "blocks.{i}.norm2.weight", "ln2.bias": "blocks.{i}.norm2.bias", "fc1.weight": "blocks.{i}.mlp.fc1.weight",
              "fc1.bias": "blocks.{i}.mlp.fc1.bias", "fc2.weight": "blocks.{i}.mlp.fc2.weight", "fc2.bias": "blocks.{i}.mlp.fc2.bias"}
TIMM_TOP = {"patch_embed.weight": "patch_embed.proj.weight", "patch_embed.bias": "patch_embed.proj.bias", "norm.weight": "norm.weight",
            "norm.bias": "norm.bias"}


def _timm(canon, layer_scale=False):
    block = dict(TIMM_BLOCK, **({"ls1": "blocks.{i}.ls1.gamma", "ls2": "blocks.{i}.ls2.gamma"} if layer_scale else {}))
    sd = _rename(canon, TIMM_TOP, block)
    sd["cls_token"] = canon["cls_token"].reshape(1, 1, -1)
    sd["pos_embed"] = canon["pos_embed"][None]
    if "reg_tokens" in canon:
        sd["reg_token"] = canon["reg_tokens"][None]
    return sd


def timm_plain():
    arch, canon = _canon(2)
    return arch, canon, _timm(canon), "timm", "blocks.0.attn.proj.bias"


def timm_registers_layerscale_swiglu():
    arch, canon = _canon(3, layer_scale=True, reg_tokens=2, no_embed_class=True, mlp="swiglu")
    return arch, canon, _timm(canon, layer_scale=True), "timm", "blocks.1.ls2.gamma"


def open_clip_timm():
    arch, canon = _canon(4, proj_dim=64)
    sd = {"visual.trunk." + k: v for k, v in _timm({k: v for k, v in canon.items() if k != "head_proj.weight"}).items()}
    sd["visual.head.proj.weight"] = canon["head_proj.weight"]
    sd["text.proj.weight"] = torch.ones(4, 4)
    return arch, canon, sd, "open_clip_timm", "visual.head.proj.weight"


def hf(version=5):
    arch, canon = _canon(5, ln_eps=1e-12)
    if version == 5:
        p = "layers.{i}."
        names = {"proj": p + "attention.o_proj", "fc1": p + "mlp.fc1", "fc2": p + "mlp.fc2"}
        qkv = [p + "attention.q_proj", p + "attention.k_proj", p + "attention.v_proj"]
    else:
        p = "encoder.layer.{i}."
        names = {"proj": p + "attention.output.dense", "fc1": p + "intermediate.dense", "fc2": p + "output.dense"}
        qkv = [p + "attention.attention.query", p + "attention.attention.key", p + "attention.attention.value"]
    names.update({"ln1": p + "layernorm_before", "ln2": p + "layernorm_after", "qkv": p + "QKV"})
    sd = _rename(canon, {"patch_embed.weight": "embeddings.patch_embeddings.projection.weight",
                         "patch_embed.bias": "embeddings.patch_embeddings.projection.bias", "norm.weight": "layernorm.weight",
                         "norm.bias": "layernorm.bias"},
                 {part + s: ck + s for part, ck in names.items() for s in (".weight", ".bias")})
    for i in range(2):
        for s in (".weight", ".bias"):
            _split(sd, (p + "QKV" + s).format(i=i), [(n + s).format(i=i) for n in qkv])
    sd["embeddings.cls_token"] = canon["cls_token"].reshape(1, 1, -1)
    sd["embeddings.position_embeddings"] = canon["pos_embed"][None]
    return arch, canon, sd, "hf", (qkv[1] + ".bias").format(i=1)


def hf_clip(prefix="vision_model."):
    arch, canon = _canon(6, pre_norm=True, act="quick_gelu", ln_eps=1e-5, **({"proj_dim": 64} if prefix else {}))
    canon["patch_embed.bias"] = torch.zeros(128)                       # the tower has none: the adapter uploads zeros
    p = prefix + "encoder.layers.{i}."
    names = {"ln1": p + "layer_norm1", "qkv": p + "QKV", "proj": p + "self_attn.out_proj", "ln2": p + "layer_norm2", "fc1": p + "mlp.fc1",
             "fc2": p + "mlp.fc2"}
    sd = _rename(canon, {"patch_embed.weight": prefix + "embeddings.patch_embedding.weight", "cls_token": prefix + "embeddings.class_embedding",
                         "pos_embed": prefix + "embeddings.position_embedding.weight", "pre_norm.weight": prefix + "pre_layrnorm.weight",
                         "pre_norm.bias": prefix + "pre_layrnorm.bias", "norm.weight": prefix + "post_layernorm.weight",
                         "norm.bias": prefix + "post_layernorm.bias"},
                 {part + s: ck + s for part, ck in names.items() for s in (".weight", ".bias")})
    for i in range(2):
        for s in (".weight", ".bias"):
            _split(sd, (p + "QKV" + s).format(i=i), [(p + "self_attn." + n + s).format(i=i) for n in ("q_proj", "k_proj", "v_proj")])
    if prefix:
        sd["visual_projection.weight"] = canon["head_proj.weight"]
    return arch, canon, sd, "hf_clip", prefix + "encoder.layers.0.self_attn.v_proj.weight"


def open_clip(prefix="visual."):
    arch, canon = _canon(7, pre_norm=True, act="quick_gelu", ln_eps=1e-5, **({"proj_dim": 64} if prefix else {}))
    canon["patch_embed.bias"] = torch.zeros(128)
    p = prefix + "transformer.resblocks.{i}."
    sd = _rename(canon, {"patch_embed.weight": prefix + "conv1.weight", "cls_token": prefix + "class_embedding",
                         "pos_embed": prefix + "positional_embedding", "pre_norm.weight": prefix + "ln_pre.weight",
                         "pre_norm.bias": prefix + "ln_pre.bias", "norm.weight": prefix + "ln_post.weight", "norm.bias": prefix + "ln_post.bias"},
                 {"ln1.weight": p + "ln_1.weight", "ln1.bias": p + "ln_1.bias", "qkv.weight": p + "attn.in_proj_weight",
                  "qkv.bias": p + "attn.in_proj_bias", "proj.weight": p + "attn.out_proj.weight", "proj.bias": p + "attn.out_proj.bias",
                  "ln2.weight": p + "ln_2.weight", "ln2.bias": p + "ln_2.bias", "fc1.weight": p + "mlp.c_fc.weight",
                  "fc1.bias": p + "mlp.c_fc.bias", "fc2.weight": p + "mlp.c_proj.weight", "fc2.bias": p + "mlp.c_proj.bias"})
    if prefix:
        sd[prefix + "proj"] = canon["head_proj.weight"].t().contiguous()
    return arch, canon, sd, "open_clip", prefix + "transformer.resblocks.1.mlp.c_fc.weight"


def hf_dinov3(root="model.layer.", gated=True):
    arch, canon = _canon(8, layer_scale=True, reg_tokens=4, no_embed_class=True, rope=True, ln_eps=1e-5, **({"mlp": "swiglu"} if gated else {}))
    for i in range(2):
        canon[f"blocks.{i}.qkv.bias"][128:256] = 0.0                    # k_proj has no bias
    p = root + "{i}."
    names = {"ln1": p + "norm1", "qkv": p + "QKV", "proj": p + "attention.o_proj", "ln2": p + "norm2", "fc1": p + "FC1", "fc2": p + "mlp.down_proj"}
    block = {part + s: ck + s for part, ck in names.items() for s in (".weight", ".bias")}
    block.update({"ls1": p + "layer_scale1.lambda1", "ls2": p + "layer_scale2.lambda1"})
    sd = _rename(canon, {"patch_embed.weight": "embeddings.patch_embeddings.weight", "patch_embed.bias": "embeddings.patch_embeddings.bias",
                         "norm.weight": "norm.weight", "norm.bias": "norm.bias"}, block)
    for i in range(2):
        for s in (".weight", ".bias"):
            _split(sd, (p + "QKV" + s).format(i=i), [(p + "attention." + n + s).format(i=i) for n in ("q_proj", "k_proj", "v_proj")])
            _split(sd, (p + "FC1" + s).format(i=i), [(p + n + s).format(i=i) for n in (("mlp.gate_proj", "mlp.up_proj") if gated else ("mlp.up_proj",))])
        del sd[(p + "attention.k_proj.bias").format(i=i)]
    sd["embeddings.cls_token"] = canon["cls_token"].reshape(1, 1, -1)
    sd["embeddings.register_tokens"] = canon["reg_tokens"][None]
    sd["embeddings.mask_token"] = torch.ones(1, 1, 128)
    return arch, canon, sd, "hf_dinov3", root + "1.mlp.up_proj.bias"


def hf_dinov2(swiglu=False, registers=False):
    arch, canon = _canon(9, layer_scale=True, no_embed_class=True, **({"mlp": "swiglu"} if swiglu else {}), **({"reg_tokens": 4} if registers else {}))
    p = "encoder.layer.{i}."
    f1, f2 = ("mlp.weights_in", "mlp.weights_out") if swiglu else ("mlp.fc1", "mlp.fc2")
    names = {"ln1": p + "norm1", "qkv": p + "QKV", "proj": p + "attention.output.dense", "ln2": p + "norm2", "fc1": p + f1, "fc2": p + f2}
    block = {part + s: ck + s for part, ck in names.items() for s in (".weight", ".bias")}
    block.update({"ls1": p + "layer_scale1.lambda1", "ls2": p + "layer_scale2.lambda1"})
    sd = _rename(canon, {"patch_embed.weight": "embeddings.patch_embeddings.projection.weight",
                         "patch_embed.bias": "embeddings.patch_embeddings.projection.bias", "norm.weight": "layernorm.weight",
                         "norm.bias": "layernorm.bias"}, block)
    for i in range(2):
        for s in (".weight", ".bias"):
            _split(sd, (p + "QKV" + s).format(i=i), [(p + "attention.attention." + n + s).format(i=i) for n in ("query", "key", "value")])
    sd["embeddings.cls_token"] = canon["cls_token"].reshape(1, 1, -1)
    sd["embeddings.position_embeddings"] = torch.cat([torch.zeros(1, 128), canon["pos_embed"]], 0)[None]   # a zero class row: the fold is exact
    sd["embeddings.mask_token"] = torch.ones(1, 128)
    if registers:
        sd["embeddings.register_tokens"] = canon["reg_tokens"][None]
    return arch, canon, sd, "hf_dinov2", f"encoder.layer.0.{f2}.weight"


CASES = {"torchvision": torchvision, "torchvision-linear_1": lambda: torchvision("mlp.linear_1", "mlp.linear_2"),
         "timm": timm_plain, "timm-registers-layerscale-swiglu": timm_registers_layerscale_swiglu, "open_clip_timm": open_clip_timm,
         "hf-transformers5": lambda: hf(5), "hf-transformers4": lambda: hf(4),
         "hf_clip-vision_model": hf_clip, "hf_clip-bare": lambda: hf_clip(""), "open_clip-visual": open_clip, "open_clip-bare": lambda: open_clip(""),
         "hf_dinov3-model.layer-gated": hf_dinov3, "hf_dinov3-layer-plain": lambda: hf_dinov3("layer.", False),
         "hf_dinov2-fc": hf_dinov2, "hf_dinov2-weights_in-registers": lambda: hf_dinov2(True, True)}


def _adapt(sd, arch, source):
    from atlaspatch_amd.encoders.vit import canonical_state_dict
    return canonical_state_dict(sd, depth=arch["depth"], layer_scale=arch["layer_scale"], source=source,
                                grid=arch["image_size"] // arch["patch_size"], heads=arch["heads"])


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == torch.float32 and got[k].is_contiguous() and torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_canonical_dict_renamed_into_a_layout_comes_back(case):
    arch, canon, sd, source, needed = CASES[case]()
    assert not set(IGNORED) & set(sd)
    sd = {**sd, **IGNORED}
    _same(_adapt(sd, arch, "auto"), canon)                            # detected ...
    _same(_adapt(sd, arch, source), canon)                            # ... and named
    assert needed in sd
    with pytest.raises(KeyError, match=re.escape(needed)):
        _adapt({k: v for k, v in sd.items() if k != needed}, arch, source)


def test_dinov2_without_a_grid_keeps_the_checkpoints_rows_and_dinov3_needs_grid_and_heads():
    from atlaspatch_amd.encoders.vit import canonical_state_dict
    arch, canon, sd, _, _ = hf_dinov2()
    _same(canonical_state_dict(sd, depth=2, layer_scale=True, source="hf_dinov2"), canon)
    arch, canon, sd, _, _ = hf_dinov3()
    with pytest.raises(ValueError, match="hf_dinov3: the patch grid and the head count"):
        canonical_state_dict(sd, depth=2, layer_scale=True)
    with pytest.raises(ValueError, match="unknown state-dict source 'nope'"):
        canonical_state_dict(sd, depth=2, layer_scale=True, source="nope")
    with pytest.raises(ValueError, match="hf_siglip checkpoints go through siglip_canonical_state_dict"):
        canonical_state_dict(sd, depth=2, layer_scale=True, source="hf_siglip")


def test_canonical_keys_pass_through():
    arch, canon = _canon(10, layer_scale=True, reg_tokens=2)
    half = {k: v.to(torch.float16) for k, v in canon.items()}
    got = _adapt(half, arch, "auto")
    _same(got, {k: v.float() for k, v in half.items()})
    _same(_adapt(canon, arch, "canonical"), canon)


def test_conch_v1_split_gives_the_trunk_and_the_folded_pooler():
    """CONCH v1: ``visual.trunk.*`` is a timm ViT, ``visual.attn_pool_contrast.*`` + ``visual.ln_contrast.*`` the pooler; the seeded
    init folds the same seeded pooler tensors, so the canonical dict comes back whole."""
    from atlaspatch_amd.encoders.vit import attn_pool_canonical, conch_state_dicts, random_attn_pool
    arch, canon = _canon(11, pool="attn", pool_dim=64, pool_heads=1, pool_ln_eps=1e-5)
    pool = random_attn_pool(arch, 11)
    sd = {"visual.trunk." + k: v for k, v in _timm({k: v for k, v in canon.items() if not k.startswith("attn_pool.")}).items()}
    sd.update({"visual.attn_pool_contrast." + k: v for k, v in pool.items() if not k.startswith("ln_out.")})
    sd.update({"visual.ln_contrast.weight": pool["ln_out.weight"], "visual.ln_contrast.bias": pool["ln_out.bias"]})
    sd.update({"text.ln_final.weight": torch.ones(8), "logit_scale": torch.ones(())})
    trunk, pooler = conch_state_dicts(sd)
    got = _adapt(trunk, arch, "auto")
    got.update(attn_pool_canonical(pooler, pool_eps=1e-5))
    _same(got, canon)
    with pytest.raises(KeyError, match=re.escape("visual.ln_contrast.bias")):
        conch_state_dicts({k: v for k, v in sd.items() if k != "visual.ln_contrast.bias"})


# ----------------------------------------------------------------------------- the parameter set
def _shrunk(arch):
    small = dict(arch, depth=1, dim=8 * arch["heads"], mlp_dim=24)
    small.update({k: v for k, v in (("pool_dim", 16), ("proj_dim", 8), ("pool_proj_dim", 8)) if k in arch})
    return small


def test_canonical_shapes_is_what_the_seeded_init_draws_for_every_architecture():
    from atlaspatch_amd.encoders.vit import ARCHS
    from atlaspatch_amd.encoders.vit import canonical_shapes, random_canonical_state_dict
    flags = set()
    for name, arch in ARCHS.items():
        small = _shrunk(arch)
        drawn = {k: tuple(v.shape) for k, v in random_canonical_state_dict(small, 0).items()}
        assert drawn == canonical_shapes(small), name
        flags |= {k for k, v in arch.items() if v and k in ("no_class_token", "reg_tokens", "no_embed_class", "layer_scale", "pre_norm",
                                                             "proj_dim", "rope", "pool_proj_dim", "pool_skip_final_norm")}
        flags |= {f"{k}={arch[k]}" for k in ("mlp", "pool") if k in arch}
    assert flags == {"no_class_token", "reg_tokens", "no_embed_class", "layer_scale", "pre_norm", "proj_dim", "rope", "pool_proj_dim",
                     "pool_skip_final_norm", "mlp=swiglu", "pool=attn", "pool=map", "pool=cls_mean"}     # every flag occurs


def _blocks(depth, d, mlp, layer_scale):
    out = {}
    for i in range(depth):
        b = f"blocks.{i}."
        out.update({b + "ln1.weight": (d,), b + "ln1.bias": (d,), b + "qkv.weight": (3 * d, d), b + "qkv.bias": (3 * d,),
                    b + "proj.weight": (d, d), b + "proj.bias": (d,), b + "ln2.weight": (d,), b + "ln2.bias": (d,),
                    b + "fc1.weight": (mlp, d), b + "fc1.bias": (mlp,), b + "fc2.weight": (d, mlp), b + "fc2.bias": (d,)})
        if layer_scale:
            out.update({b + "ls1": (d,), b + "ls2": (d,)})
    return out


def test_canonical_shapes_of_the_three_pooled_towers_at_full_size():
    """Written out from ``siglip_canonical_shapes`` / ``attn_tower_canonical_shapes`` as they stood before ``canonical_shapes``
    replaced them (both names remain, as aliases)."""
    from atlaspatch_amd.encoders.vit import ARCHS, attn_tower_canonical_shapes, canonical_shapes, siglip_canonical_shapes
    d, mlp = 1152, 4304
    assert canonical_shapes(ARCHS["medsiglip"]) == siglip_canonical_shapes(ARCHS["medsiglip"]) == {
        "patch_embed.weight": (d, 3, 14, 14), "patch_embed.bias": (d,), "pos_embed": (1024, d), "norm.weight": (d,), "norm.bias": (d,),
        "map.q": (d,), "map.kv.weight": (2 * d, d), "map.kv.bias": (2 * d,), "map.out.weight": (d, d), "map.out.bias": (d,),
        "map.ln.weight": (d,), "map.ln.bias": (d,), "map.fc1.weight": (mlp, d), "map.fc1.bias": (mlp,), "map.fc2.weight": (d, mlp),
        "map.fc2.bias": (d,), **_blocks(27, d, mlp, False)}
    d, mlp, P = 1024, 4096, 768
    pooler = {"attn_pool.q": (P,), "attn_pool.ln_k.weight": (d,), "attn_pool.ln_k.bias": (d,), "attn_pool.kv.weight": (2 * P, d),
              "attn_pool.kv.bias": (2 * P,), "attn_pool.out.weight": (P, P), "attn_pool.out.bias": (P,), "attn_pool.ln_out.weight": (P,),
              "attn_pool.ln_out.bias": (P,)}
    assert canonical_shapes(ARCHS["omiclip"]) == attn_tower_canonical_shapes(ARCHS["omiclip"]) == {
        "patch_embed.weight": (d, 3, 14, 14), "patch_embed.bias": (d,), "cls_token": (d,), "pos_embed": (257, d), **pooler,
        "pre_norm.weight": (d,), "pre_norm.bias": (d,), "attn_pool.proj.weight": (768, P), **_blocks(24, d, mlp, False)}
    assert canonical_shapes(ARCHS["conch_v15"]) == attn_tower_canonical_shapes(ARCHS["conch_v15"]) == {
        "patch_embed.weight": (d, 3, 16, 16), "patch_embed.bias": (d,), "cls_token": (d,), "pos_embed": (785, d), **pooler,
        "norm.weight": (d,), "norm.bias": (d,), **_blocks(24, d, mlp, True)}


# ----------------------------------------------------------------------------- the structure handed to ap_vit_create
def _rsqrt_f32(head_dim):                                            # the softmax scale is worked out in float32
    return float(np.float32(1.0) / np.sqrt(np.float32(head_dim)))


F16 = 1                                                              # AP_DTYPE_F16 (include/atlaspatch_hip.h)
BASE = dict(layer_scale=0, compute_dtype=F16, pool=0, pool_dim=0, pool_heads=0, pool_ln_eps=1e-5, reg_tokens=0, no_embed_class=0, mlp_type=0,
            head_dim=64, attn_scale=0.0, pre_norm=0, act=0, proj_dim=0, rope=0)
CONFIGS = {
    "vit_b_16": ("VitConfig", 92, dict(BASE, image_size=224, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-6)),
    # heads 1280 / 16 = 80 wide, stored 96 wide with the true softmax scale; MLP 3416 stored as 27 x 128 = 3456; pool 2 = class | mean
    "virchow_v2": ("VitConfig", 92, dict(BASE, image_size=224, patch_size=14, dim=1280, depth=32, heads=16, mlp_dim=3456, ln_eps=1e-6,
                                         layer_scale=1, pool=2, reg_tokens=4, mlp_type=1, head_dim=96, attn_scale=_rsqrt_f32(80))),
    "clip_vit_b_32": ("VitConfig", 92, dict(BASE, image_size=224, patch_size=32, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-5,
                                            pre_norm=1, act=1, proj_dim=512)),
    "dinov3_vits16_plus": ("VitConfig", 92, dict(BASE, image_size=224, patch_size=16, dim=384, depth=12, heads=6, mlp_dim=1536, ln_eps=1e-5,
                                                 layer_scale=1, reg_tokens=4, no_embed_class=1, mlp_type=1, rope=1)),
    # heads 1152 / 16 = 72 wide -> 96; MLP 4304 -> 34 x 128 = 4352; pool 3 = SigLIP's head; act 2 = tanh GELU; the 96-byte form
    "medsiglip": ("VitConfigEx", 96, dict(BASE, image_size=448, patch_size=14, dim=1152, depth=27, heads=16, mlp_dim=4352, ln_eps=1e-6,
                                          pool=3, head_dim=96, attn_scale=_rsqrt_f32(72), act=2, no_class_token=1)),
    "omiclip": ("VitConfigEx2", 112, dict(BASE, image_size=224, patch_size=14, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-5,
                                          pool=1, pool_dim=768, pool_heads=8, pre_norm=1, no_class_token=0, pool_head_dim=96,
                                          pool_skip_final_norm=1, pool_proj_dim=768, out_normalize=1)),
    "conch_v1": ("VitConfig", 92, dict(BASE, image_size=448, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072, ln_eps=1e-6,
                                       pool=1, pool_dim=512, pool_heads=8)),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_vit_config_field_by_field(name):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.encoders.vit import ARCHS, vit_config
    kind, size, fields = CONFIGS[name]
    cfg = vit_config(ARCHS[name], torch.float16)
    assert type(cfg) is getattr(_lib, kind) and cfg.struct_size == size == C.sizeof(cfg)
    assert _lib.torch_dtype_code(torch.float16) == F16
    names = [f for klass in reversed(type(cfg).__mro__) for f, _ in klass.__dict__.get("_fields_", ())]     # base structure first
    got = {f: getattr(cfg, f) for f in names if f != "struct_size"}
    assert got.keys() == fields.keys()
    for f, want in fields.items():
        assert got[f] == (C.c_float(want).value if isinstance(want, float) else want), (f, got[f], want)


# ----------------------------------------------------------------------------- what each registered name is built with
def test_every_registered_vit_is_built_from_the_four_tables(monkeypatch):
    from atlaspatch_amd.encoders import build_default_registry, vit
    from atlaspatch_amd.encoders.checkpoints import IMAGENET_MEAN, IMAGENET_STD
    recorded = []
    monkeypatch.setattr(vit, "build_hip_vit_extractor", lambda **kw: recorded.append(kw) or kw)
    registry = build_default_registry(device="cpu", dtype=torch.float16)
    names = [n for n in registry.available() if n in vit.ARCHS]
    for n in names:
        recorded.clear()
        registry.create(n)
        (kw,) = recorded
        mean, std = vit.TRANSFORM_NORM.get(n, (IMAGENET_MEAN, IMAGENET_STD))
        assert kw["name"] == n and (vit.ARCHS[kw["arch"]] if isinstance(kw["arch"], str) else kw["arch"]) == vit.ARCHS[n]
        assert (kw["mean"], kw["std"]) == (mean, std), n
        assert kw["resize"] == vit.TRANSFORM_RESIZE[n] and kw["max_batch"] == vit.MAX_BATCH[n] and kw["expect_size"] is None, n
        assert kw["dtype"] == torch.float16 and kw.get("source", "auto") == "auto"
    assert set(vit.MAX_BATCH) == set(names) | {"medsiglip", "omiclip", "conch_v15"}
    assert set(vit.MAX_BATCH) == set(vit.ARCHS) == set(vit.TRANSFORM_RESIZE)
