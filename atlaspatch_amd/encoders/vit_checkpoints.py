"""From a ViT checkpoint, or a seed, to the canonical state dict of ``ap_vit_set_param`` (QKV is packed ``[q; k; v]``
rows): layout detection, one table per checkpoint layout and the mapper that walks them, ``canonical_shapes`` (the canonical
parameter set of an architecture), the position-grid and rotary helpers, the pooler folds, the head / MLP padding the device
stores, and the seeded random init.  ``to_canonical`` is the one road from a checkpoint to canonical names."""
from __future__ import annotations

import re
from typing import Optional

import torch

from .checkpoints import check_canonical


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


# ----------------------------------------------------------------------------- layouts
# One table per checkpoint layout, canonical name -> where it is in the checkpoint: a key, a tuple of keys to stack on axis 0
# (q | k | v, gate | up), or a callable on the ``_Reader`` for the few real transforms (None = leave the name out; under a tuple of
# canonical names, as many tensors).  ``top`` / ``block`` / ``layer_scale`` / ``head``: outside the blocks, per block (names under
# ``blocks.<i>.``), the per-block entries of a model with LayerScale, after the blocks.  ``prefix`` / ``block_prefix`` go in front
# of every key / of the per-block keys; ``{i}`` is the block index.  ``alts``, the alternatives inside a layout: [(probe,
# placeholders if the checkpoint has the probe key, placeholders if not)]; a probe ending in "." asks for any key under it, one
# with ``{i}`` is asked per block.  ``trunk``: (prefix, layout) -- the keys under the prefix are a checkpoint of that layout.
# The strict layouts (``family``) also say what to leave out (``drop``: prefixes and whole keys), which prefix to strip (the
# first of ``roots`` under which ``anchor`` occurs), their open_clip AttentionalPooler (``pooler``: prefix, closing LayerNorm)
# and the key whose presence says the checkpoint has LayerScale (``layer_scale_if``).
def _wb(**mods) -> dict:
    """canonical module = checkpoint module(s), written out as the ``.weight`` and ``.bias`` entries."""
    return {name + s: (tuple(m + s for m in mod) if isinstance(mod, tuple) else mod + s)
            for name, mod in mods.items() for s in (".weight", ".bias")}


_flat = lambda key: lambda r: r[key].reshape(-1)                       # timm / torchvision / HF tokens: [1, 1, D] -> [D]
_row0 = lambda key: lambda r: r[key][0]                                # ... and their leading batch axis: [1, N, D] -> [N, D]
_row0_if_there = lambda key: lambda r: r[key][0] if key in r else None    # register tokens [1, R, D], when the model has any
_zeros_like = lambda key: lambda r: torch.zeros(r[key].shape[0])       # the CLIP towers' patch embedding has no bias


def _dinov3_rope(r):
    if r.grid is None or r.heads is None:
        raise ValueError("hf_dinov3: the patch grid and the head count are needed for the rotary tables")
    return dinov3_rope_tables(int(r.grid), r["embeddings.cls_token"].shape[-1] // int(r.heads), r.rope_theta)


def _dinov3_qkv_bias(r):                                              # k_proj has no bias
    zeros = torch.zeros(r.sd["embeddings.cls_token"].shape[-1])
    return torch.cat([r[k] if k in r else zeros for k in ("attention.q_proj.bias", "attention.k_proj.bias", "attention.v_proj.bias")], 0)


def _dinov3_fc1(suffix):                                              # plain, or gated: silu(gate) * up = the packed SwiGLU [gate; up]
    def entry(r):
        if "mlp.gate_proj.weight" in r:
            return torch.cat([r["mlp.gate_proj" + suffix], r["mlp.up_proj" + suffix]], 0)
        return r["mlp.up_proj" + suffix]
    return entry


def _dinov2_pos(r):                                                   # the patch rows, resampled to the input's grid when it is known
    pos = r["embeddings.position_embeddings"][0][1:]
    return pos if r.grid is None else resample_position_grid(pos, int(r.grid))


def _siglip_probe(r):
    """(map.q, map.kv.weight, map.kv.bias): ``map.q`` = W_q probe + b_q, the query third of ``head.attention.in_proj`` applied to
    the probe (input independent; float64 on the host, as for CONCH's pooler)."""
    d = r.arch["dim"]
    probe, w_in, b_in = r["head.probe"], r["head.attention.in_proj_weight"], r["head.attention.in_proj_bias"]
    if w_in is None or b_in is None:
        return None, None, None
    if probe is not None and tuple(w_in.shape) == (3 * d, d) and tuple(b_in.shape) == (3 * d,) and probe.numel() == d:
        f = lambda t: t.detach().to(torch.float64, copy=True).cpu()
        return f(w_in)[:d] @ f(probe).reshape(d) + f(b_in)[:d], w_in[d:], b_in[d:]
    return None, w_in, b_in                                            # wrong shapes: check_canonical names them


_LAMBDA1 = {"ls1": "layer_scale1.lambda1", "ls2": "layer_scale2.lambda1"}
_HF_QKV = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")

LAYOUTS = {
    "torchvision": dict(
        block_prefix="encoder.layers.encoder_layer_{i}.",
        alts=[("encoder.layers.encoder_layer_{i}.mlp.0.weight", {"f1": "mlp.0"}, {"f1": "mlp.linear_1"}),
              ("encoder.layers.encoder_layer_{i}.mlp.3.weight", {"f2": "mlp.3"}, {"f2": "mlp.linear_2"})],
        top={**_wb(patch_embed="conv_proj"), "cls_token": _flat("class_token"), "pos_embed": _row0("encoder.pos_embedding"),
             **_wb(norm="encoder.ln")},
        block={**_wb(ln1="ln_1"), "qkv.weight": "self_attention.in_proj_weight", "qkv.bias": "self_attention.in_proj_bias",
               **_wb(proj="self_attention.out_proj", ln2="ln_2", fc1="{f1}", fc2="{f2}")}),
    "timm": dict(
        block_prefix="blocks.{i}.",
        top={**_wb(patch_embed="patch_embed.proj"), "cls_token": _flat("cls_token"), "pos_embed": _row0("pos_embed"),
             "reg_tokens": _row0_if_there("reg_token"), **_wb(norm="norm")},
        block=_wb(ln1="norm1", qkv="attn.qkv", proj="attn.proj", ln2="norm2", fc1="mlp.fc1", fc2="mlp.fc2"),
        layer_scale={"ls1": "ls1.gamma", "ls2": "ls2.gamma"}),
    # open_clip TimmModel (biomedclip.py:40: hf-hub:microsoft/BiomedCLIP-...-vit_base_patch16_224): visual.trunk = a timm ViT
    # (class-token pooling), visual.head.proj = the bias-free linear projection [embed_dim, width] [3P, unverified offline]
    "open_clip_timm": dict(trunk=("visual.trunk.", "timm"), top={"head_proj.weight": "visual.head.proj.weight"}),
    # transformers ViTModel: the key names of transformers >= 5 and of 4.x
    "hf": dict(
        block_prefix="{p}{i}.",
        alts=[("layers.{i}.layernorm_before.weight",
               dict(p="layers.", q="attention.q_proj", k="attention.k_proj", v="attention.v_proj", o="attention.o_proj",
                    f1="mlp.fc1", f2="mlp.fc2"),
               dict(p="encoder.layer.", q="attention.attention.query", k="attention.attention.key", v="attention.attention.value",
                    o="attention.output.dense", f1="intermediate.dense", f2="output.dense"))],
        top={**_wb(patch_embed="embeddings.patch_embeddings.projection"), "cls_token": _flat("embeddings.cls_token"),
             "pos_embed": _row0("embeddings.position_embeddings"), **_wb(norm="layernorm")},
        block=_wb(ln1="layernorm_before", qkv=("{q}", "{k}", "{v}"), proj="{o}", ln2="layernorm_after", fc1="{f1}", fc2="{f2}")),
    # transformers CLIPModel / CLIPVisionModelWithProjection (plip.py:34, quilt.py: CLIPModel.from_pretrained): the vision
    # tower + visual_projection.  No patch-embedding bias; class_embedding + position_embedding rows; pre_layrnorm (sic)
    "hf_clip": dict(
        prefix="{v}", block_prefix="encoder.layers.{i}.",
        alts=[("vision_model.pre_layrnorm.weight", {"v": "vision_model."}, {"v": ""})],
        top={"patch_embed.weight": "embeddings.patch_embedding.weight", "patch_embed.bias": _zeros_like("embeddings.class_embedding"),
             "cls_token": _flat("embeddings.class_embedding"), "pos_embed": "embeddings.position_embedding.weight",
             **_wb(pre_norm="pre_layrnorm", norm="post_layernorm"), "head_proj.weight": lambda r: r.sd.get("visual_projection.weight")},
        block=_wb(ln1="layer_norm1", qkv=_HF_QKV, proj="self_attn.out_proj", ln2="layer_norm2", fc1="mlp.fc1", fc2="mlp.fc2")),
    # open_clip VisionTransformer (clip.py:38-40, the OpenAI checkpoints; key names of the public package [3P], unverified
    # offline): visual.conv1 (no bias), class_embedding, positional_embedding, ln_pre, transformer.resblocks.<i>.{ln_1,
    # attn.in_proj_weight | in_proj_bias | out_proj, ln_2, mlp.c_fc, mlp.c_proj}, ln_post, proj [width, output_dim]
    "open_clip": dict(
        prefix="{v}", block_prefix="transformer.resblocks.{i}.",
        alts=[("visual.ln_pre.weight", {"v": "visual."}, {"v": ""})],
        top={"patch_embed.weight": "conv1.weight", "patch_embed.bias": _zeros_like("class_embedding"), "cls_token": _flat("class_embedding"),
             "pos_embed": "positional_embedding", **_wb(pre_norm="ln_pre", norm="ln_post"),
             "head_proj.weight": lambda r: r["proj"].t() if "proj" in r else None},
        block={**_wb(ln1="ln_1"), "qkv.weight": "attn.in_proj_weight", "qkv.bias": "attn.in_proj_bias",
               **_wb(proj="attn.out_proj", ln2="ln_2", fc1="mlp.c_fc", fc2="mlp.c_proj")}),
    # transformers DINOv3ViTModel (dinov3.py:52-67): class + register tokens, NO position embedding (zeros here; the rotary
    # tables rope.cos | rope.sin carry the positions), k_proj without bias, LayerScale, plain or gated MLP, LayerNorm 1e-5,
    # pooler_output = final LayerNorm of the class token.  Blocks: `model.layer.<i>.` in memory (transformers 5), `layer.<i>.`
    # in the published model.safetensors
    "hf_dinov3": dict(
        block_prefix="{root}{i}.",
        alts=[("model.layer.", {"root": "model.layer."}, {"root": "layer."})],
        top={("rope.cos", "rope.sin"): _dinov3_rope, **_wb(patch_embed="embeddings.patch_embeddings"),
             "cls_token": _flat("embeddings.cls_token"),
             "reg_tokens": lambda r: r["embeddings.register_tokens"][0] if r["embeddings.register_tokens"].shape[1] > 0 else None,
             "pos_embed": lambda r: torch.zeros(int(r.grid) * int(r.grid), r["embeddings.cls_token"].shape[-1]), **_wb(norm="norm")},
        block={**_wb(ln1="norm1"), "qkv.weight": ("attention.q_proj.weight", "attention.k_proj.weight", "attention.v_proj.weight"),
               "qkv.bias": _dinov3_qkv_bias, **_wb(proj="attention.o_proj", ln2="norm2"),
               "fc1.weight": _dinov3_fc1(".weight"), "fc1.bias": _dinov3_fc1(".bias"), **_wb(fc2="mlp.down_proj")},
        layer_scale=_LAMBDA1),
    # transformers Dinov2Model / Dinov2WithRegistersModel: the position embedding has a class row and patch rows but none
    # for the register tokens, which are inserted AFTER it is added -> canonical no_embed_class form with the class row
    # folded into the class token (one f32 add, the same one the model performs); the patch rows resampled to the input's grid
    "hf_dinov2": dict(
        block_prefix="encoder.layer.{i}.",
        alts=[("encoder.layer.{i}.mlp.weights_in.weight", dict(f1="mlp.weights_in", f2="mlp.weights_out"), dict(f1="mlp.fc1", f2="mlp.fc2"))],
        top={**_wb(patch_embed="embeddings.patch_embeddings.projection"),
             "cls_token": lambda r: r["embeddings.cls_token"].reshape(-1).float() + r["embeddings.position_embeddings"][0][0].float(),
             "reg_tokens": _row0_if_there("embeddings.register_tokens"),
             "pos_embed": _dinov2_pos, **_wb(norm="layernorm")},
        block=_wb(ln1="norm1", qkv=("attention.attention.query", "attention.attention.key", "attention.attention.value"),
                  proj="attention.output.dense", ln2="norm2", fc1="{f1}", fc2="{f2}"),
        layer_scale=_LAMBDA1),
    # transformers' SigLIP vision tower, in the three layouts that occur: ``SiglipVisionModel.state_dict()`` of transformers 5 (bare
    # keys), the same prefixed ``vision_model.`` (older versions and the published ``model.safetensors``), and a whole
    # ``SiglipModel`` checkpoint, whose ``text_model.*``, ``logit_scale`` and ``logit_bias`` are dropped
    "hf_siglip": dict(
        family="SigLIP", drop=("text_model.", "logit_scale", "logit_bias"), roots=("vision_model.",),
        block_prefix="encoder.layers.{i}.",
        top={**_wb(patch_embed="embeddings.patch_embedding"), "pos_embed": "embeddings.position_embedding.weight",
             **_wb(norm="post_layernorm")},
        block=_wb(ln1="layer_norm1", qkv=_HF_QKV, proj="self_attn.out_proj", ln2="layer_norm2", fc1="mlp.fc1", fc2="mlp.fc2"),
        head={("map.q", "map.kv.weight", "map.kv.bias"): _siglip_probe,
              **_wb(**{"map.out": "head.attention.out_proj", "map.ln": "head.layernorm", "map.fc1": "head.mlp.fc1",
                       "map.fc2": "head.mlp.fc2"})}),
}
# open_clip's CoCa visual tower (``coca_ViT-L-14``; key names from the public package [3P], unverified offline): ``visual.*`` bare
# or prefixed, or the whole CoCa model, whose ``text.*``, ``text_decoder.*`` and ``logit_scale`` are dropped.  ``conv1`` has no bias
# (zeros are uploaded, as for the CLIP towers); no LayerNorm after the last block; ``ln_post`` closes the pooler, whose query row 0
# is folded in float64 and whose ``proj`` is stored transposed as ``attn_pool.proj.weight`` (``attn_pool_canonical``)
LAYOUTS["open_clip_coca"] = dict(
    family="CoCa", drop=("text.", "text_decoder.", "logit_scale"), roots=("visual.",),
    block_prefix="transformer.resblocks.{i}.",
    top={"patch_embed.weight": "conv1.weight", "patch_embed.bias": lambda r: torch.zeros(r.arch["dim"]), "cls_token": "class_embedding",
         "pos_embed": "positional_embedding", **_wb(pre_norm="ln_pre")},
    block=LAYOUTS["open_clip"]["block"], pooler=("attn_pool.", "ln_post"))
# CONCH v1.5 (``conch_v1_5.py`` of the TITAN repository; key names from the public package [3P], unverified offline): ``trunk.*``
# (timm ViT-L/16), ``attn_pool_contrast.*`` and ``ln_contrast.*``, bare or under ``visual.`` / ``vision_encoder.``
LAYOUTS["conch_v15"] = dict(
    family="CONCH v1.5", roots=("visual.", "vision_encoder.", ""), anchor="trunk.", layer_scale_if="trunk.blocks.0.ls1.gamma",
    prefix="trunk.", block_prefix="blocks.{i}.",
    top={**_wb(patch_embed="patch_embed.proj"), "cls_token": lambda r: None if r["cls_token"] is None else r["cls_token"].reshape(-1),
         "pos_embed": lambda r: r["pos_embed"][0] if "pos_embed" in r and r["pos_embed"].dim() == 3 else r["pos_embed"], **_wb(norm="norm")},
    block=LAYOUTS["timm"]["block"], layer_scale=LAYOUTS["timm"]["layer_scale"], pooler=("attn_pool_contrast.", "ln_contrast"))


class _Reader:
    """What a table entry sees of a checkpoint.  ``r[key]`` fills the placeholders and the block index into ``key``, puts the
    prefix of the table being walked in front and fetches the tensor.  Lenient: a missing key is the ``KeyError`` of indexing.
    Strict: it is None, and every key asked for is remembered for the error message.  ``key in r`` asks without fetching.
    ``arch`` (strict) and ``grid`` / ``heads`` / ``rope_theta`` (lenient) are what the caller knows of the model."""

    def __init__(self, sd: dict, family: Optional[str] = None, **known) -> None:
        self.sd, self.family, self.used, self.fill, self.prefix = sd, family, set(), {}, ""
        self.__dict__.update(known)

    def key(self, key: str) -> str:
        return self.prefix + (key.format(**self.fill) if "{" in key else key)

    def take(self, key: str):
        if not self.family:
            return self.sd[key]
        self.used.add(key)
        return self.sd.get(key)

    def __getitem__(self, key: str):
        return self.take(self.key(key))

    def __contains__(self, key: str) -> bool:
        return self.key(key) in self.sd

    def choose(self, alts, i: Optional[int] = None) -> None:
        for probe, there, absent in alts:
            if ("{i}" in probe) == (i is not None):
                probe = probe.format(i=i)
                has = any(k.startswith(probe) for k in self.sd) if probe.endswith(".") else probe in self.sd
                self.fill.update(there if has else absent)

    def resolve(self, entry):
        if isinstance(entry, str):
            return self[entry]
        if callable(entry):
            return entry(self)
        parts = [self[k] for k in entry]
        if any(p is None for p in parts):
            return None
        if self.family and any(p.shape[1:] != parts[0].shape[1:] for p in parts):
            raise ValueError(f"{self.family} checkpoint: {[self.key(k) for k in entry]} have shapes "
                             f"{[tuple(p.shape) for p in parts]}, which do not stack")
        return torch.cat(parts, 0)


def _f32(tensor: torch.Tensor) -> torch.Tensor:
    return tensor.detach().to(dtype=torch.float32, device="cpu").contiguous()


def _map_layout(r: _Reader, layout: dict, depth: int, layer_scale: bool) -> dict:
    """Walk ``layout``'s tables over the reader's checkpoint: ``{canonical name: float32 CPU tensor}``."""
    out: dict[str, torch.Tensor] = {}

    def walk(table, prefix, under=""):
        r.prefix = prefix.format(**r.fill)
        for name, entry in table.items():
            got = r.resolve(entry)
            for n, t in zip(name, got) if isinstance(name, tuple) else ((name, got),):
                if t is not None:
                    out[under + n] = _f32(t)

    alts, root = layout.get("alts", ()), layout.get("prefix", "")
    block = {**layout.get("block", {}), **(layout.get("layer_scale", {}) if layer_scale else {})}
    r.choose(alts)
    walk(layout["top"], root)
    for i in range(depth):
        r.fill["i"] = i
        r.choose(alts, i)
        walk(block, root + layout["block_prefix"], f"blocks.{i}.")
    walk(layout.get("head", {}), root)
    return out


def canonical_state_dict(sd: dict, *, depth: int, layer_scale: bool, source: str = "auto", grid: Optional[int] = None,
                         heads: Optional[int] = None, rope_theta: float = 100.0) -> dict:
    """Return ``{canonical name: float32 CPU tensor}`` for ``ap_vit_set_param`` from one of the lenient layouts (torchvision,
    timm, open_clip_timm, hf, hf_clip, open_clip, hf_dinov3, hf_dinov2, canonical): checkpoint keys that nothing reads are
    ignored, a key the layout needs is the ``KeyError`` of indexing, and there is no shape check (no architecture here).
    ``grid``: patches per side of the input the encoder will see; an HF DINOv2 checkpoint trained on another grid has its
    position rows resampled to it (as the model itself does in every forward)."""
    if source == "auto":
        source = _detect_source(sd)
    if source == "canonical":
        return {k: _f32(v) for k, v in sd.items()}
    if source == "hf_siglip":
        raise ValueError("hf_siglip checkpoints go through siglip_canonical_state_dict (it needs the architecture for its checks)")
    layout = LAYOUTS.get(source)
    if layout is None or "family" in layout:
        raise ValueError(f"unknown state-dict source '{source}'")
    out: dict[str, torch.Tensor] = {}
    if "trunk" in layout:
        prefix, inner = layout["trunk"]
        out = canonical_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, depth=depth,
                                   layer_scale=layer_scale, source=inner, grid=grid)
        depth = 0                                                      # the blocks are the trunk's
    out.update(_map_layout(_Reader(sd, grid=grid, heads=heads, rope_theta=rope_theta), layout, depth, layer_scale))
    return out


def canonical_shapes(arch: dict) -> dict:
    """Canonical key -> shape BEFORE head / MLP padding of any ``ARCHS``-style dict: the parameter set ``random_canonical_state_dict``
    draws and the strict adapters check a checkpoint against."""
    d, mlp, ps, pool = arch["dim"], arch["mlp_dim"], arch["patch_size"], arch.get("pool")
    hd = int(arch.get("head_dim") or d // arch["heads"])                # "head_dim": heads narrower than dim / heads (da < d)
    da = arch["heads"] * hd
    reg, patches = int(arch.get("reg_tokens", 0)), (arch["image_size"] // ps) ** 2
    rows = patches if (arch.get("no_embed_class") or arch.get("no_class_token")) else 1 + reg + patches
    f1 = 2 * mlp if arch.get("mlp") == "swiglu" else mlp
    want = {"patch_embed.weight": (d, 3, ps, ps), "patch_embed.bias": (d,)}
    if not arch.get("no_class_token"):
        want["cls_token"] = (d,)
    want["pos_embed"] = (rows, d)
    if pool == "attn":
        P = arch["pool_dim"]
        want.update({"attn_pool.q": (P,), "attn_pool.ln_k.weight": (d,), "attn_pool.ln_k.bias": (d,), "attn_pool.kv.weight": (2 * P, d),
                     "attn_pool.kv.bias": (2 * P,), "attn_pool.out.weight": (P, P), "attn_pool.out.bias": (P,),
                     "attn_pool.ln_out.weight": (P,), "attn_pool.ln_out.bias": (P,)})
    if not arch.get("pool_skip_final_norm"):
        want.update({"norm.weight": (d,), "norm.bias": (d,)})
    if pool == "map":
        want.update({"map.q": (da,), "map.kv.weight": (2 * da, d), "map.kv.bias": (2 * da,), "map.out.weight": (d, da), "map.out.bias": (d,),
                     "map.ln.weight": (d,), "map.ln.bias": (d,), "map.fc1.weight": (mlp, d), "map.fc1.bias": (mlp,),
                     "map.fc2.weight": (d, mlp), "map.fc2.bias": (d,)})
    if arch.get("pre_norm"):
        want.update({"pre_norm.weight": (d,), "pre_norm.bias": (d,)})
    if pool == "attn" and arch.get("pool_proj_dim"):
        want["attn_pool.proj.weight"] = (arch["pool_proj_dim"], arch["pool_dim"])
    if reg:
        want["reg_tokens"] = (reg, d)
    if arch.get("proj_dim"):
        want["head_proj.weight"] = (arch["proj_dim"], d)
    if arch.get("rope"):
        want.update({"rope.cos": (patches, hd), "rope.sin": (patches, hd)})
    for i in range(arch["depth"]):
        b = f"blocks.{i}."
        want.update({b + "ln1.weight": (d,), b + "ln1.bias": (d,), b + "qkv.weight": (3 * da, d), b + "qkv.bias": (3 * da,),
                     b + "proj.weight": (d, da), b + "proj.bias": (d,), b + "ln2.weight": (d,), b + "ln2.bias": (d,),
                     b + "fc1.weight": (f1, d), b + "fc1.bias": (f1,), b + "fc2.weight": (d, mlp), b + "fc2.bias": (d,)})
        if arch.get("layer_scale"):
            want.update({b + "ls1": (d,), b + "ls2": (d,)})
    return want


siglip_canonical_shapes = attn_tower_canonical_shapes = canonical_shapes


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

def _fold_pooler(r: _Reader, pool_prefix: str, ln_out: str, arch: dict) -> dict:
    """The AttentionalPooler under ``pool_prefix`` with ``ln_out`` as its closing LayerNorm -> ``attn_pool.*``; what the float64
    fold of ``attn_pool_canonical`` multiplies must fit first.  A pooler with a key missing gives nothing."""
    pool = {k: r.take(pool_prefix + k) for k in POOLER_KEYS}
    pool["ln_out.weight"], pool["ln_out.bias"] = r.take(ln_out + ".weight"), r.take(ln_out + ".bias")
    if arch.get("pool_proj_dim"):
        pool["proj"] = r.take("proj")
    P, d = arch["pool_dim"], arch["dim"]
    shapes = {"query": None, "ln_q.weight": (P,), "ln_q.bias": (P,), "ln_k.weight": (d,), "ln_k.bias": (d,),
              "attn.q_proj_weight": (P, P), "attn.k_proj_weight": (P, d), "attn.v_proj_weight": (P, d), "attn.in_proj_bias": (3 * P,),
              "attn.out_proj.weight": (P, P), "attn.out_proj.bias": (P,), "ln_out.weight": (P,), "ln_out.bias": (P,),
              "proj": (P, arch.get("pool_proj_dim") or 0)}
    for k, t in pool.items():
        want = shapes[k]
        if t is not None and (tuple(t.shape) != want if want else (t.dim() != 2 or t.shape[1] != P)):
            key = {"ln_out.weight": ln_out + ".weight", "ln_out.bias": ln_out + ".bias", "proj": "proj"}.get(k, pool_prefix + k)
            raise ValueError(f"{r.family} checkpoint: {key} has shape {tuple(t.shape)}, expected {want or ('Q', P)}")
    if any(t is None for k, t in pool.items() if k != "proj"):
        return {}
    return attn_pool_canonical({k: t for k, t in pool.items() if t is not None}, pool_eps=arch.get("pool_ln_eps", 1e-5))


def _strict_canonical(sd: dict, arch: dict, source: str) -> tuple[dict, bool]:
    """A strict layout (hf_siglip, open_clip_coca, conch_v15) -> (canonical names, unpadded; layer_scale).  A checkpoint key
    nothing reads, a key the architecture needs and a wrong shape are each a ``ValueError`` naming it (``check_canonical``
    against ``canonical_shapes``)."""
    layout = LAYOUTS[source]
    src = {k: v for k, v in sd.items() if not any(k.startswith(d) if d.endswith(".") else k == d for d in layout.get("drop", ()))}
    root = next((p for p in layout["roots"] if any(k.startswith(p + layout.get("anchor", "")) for k in src)), "")
    src = {(k[len(root):] if k.startswith(root) else k): v for k, v in src.items()}
    if "layer_scale_if" in layout:
        arch = dict(arch, layer_scale=layout["layer_scale_if"] in src)
    layer_scale = bool(arch.get("layer_scale"))
    r = _Reader(src, layout["family"], arch=arch)
    out = _map_layout(r, layout, arch["depth"], layer_scale)
    if "pooler" in layout:
        out.update(_fold_pooler(r, *layout["pooler"], arch))
    unknown = sorted(k for k in src if k not in r.used)
    absent = sorted(k for k in r.used if k not in src)
    try:
        return check_canonical(out, canonical_shapes(arch), unknown, family=r.family, source=source), layer_scale
    except ValueError as exc:
        if unknown or not absent:
            raise
        raise ValueError(f"{exc}; the checkpoint lacks {absent[:5]}") from None


def siglip_canonical_state_dict(sd: dict, arch: dict) -> dict:
    """The ``hf_siglip`` adapter (see ``LAYOUTS``): canonical names, unpadded -- ``HipViT`` pads heads and MLP."""
    return _strict_canonical(sd, arch, "hf_siglip")[0]


def coca_canonical_state_dict(sd: dict, arch: dict) -> dict:
    """The ``open_clip_coca`` adapter (see ``LAYOUTS``)."""
    return _strict_canonical(sd, arch, "open_clip_coca")[0]


def conch_v15_canonical_state_dict(sd: dict, arch: dict) -> tuple[dict, bool]:
    """The ``conch_v15`` adapter (see ``LAYOUTS``) -> (canonical names, layer_scale): LayerScale is taken from the checkpoint when
    ``trunk.blocks.<i>.ls1.gamma`` is there; a checkpoint without it gives a model without it."""
    return _strict_canonical(sd, arch, "conch_v15")


def to_canonical(state_dict: dict, spec: dict, source: str = "auto") -> tuple[dict, bool]:
    """The one road from a checkpoint to (canonical state dict, layer_scale) of the architecture ``spec``.  ``source``: a lenient
    layout, "auto" (``_detect_source``; a ``pool="map"`` model also takes hf_siglip, a ``pool="attn"`` model a CONCH v1
    checkpoint or a trunk checkpoint with ``attn_pool.*`` tensors beside it), or a strict layout by name -- of which conch_v15
    reads ``layer_scale`` from the checkpoint; everywhere else it is ``spec``'s."""
    if spec.get("pool") == "map" and source == "auto" and _detect_source(state_dict) == "hf_siglip":
        source = "hf_siglip"
    if "family" in LAYOUTS.get(source, {}):
        return _strict_canonical(state_dict, spec, source)
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
        state.update({k: _f32(v) for k, v in pool_state.items()})
    return state, bool(spec.get("layer_scale"))


# ----------------------------------------------------------------------------- what the device stores
def stored_head_dim(dim: int, heads: int, head_dim: Optional[int] = None) -> int:
    """Width of one q / k / v head as the device stores it: 64, 96 or 128 (other true widths are zero-padded up; 96 -- the 80-wide
    heads of ViT-H/14 and Virchow -- exists in the float16 / bfloat16 attention kernels only, like 128).  ``head_dim``: the true
    width where it is not dim / heads (an ``ARCHS``-style dict's "head_dim")."""
    hd = int(head_dim or dim // heads)
    if hd <= 64:
        return 64
    if hd <= 96:
        return 96
    if hd <= 128:
        return 128
    raise ValueError(f"head width {hd} (dim {dim} / heads {heads}) exceeds 128")


def pad_heads(state: dict, *, dim: int, heads: int, depth: int, head_dim: Optional[int] = None) -> dict:
    """Canonical state dict -> the same model with every attention head zero-padded from dim / heads to
    ``stored_head_dim`` channels: qkv rows [3, heads, hd, :] -> [3, heads, hdp, :], proj columns likewise.  Zero q / k
    channels add nothing to q.k, zero v channels give zero outputs that meet zero proj columns: the function is unchanged
    as long as the softmax scale stays 1 / sqrt(hd) (``attn_scale``)."""
    hd, hdp = int(head_dim or dim // heads), stored_head_dim(dim, heads, head_dim)
    if hd == hdp:
        return state
    out = dict(state)

    def pad(key, view, shape):                                       # `view`: [.., heads, hd(, :)], its axis 2 zero-padded to hdp
        v = state[key].reshape(view)
        p = torch.zeros(v.shape[:2] + (hdp,) + v.shape[3:], dtype=v.dtype)
        p[:, :, :hd] = v
        out[key] = p.reshape(shape).contiguous()

    for i in range(depth):
        b = f"blocks.{i}."
        pad(b + "qkv.weight", (3, heads, hd, -1), (3 * heads * hdp, -1))
        pad(b + "qkv.bias", (3, heads, hd), (-1,))
        pad(b + "proj.weight", (-1, heads, hd), (-1, heads * hdp))
    if "map.kv.weight" in state:                                     # SigLIP's pooling head: q [heads, hd], kv rows [2, heads, hd, :], out columns
        pad("map.q", (1, heads, hd), (-1,))
        pad("map.kv.weight", (2, heads, hd, -1), (2 * heads * hdp, -1))
        pad("map.kv.bias", (2, heads, hd), (-1,))
        pad("map.out.weight", (-1, heads, hd), (-1, heads * hdp))
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

# ----------------------------------------------------------------------------- seeded init
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
