"""Restatements of the two ViT-L towers behind a 96-wide attentional pooler, for tests/test_coca_cpu.py and tests/test_gpu_coca.py
(helpers, no tests).  Neither open_clip nor the TITAN repository's conch_v1_5.py is importable here, so the architectures are
restated from the published packages with the packages' key names -- UNVERIFIED OFFLINE, like ``ARCHS["conch_v1"]`` -- and
parity is claimed against THIS file:

* ``CocaVisual`` / ``CocaModel``: open_clip's ``coca_ViT-L-14`` visual tower and the ``encode_image`` around it;
* ``ConchV15``: ``build_conch(ConchConfig())``, ``model(x)``;
  both run their attention through ``torch.nn.MultiheadAttention`` / ``F.multi_head_attention_forward`` (the pooler with kdim / vdim);
* ``canonical_forward``: a second, independent forward in plain matrix products on the canonical state dict (what the engine is
  given), in any dtype -- the float64 reference of the device tests, and the one place where the four fields of
  ``ap_vit_config_ex2`` can be toggled one by one;
* ``l2_normalize_ref``: float64 reference of ``ap_l2_normalize_rows``.
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

TOL = {torch.float32: 2e-5, torch.float16: 4e-3, torch.bfloat16: 3e-2}      # tests/test_encoder_zoo.py's device-vs-reference bounds
FIELDS = ("pool_head_dim", "pool_skip_final_norm", "pool_proj_dim", "out_normalize")


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ----------------------------------------------------------------------------- open_clip AttentionalPooler
class AttentionalPooler(nn.Module):
    def __init__(self, d_model, context_dim, n_head, n_queries):
        super().__init__()
        self.query = nn.Parameter(torch.randn(n_queries, d_model))
        self.attn = nn.MultiheadAttention(d_model, n_head, kdim=context_dim, vdim=context_dim, batch_first=True)
        self.ln_q = nn.LayerNorm(d_model)
        self.ln_k = nn.LayerNorm(context_dim)

    def forward(self, x):
        x = self.ln_k(x)
        q = self.ln_q(self.query)
        return self.attn(q.unsqueeze(0).expand(x.shape[0], -1, -1), x, x, need_weights=False)[0]


# ----------------------------------------------------------------------------- open_clip VisionTransformer as CoCa builds it
class ResidualAttentionBlock(nn.Module):
    def __init__(self, width, heads, mlp):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width)
        self.attn = nn.MultiheadAttention(width, heads, batch_first=True)
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, mlp)), ("gelu", nn.GELU()), ("c_proj", nn.Linear(mlp, width))]))

    def forward(self, x):
        y = self.ln_1(x)
        x = x + self.attn(y, y, y, need_weights=False)[0]
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, width, layers, heads, mlp):
        super().__init__()
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads, mlp) for _ in range(layers)])

    def forward(self, x):
        for blk in self.resblocks:
            x = blk(x)
        return x


class CocaVisual(nn.Module):
    """ln_pre on the embedded tokens, NO LayerNorm after the last block, attn_pool over all tokens, ln_post on the pooled rows,
    row 0 = the pooled vector (rows 1 .. are CoCa's caption tokens), times ``proj`` without bias."""

    def __init__(self, *, width=1024, layers=24, heads=16, mlp=4096, image=224, patch=14, pool_dim=768, pool_heads=8, n_queries=256,
                 output_dim=768):
        super().__init__()
        tokens = 1 + (image // patch) ** 2
        self.conv1 = nn.Conv2d(3, width, patch, patch, bias=False)
        self.class_embedding = nn.Parameter(torch.randn(width))
        self.positional_embedding = nn.Parameter(torch.randn(tokens, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers, heads, mlp)
        self.attn_pool = AttentionalPooler(pool_dim, width, pool_heads, n_queries)
        self.ln_post = nn.LayerNorm(pool_dim)
        self.proj = nn.Parameter(torch.randn(pool_dim, output_dim))

    def forward(self, x):
        x = self.conv1(x).flatten(2).transpose(1, 2)
        x = torch.cat([self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1), x], 1) + self.positional_embedding.to(x.dtype)
        x = self.transformer(self.ln_pre(x))
        x = self.ln_post(self.attn_pool(x))
        return x[:, 0] @ self.proj, x[:, 1:]


class CocaModel(nn.Module):
    """The whole model as far as its state dict goes: ``visual.*`` plus stand-ins for ``text.*``, ``text_decoder.*``, ``logit_scale``."""

    def __init__(self, **kw):
        super().__init__()
        self.visual = CocaVisual(**kw)
        self.text = nn.Linear(8, 8)
        self.text_decoder = nn.Linear(8, 8)
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))

    def encode_image(self, images, normalize=True):
        pooled, _ = self.visual(images)
        return F.normalize(pooled, dim=-1) if normalize else pooled


# ----------------------------------------------------------------------------- timm ViT trunk + CONCH v1.5's head
class TimmAttention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):                      # timm's packed-qkv attention, computed by nn.MultiheadAttention's own routine
        y = x.transpose(0, 1)
        out = F.multi_head_attention_forward(y, y, y, x.shape[-1], self.heads, self.qkv.weight, self.qkv.bias, None, None, False, 0.0,
                                             self.proj.weight, self.proj.bias, training=False, need_weights=False)[0]
        return out.transpose(0, 1)


class LayerScale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class TimmMlp(nn.Module):
    def __init__(self, dim, mlp):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(dim, mlp), nn.GELU(), nn.Linear(mlp, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class TimmBlock(nn.Module):
    def __init__(self, dim, heads, mlp, layer_scale):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = TimmAttention(dim, heads)
        self.ls1 = LayerScale(dim) if layer_scale else nn.Identity()
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = TimmMlp(dim, mlp)
        self.ls2 = LayerScale(dim) if layer_scale else nn.Identity()

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class PatchEmbed(nn.Module):
    def __init__(self, dim, patch):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, patch, patch)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class TimmViT(nn.Module):
    def __init__(self, dim, depth, heads, mlp, image, patch, layer_scale):
        super().__init__()
        self.patch_embed = PatchEmbed(dim, patch)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.randn(1, 1 + (image // patch) ** 2, dim))
        self.blocks = nn.ModuleList([TimmBlock(dim, heads, mlp, layer_scale) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)

    def forward_features(self, x):
        x = self.patch_embed(x)
        x = torch.cat([self.cls_token.to(x.dtype).expand(x.shape[0], -1, -1), x], 1) + self.pos_embed.to(x.dtype)
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x)


class ConchV15(nn.Module):
    """trunk.forward_features (final norm on all tokens) -> attn_pool_contrast (one query) -> ln_contrast; no projection."""

    def __init__(self, *, width=1024, layers=24, heads=16, mlp=4096, image=448, patch=16, pool_dim=768, pool_heads=8, layer_scale=True):
        super().__init__()
        self.trunk = TimmViT(width, layers, heads, mlp, image, patch, layer_scale)
        self.attn_pool_contrast = AttentionalPooler(pool_dim, width, pool_heads, 1)
        self.ln_contrast = nn.LayerNorm(pool_dim)

    def forward(self, x):
        return self.ln_contrast(self.attn_pool_contrast(self.trunk.forward_features(x))[:, 0])


# ----------------------------------------------------------------------------- seeded weights
def seed_module(model, seed):
    """Weights with which every part of the network shows in the output (tests/test_coca_cpu.py asserts it for the four new
    fields): matrices at 1 / sqrt(fan-in) so that activations stay O(1) and the pooler's scores spread over about +-2; LayerNorm
    gains between 0.4 and 1.8 with biases of 0.3 (a skipped or doubled LayerNorm is a large change); LayerScale around 0.5."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if leaf == "weight" and p.dim() == 1:                    # every LayerNorm gain
                p.copy_(0.4 + 1.4 * torch.rand(p.shape, generator=g))
            elif leaf == "gamma":                                    # LayerScale
                p.copy_(0.3 + 0.4 * torch.rand(p.shape, generator=g))
            elif leaf == "query":
                p.copy_(torch.randn(p.shape, generator=g))
            elif leaf in ("class_embedding", "positional_embedding", "cls_token", "pos_embed") or p.dim() < 2:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)     # embeddings and biases
            else:                                                    # matrices [out, in ...]; CoCa's `proj` is [in, out]
                fan_in = p.shape[0] if name.endswith("visual.proj") or name == "proj" else p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (1.4 * fan_in ** -0.5))
    return model.eval()


def tiny_coca(seed=1, n_queries=6, **kw):
    """The CoCa form at a reduced width: dim 256, 4 heads, MLP 768, depth 2, image 28 / patch 14 = 5 tokens, pool 384 = 4 x 96."""
    cfg = dict(width=256, layers=2, heads=4, mlp=768, image=28, patch=14, pool_dim=384, pool_heads=4, n_queries=n_queries, output_dim=384)
    cfg.update(kw)
    return seed_module(CocaModel(**cfg), seed), coca_arch(cfg)


def tiny_conch(seed=2, **kw):
    """The CONCH v1.5 form: the same trunk with LayerScale, image 64 / patch 16 = 17 tokens, final norm kept, no projection."""
    cfg = dict(width=256, layers=2, heads=4, mlp=768, image=64, patch=16, pool_dim=384, pool_heads=4, layer_scale=True)
    cfg.update(kw)
    return seed_module(ConchV15(**cfg), seed), conch_arch(cfg)


def coca_arch(cfg):
    return dict(image_size=cfg["image"], patch_size=cfg["patch"], dim=cfg["width"], depth=cfg["layers"], heads=cfg["heads"],
                mlp_dim=cfg["mlp"], ln_eps=1e-5, layer_scale=False, pre_norm=True, pool="attn", pool_dim=cfg["pool_dim"],
                pool_heads=cfg["pool_heads"], pool_ln_eps=1e-5, pool_head_dim=cfg["pool_dim"] // cfg["pool_heads"],
                pool_skip_final_norm=True, pool_proj_dim=cfg["output_dim"], out_normalize=True)


def conch_arch(cfg):
    return dict(image_size=cfg["image"], patch_size=cfg["patch"], dim=cfg["width"], depth=cfg["layers"], heads=cfg["heads"],
                mlp_dim=cfg["mlp"], ln_eps=1e-6, layer_scale=bool(cfg.get("layer_scale", True)), pool="attn", pool_dim=cfg["pool_dim"],
                pool_heads=cfg["pool_heads"], pool_ln_eps=1e-5, pool_head_dim=cfg["pool_dim"] // cfg["pool_heads"])


def images(n, size, seed=3):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------- the independent forward on canonical names
def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def canonical_forward(state, x, arch, dtype=torch.float64):
    """x [n, 3, S, S] -> features, from the canonical state dict (``ap_vit_set_param`` names) and an ``ARCHS``-style dict, in plain
    matrix products in ``dtype``.  Honours every field the two towers use, the four of ``ap_vit_config_ex2`` included
    (``pool_head_dim`` 0 = 64), an optional ``head_dim`` -- H heads of that width whatever dim / H is: ``qkv.weight`` [3 H hd, D],
    ``proj.weight`` [D, H hd], scale 1 / sqrt(hd) -- and the readouts ``pool`` "attn", "cls_mean" ([class token | mean of the patch
    tokens] after the final norm) and none (the class token after the final norm)."""
    s = {k: v.to(dtype) for k, v in state.items()}
    n, S, ps, D, H = x.shape[0], arch["image_size"], arch["patch_size"], arch["dim"], arch["heads"]
    g, hd = S // ps, int(arch.get("head_dim") or D // H)
    rows = x.to(dtype).reshape(n, 3, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(n, g * g, 3 * ps * ps)
    t = rows @ s["patch_embed.weight"].reshape(D, -1).T + s["patch_embed.bias"]
    t = torch.cat([s["cls_token"].reshape(1, 1, D).expand(n, 1, D), t], 1) + s["pos_embed"]
    T = t.shape[1]
    if arch.get("pre_norm"):
        t = _ln(t, s["pre_norm.weight"], s["pre_norm.bias"], arch["ln_eps"])
    for i in range(arch["depth"]):
        b = f"blocks.{i}."
        y = _ln(t, s[b + "ln1.weight"], s[b + "ln1.bias"], arch["ln_eps"])
        q, k, v = (y @ s[b + "qkv.weight"].T + s[b + "qkv.bias"]).reshape(n, T, 3, H, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1) @ v
        o = a.permute(0, 2, 1, 3).reshape(n, T, H * hd) @ s[b + "proj.weight"].T + s[b + "proj.bias"]
        t = t + (o * s[b + "ls1"] if arch.get("layer_scale") else o)
        y = _ln(t, s[b + "ln2.weight"], s[b + "ln2.bias"], arch["ln_eps"])
        h = y @ s[b + "fc1.weight"].T + s[b + "fc1.bias"]
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        o = h @ s[b + "fc2.weight"].T + s[b + "fc2.bias"]
        t = t + (o * s[b + "ls2"] if arch.get("layer_scale") else o)
    if not arch.get("pool_skip_final_norm"):
        t = _ln(t, s["norm.weight"], s["norm.bias"], arch["ln_eps"])
    if arch.get("pool") == "cls_mean":
        return torch.cat([t[:, 0], t[:, 1:].mean(1)], -1)
    if arch.get("pool") != "attn":
        return t[:, 0]
    P, ph = arch["pool_dim"], arch["pool_heads"]
    pw = arch.get("pool_head_dim") or 64
    assert P == ph * pw
    xk = _ln(t, s["attn_pool.ln_k.weight"], s["attn_pool.ln_k.bias"], arch["pool_ln_eps"])
    kv = xk @ s["attn_pool.kv.weight"].T + s["attn_pool.kv.bias"]
    k, v = kv[..., :P].reshape(n, T, ph, pw), kv[..., P:].reshape(n, T, ph, pw)
    sc = torch.einsum("hd,nthd->nht", s["attn_pool.q"].reshape(ph, pw), k) / math.sqrt(pw)
    pooled = torch.einsum("nht,nthd->nhd", torch.softmax(sc, -1), v).reshape(n, P)
    o = _ln(pooled @ s["attn_pool.out.weight"].T + s["attn_pool.out.bias"], s["attn_pool.ln_out.weight"], s["attn_pool.ln_out.bias"],
            arch["pool_ln_eps"])
    if arch.get("pool_proj_dim"):
        o = o @ s["attn_pool.proj.weight"].T
    if arch.get("out_normalize"):
        o = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return o


def toggled(arch, field):
    """``arch`` with one of the four new fields switched: the head width regrouped (same pool_dim, other head count), the final
    LayerNorm skipped / kept, the projection dropped / added (square, so the output width stays), the normalisation flipped."""
    a = dict(arch)
    if field == "pool_head_dim":
        a["pool_head_dim"] = {96: 64, 64: 128, 128: 96}[arch.get("pool_head_dim") or 64]
        a["pool_heads"] = arch["pool_dim"] // a["pool_head_dim"]
    elif field == "pool_skip_final_norm":
        a[field] = not arch.get(field)
    elif field == "pool_proj_dim":
        a[field] = 0 if arch.get(field) else arch["pool_dim"]
    else:
        a[field] = not arch.get(field)
    return a


def full_state(arch, seed):
    """A canonical state dict that holds EVERY optional tensor (norm.*, attn_pool.proj.weight, ...), seeded like ``seed_module``, so
    that any toggle of the four fields finds its parameters; ``select`` cuts it down to what one configuration uploads.  With
    ``head_dim`` the attention is heads x head_dim wide; without ``pool_dim`` there are no ``attn_pool.*`` tensors."""
    g = torch.Generator().manual_seed(seed)
    d, mlp, ps, P = arch["dim"], arch["mlp_dim"], arch["patch_size"], arch.get("pool_dim")
    da = arch["heads"] * int(arch.get("head_dim") or d // arch["heads"])
    tokens = 1 + (arch["image_size"] // ps) ** 2
    mat = lambda r, c: torch.randn(r, c, generator=g) * (1.4 * c ** -0.5)
    vec = lambda k: torch.randn(k, generator=g) * 0.3
    gain = lambda k: 0.4 + 1.4 * torch.rand(k, generator=g)
    s = {"patch_embed.weight": mat(d, 3 * ps * ps).reshape(d, 3, ps, ps), "patch_embed.bias": vec(d), "cls_token": vec(d),
         "pos_embed": torch.randn(tokens, d, generator=g) * 0.3, "norm.weight": gain(d), "norm.bias": vec(d),
         "pre_norm.weight": gain(d), "pre_norm.bias": vec(d)}
    for i in range(arch["depth"]):
        b = f"blocks.{i}."
        s.update({b + "ln1.weight": gain(d), b + "ln1.bias": vec(d), b + "qkv.weight": mat(3 * da, d), b + "qkv.bias": vec(3 * da),
                  b + "proj.weight": mat(d, da), b + "proj.bias": vec(d), b + "ln2.weight": gain(d), b + "ln2.bias": vec(d),
                  b + "fc1.weight": mat(mlp, d), b + "fc1.bias": vec(mlp), b + "fc2.weight": mat(d, mlp), b + "fc2.bias": vec(d),
                  b + "ls1": 0.3 + 0.4 * torch.rand(d, generator=g), b + "ls2": 0.3 + 0.4 * torch.rand(d, generator=g)})
    if not P:
        return s
    s.update({"attn_pool.q": torch.randn(P, generator=g) * 5.0, "attn_pool.ln_k.weight": gain(d), "attn_pool.ln_k.bias": vec(d),
              "attn_pool.kv.weight": mat(2 * P, d), "attn_pool.kv.bias": vec(2 * P), "attn_pool.out.weight": mat(P, P),
              "attn_pool.out.bias": vec(P), "attn_pool.ln_out.weight": gain(P), "attn_pool.ln_out.bias": vec(P),
              "attn_pool.proj.weight": mat(P, P)})
    return s


def select(state, arch):
    """The tensors of ``state`` that the configuration ``arch`` uploads (``attn_tower_canonical_shapes``)."""
    from atlaspatch_amd.encoders.vit import attn_tower_canonical_shapes
    want = attn_tower_canonical_shapes(arch)
    assert all(tuple(state[k].shape) == shape for k, shape in want.items())
    return {k: state[k] for k in want}


# ----------------------------------------------------------------------------- ap_l2_normalize_rows
L2_ROWS, L2_DIMS = (1, 3, 257), (4, 128, 768, 1000)


def l2_normalize_ref(x, eps):
    """float64: x / max(||x||, eps) per row (torch F.normalize)."""
    x = x.double()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)
