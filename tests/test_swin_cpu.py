"""CHIEF-CTransPath (Swin-Tiny with a convolutional stem), CPU side: the restatement's stem against torch.nn modules and its
stages against transformers SwinModel, the three checkpoint layouts, BatchNorm folding, the relative-position bias expansion,
the registration through the shipped plugin, and the seeded random init."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import swin_reference as ref

ARCH = "chief-ctranspath"
HEADS = (3, 6, 12, 24)


def _canonical(seed=5, arch=ARCH):
    from atlaspatch_amd.encoders.swin import random_canonical_state_dict
    return random_canonical_state_dict(arch, seed)


# ----------------------------------------------------------------------------- the restatement
def test_restatement_stem_equals_conv_batchnorm_relu_modules():
    sd = _canonical(seed=1)
    seq = nn.Sequential(nn.Conv2d(3, 12, 3, 2, 1, bias=False), nn.BatchNorm2d(12), nn.ReLU(),
                        nn.Conv2d(12, 24, 3, 2, 1, bias=False), nn.BatchNorm2d(24), nn.ReLU(), nn.Conv2d(24, 96, 1)).eval()
    seq.load_state_dict({k[len("patch_embed.proj."):]: v for k, v in sd.items() if k.startswith("patch_embed.proj.")}, strict=True)
    norm = nn.LayerNorm(96, eps=1e-5)
    norm.load_state_dict({"weight": sd["patch_embed.norm.weight"], "bias": sd["patch_embed.norm.bias"]})
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = norm(seq(x).flatten(2).transpose(1, 2))
        got = ref.stem(sd, x)
    assert got.shape == (2, 56, 56, 96)
    rel = float((got.reshape(2, -1, 96) - want).norm() / want.norm())
    assert rel <= 1e-5, rel
    assert float(sd["patch_embed.proj.1.running_var"].sub(1).abs().min()) > 0        # the BatchNorms are not the identity


def _hf_model(depths, seed=0):
    from transformers import SwinConfig, SwinModel
    torch.manual_seed(seed)
    model = SwinModel(SwinConfig(image_size=224, patch_size=4, embed_dim=96, depths=list(depths), num_heads=list(HEADS),
                                 window_size=7, layer_norm_eps=1e-5), add_pooling_layer=False).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("relative_position_bias_table"):       # O(1), not the 0.02 init: a wrong index must matter
                p.copy_(torch.randn(p.shape, generator=g))
            elif p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) / float(np.sqrt(int(np.prod(p.shape[1:])))))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(0.8 + 0.4 * torch.rand(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return model


def _stem_keys(seed=3):
    return {k: v for k, v in _canonical(seed).items() if k.startswith("patch_embed.proj.")}


@pytest.mark.parametrize("depths", [(2, 2, 6, 2), (2, 2, 2, 2)], ids=["tiny", "short"])
def test_restatement_stages_equal_transformers_swin(depths):
    from atlaspatch_amd.encoders.swin import canonical_state_dict
    model = _hf_model(depths)
    hf = {k: v for k, v in model.state_dict().items() if not k.startswith("embeddings.patch_embeddings.")}
    hf.update(_stem_keys())
    arch = {"depths": depths, "heads": HEADS, "embed_dim": 96}
    sd = canonical_state_dict(hf, arch=arch)
    emb = torch.randn(2, 56 * 56, 96, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        h = model.embeddings.norm(emb)
        want = model.layernorm(model.encoder(h, (56, 56)).last_hidden_state).mean(1)
        tokens = torch.nn.functional.layer_norm(emb, (96,), sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"], 1e-5)
        got = ref.stages(sd, tokens.view(2, 56, 56, 96), depths=depths)
    rel = float((got - want).norm() / want.norm())
    assert got.shape == want.shape == (2, 768) and rel <= 1e-5, rel


def test_restatement_uses_the_shift_and_the_mask():
    """Shift-3 blocks and the -100 mask change the features: a restatement without them would not be pinned by the test above."""
    sd = _canonical(seed=6)
    x = torch.randn(1, 14, 14, 3 * 96, generator=torch.Generator().manual_seed(0))
    bias = ref.pair_bias(sd["layers.0.blocks.1.attn.relative_position_bias_table"])
    with torch.no_grad():
        plain = ref.window_attention(x, 3, 0, bias)
        shifted = ref.window_attention(x, 3, 3, bias)
    assert float((plain - shifted).norm() / plain.norm()) > 0.1
    mask = ref.region_mask(14, 14, 3, "cpu", torch.float32)
    assert mask.shape == (4, 49, 49) and float(mask.min()) == -100.0 and float(mask.max()) == 0.0
    assert int((mask[0] != 0).sum()) == 0 and all(int((mask[i] != 0).sum()) > 0 for i in (1, 2, 3))


# ----------------------------------------------------------------------------- adapters
def _to_original_layout(canonical):
    """Current timm keys -> the original CTransPath checkpoint: downsample at the END of the previous stage, plus the buffers
    and the head the original file carries."""
    out = {}
    for k, v in canonical.items():
        f = k.split(".")
        if f[0] == "layers" and f[2] == "downsample":
            f[1] = str(int(f[1]) - 1)
        out[".".join(f)] = v
    out["layers.0.blocks.0.attn.relative_position_index"] = torch.zeros(49, 49, dtype=torch.long)
    out["layers.0.blocks.1.attn_mask"] = torch.zeros(64, 49, 49)
    out["patch_embed.proj.1.num_batches_tracked"] = torch.tensor(7)
    out["head.weight"] = torch.zeros(1000, 768)
    out["head.bias"] = torch.zeros(1000)
    return out


def _to_hf_layout(canonical):
    """Current timm keys -> transformers SwinModel keys for the stages (written independently of the adapter)."""
    names = {"norm1": "layernorm_before", "norm2": "layernorm_after", "attn.proj": "attention.o_proj"}
    out = {}
    for k, v in canonical.items():
        f = k.split(".")
        if k.startswith("patch_embed.proj."):
            out[k] = v
        elif k.startswith("patch_embed.norm."):
            out["swin.embeddings.norm." + f[-1]] = v
        elif f[0] == "norm":
            out["swin.layernorm." + f[-1]] = v
        elif f[2] == "downsample":
            out[f"swin.encoder.layers.{int(f[1]) - 1}.downsample." + ".".join(f[3:])] = v
        else:
            pre = f"swin.encoder.layers.{f[1]}.blocks.{f[3]}."
            rest = ".".join(f[4:-1])
            if rest == "attn.qkv":
                for name, part in zip(("q_proj", "k_proj", "v_proj"), v.chunk(3, 0)):
                    out[pre + f"attention.{name}.{f[-1]}"] = part.clone()
            elif f[-1] == "relative_position_bias_table":
                out[pre + "attention.relative_position_bias.relative_position_bias_table"] = v
            else:
                out[pre + names.get(rest, rest) + "." + f[-1]] = v
    out["classifier.weight"] = torch.zeros(1000, 768)
    return out


def test_the_three_checkpoint_layouts_give_the_same_canonical_dict():
    from atlaspatch_amd.encoders.swin import canonical_keys, canonical_state_dict, detect_source
    canonical = _canonical(seed=5)
    assert list(canonical) == list(canonical_keys(ARCH))
    timm = dict(canonical)
    original = _to_original_layout(canonical)
    hf = _to_hf_layout(canonical)
    assert detect_source(timm) == "timm" and detect_source(hf) == "hf"
    assert detect_source({k: v for k, v in original.items() if "attn_mask" not in k}) == "ctranspath"
    dicts = [canonical_state_dict(timm), canonical_state_dict({"model": original}), canonical_state_dict(original),
             canonical_state_dict(hf), canonical_state_dict({"model": timm})]
    for d in dicts:
        assert d.keys() == canonical.keys()
        for k in d:
            assert d[k].dtype == torch.float32 and torch.equal(d[k], canonical[k]), k


def test_adapter_refuses_unknown_missing_and_misshapen_keys():
    from atlaspatch_amd.encoders.swin import canonical_state_dict
    canonical = _canonical(seed=0)
    bad = dict(canonical)
    bad["layers.0.blocks.2.norm1.weight"] = torch.zeros(96)
    with pytest.raises(ValueError, match="unknown key"):
        canonical_state_dict(bad)
    short = dict(canonical)
    del short["layers.2.blocks.5.attn.relative_position_bias_table"]
    with pytest.raises(ValueError, match="missing key"):
        canonical_state_dict(short)
    wide = dict(canonical)
    wide["layers.1.downsample.reduction.weight"] = torch.zeros(192, 96)
    with pytest.raises(ValueError, match="shape"):
        canonical_state_dict(wide)
    hf = _to_hf_layout(canonical)
    del hf["swin.encoder.layers.1.blocks.0.attention.k_proj.weight"]
    with pytest.raises(ValueError, match="missing key"):
        canonical_state_dict(hf)
    hf = _to_hf_layout(canonical)
    hf["swin.embeddings.patch_embeddings.projection.weight"] = torch.zeros(96, 3, 4, 4)      # not this network's stem
    with pytest.raises(ValueError, match="unknown key"):
        canonical_state_dict(hf)
    with pytest.raises(ValueError, match="neither timm"):
        canonical_state_dict({"blocks.0.weight": torch.zeros(1)})


# ----------------------------------------------------------------------------- folding and expansion
def test_batchnorm_folding_matches_conv_then_batchnorm_in_fp64():
    import torch.nn.functional as F
    from atlaspatch_amd.encoders.swin import canonical_keys, fold_batchnorm
    canonical = _canonical(seed=2)
    folded = fold_batchnorm(canonical)
    assert not any("running_" in k or ".proj.1." in k or ".proj.4." in k for k in folded)
    assert set(folded) == ({k for k in canonical_keys(ARCH) if ".proj.1." not in k and ".proj.4." not in k}
                           | {"patch_embed.proj.0.bias", "patch_embed.proj.3.bias"})
    g = torch.Generator().manual_seed(0)
    for conv, bn, cin in ((0, 1, 3), (3, 4, 12)):
        x = torch.randn(2, cin, 9, 9, generator=g, dtype=torch.float64)
        p = lambda name: canonical[f"patch_embed.proj.{bn}.{name}"].double()
        want = F.batch_norm(F.conv2d(x, canonical[f"patch_embed.proj.{conv}.weight"].double(), stride=2, padding=1),
                            p("running_mean"), p("running_var"), p("weight"), p("bias"), False, 0.0, 1e-5)
        got = F.conv2d(x, folded[f"patch_embed.proj.{conv}.weight"].double(), folded[f"patch_embed.proj.{conv}.bias"].double(),
                       stride=2, padding=1)
        rel = float((got - want).norm() / want.norm())
        assert rel <= 1e-6, (conv, rel)     # the fold itself is float32
    assert torch.equal(folded["layers.0.blocks.0.attn.qkv.weight"], canonical["layers.0.blocks.0.attn.qkv.weight"])


def test_relative_bias_expansion_against_a_double_loop():
    from atlaspatch_amd.encoders.swin import expand_relative_bias
    table = torch.randn(169, 6, generator=torch.Generator().manual_seed(1))
    got = expand_relative_bias(table)
    assert got.shape == (6, 49, 49) and got.dtype == torch.float32 and got.is_contiguous()
    want = torch.empty(6, 49, 49)
    for yi in range(7):
        for xi in range(7):
            for yj in range(7):
                for xj in range(7):
                    want[:, yi * 7 + xi, yj * 7 + xj] = table[(yi - yj + 6) * 13 + (xi - xj + 6)]
    assert torch.equal(got, want)
    assert torch.equal(got, ref.pair_bias(table))


# ----------------------------------------------------------------------------- registration and builder
def test_shipped_plugin_adds_the_name_and_the_default_registry_is_unchanged():
    import atlaspatch_amd.plugins.chief_ctranspath as plugin
    import atlaspatch_amd.plugins.torchvision_convnexts as convnexts
    import atlaspatch_amd.plugins.torchvision_resnets as resnets
    from atlaspatch_amd.encoders import build_default_registry, register_feature_extractors_from_module
    base = build_default_registry(device="cpu").available()
    assert len(base) == 40 and "chief-ctranspath" not in base
    reg = build_default_registry(device="cpu")
    register_feature_extractors_from_module(plugin.__file__, reg, device=torch.device("cpu"), dtype=torch.float16)
    assert sorted(set(reg.available()) - set(base)) == ["chief-ctranspath"]
    register_feature_extractors_from_module(convnexts.__file__, reg, device=torch.device("cpu"), dtype=torch.float16)
    register_feature_extractors_from_module(resnets.__file__, reg, device=torch.device("cpu"), dtype=torch.float16)
    assert len(set(reg.available()) - set(base)) == 10         # all three plugins in one registry
    assert build_default_registry(device="cpu").available() == base


def test_builder_without_weights_or_seed_says_what_to_do(monkeypatch):
    from atlaspatch_amd.encoders.swin import build_hip_swin_extractor
    monkeypatch.delenv("ATLASPATCH_WEIGHTS_DIR", raising=False)
    with pytest.raises(FileNotFoundError, match="ATLASPATCH_RANDOM_INIT"):
        build_hip_swin_extractor(device="cpu", dtype=torch.float32)


def test_seeded_random_init_is_deterministic_and_well_conditioned():
    from atlaspatch_amd.encoders.swin import ARCHS, random_canonical_state_dict
    a = random_canonical_state_dict(ARCH, seed=11)
    b = random_canonical_state_dict(ARCH, seed=11)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    c = random_canonical_state_dict(ARCH, seed=12)
    assert not torch.equal(a["patch_embed.proj.0.weight"], c["patch_embed.proj.0.weight"])
    table = a["layers.0.blocks.1.attn.relative_position_bias_table"]
    assert float(table.std()) > 0.5                                                  # O(1): a wrong index changes the features
    assert float(a["patch_embed.proj.4.running_var"].sub(1).abs().mean()) > 0.1
    rng = np.random.default_rng(0)
    tiles = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(2)]
    x = torch.stack([ref.preprocess(t) for t in tiles])
    assert x.shape == (2, 3, 224, 224)
    ratios = []
    with torch.no_grad():
        feat = ref.forward(a, x, branch_ratios=ratios)
    assert len(ratios) == 2 * sum(ARCHS[ARCH]["depths"])
    assert 0.05 < min(ratios) and max(ratios) < 2.0, (min(ratios), max(ratios))   # every block's branches are visible
    assert feat.shape == (2, 768) and float(feat.abs().max()) < 100.0 and float(feat.std()) > 0.01
