"""ConvNeXt encoders, CPU side: the restatement against transformers ConvNextModel, the two checkpoint layouts, layer_scale
folding, the registration through the shipped plugin, and the seeded random init."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import convnext_reference as ref


def _hf_model(depths, widths, seed=0):
    from transformers import ConvNextConfig, ConvNextModel
    torch.manual_seed(seed)
    model = ConvNextModel(ConvNextConfig(depths=list(depths), hidden_sizes=list(widths))).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("layer_scale_parameter"):          # O(1), not the 1e-6 init: every block must matter
                p.copy_(0.3 + 0.5 * torch.rand(p.shape, generator=g))
            elif "layernorm" in name and name.endswith("weight"):
                p.copy_(0.8 + 0.4 * torch.rand(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return model


CONFIGS = [((3, 3, 9, 3), (96, 192, 384, 768)),          # convnext_tiny
           ((2, 1, 3, 1), (128, 256, 512, 1024))]        # base widths, shortened depth


@pytest.mark.parametrize("depths,widths", CONFIGS, ids=["tiny", "base_width_short"])
def test_restatement_equals_transformers_convnext(depths, widths):
    from atlaspatch_amd.encoders.convnext import canonical_state_dict
    model = _hf_model(depths, widths)
    arch = {"depths": depths, "widths": widths}
    sd = canonical_state_dict(model.state_dict(), arch=arch, source="auto")
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        out = model(pixel_values=x)
        want = out.last_hidden_state.mean((-2, -1))
        got = ref.forward(sd, x, depths=depths)
    rel = float((got - want).norm() / want.norm())
    assert got.shape == want.shape == (2, widths[3]) and rel <= 1e-5, rel
    # the feature is the pool BEFORE the head's LayerNorm: pooler_output (LayerNorm applied) is something else
    far = float((got - out.pooler_output).norm() / out.pooler_output.norm())
    assert far > 0.1, far


def _canonical_to_hf(canonical):
    """torchvision keys -> transformers ConvNextModel keys (the inverse of the adapter, written independently)."""
    parts = {"0": "dwconv", "2": "layernorm", "3": "pwconv1", "5": "pwconv2"}
    out = {}
    for k, v in canonical.items():
        f = k.split(".")
        idx = int(f[1])
        if idx == 0:
            out[("embeddings.patch_embeddings." if f[2] == "0" else "embeddings.layernorm.") + f[3]] = v
        elif idx % 2 == 0:
            out[f"encoder.stages.{idx // 2}.downsampling_layer.{f[2]}.{f[3]}"] = v
        elif f[3] == "layer_scale":
            out[f"encoder.stages.{idx // 2}.layers.{f[2]}.layer_scale_parameter"] = v.reshape(-1)
        else:
            out[f"encoder.stages.{idx // 2}.layers.{f[2]}.{parts[f[4]]}.{f[5]}"] = v
    return out


@pytest.mark.parametrize("arch", ["convnext_tiny", "convnext_large"])
def test_torchvision_and_hf_adapters_agree(arch):
    from atlaspatch_amd.encoders.convnext import canonical_state_dict, detect_source, random_canonical_state_dict
    canonical = random_canonical_state_dict(arch, seed=5)
    tv = dict(canonical)
    tv["classifier.0.weight"] = torch.ones(canonical["features.0.0.bias"].shape[0] * 8)
    tv["classifier.2.weight"] = torch.zeros(1000, canonical["features.0.0.bias"].shape[0] * 8)
    hf = {"convnext." + k: v for k, v in _canonical_to_hf(canonical).items()}
    hf["convnext.layernorm.weight"] = torch.ones(3)
    hf["classifier.weight"] = torch.zeros(1000, 3)
    assert detect_source(tv) == "torchvision" and detect_source(hf) == "hf"
    a = canonical_state_dict(tv, arch=arch)
    b = canonical_state_dict(hf, arch=arch)
    assert a.keys() == b.keys() == canonical.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], canonical[k]), k


def test_adapter_refuses_unknown_and_missing_keys():
    from atlaspatch_amd.encoders.convnext import canonical_state_dict, random_canonical_state_dict
    canonical = random_canonical_state_dict("convnext_tiny", seed=0)
    bad = dict(canonical)
    bad["features.9.0.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="unknown key"):
        canonical_state_dict(bad, arch="convnext_tiny")
    short = dict(canonical)
    del short["features.5.8.layer_scale"]
    with pytest.raises(ValueError, match="missing key"):
        canonical_state_dict(short, arch="convnext_tiny")
    with pytest.raises(ValueError, match="unknown key"):        # a convnext_small checkpoint is not a convnext_tiny one
        canonical_state_dict(random_canonical_state_dict("convnext_small", seed=0), arch="convnext_tiny")
    with pytest.raises(ValueError, match="shape"):               # nor is a convnext_base one (same depths, other widths)
        canonical_state_dict(random_canonical_state_dict("convnext_base", seed=0), arch="convnext_small")
    with pytest.raises(ValueError, match="neither torchvision"):
        canonical_state_dict({"blocks.0.weight": torch.zeros(1)}, arch="convnext_tiny")


def test_layer_scale_folding_matches_unfolded_fc2_in_fp64():
    from atlaspatch_amd.encoders.convnext import canonical_keys, fold_layer_scale, random_canonical_state_dict
    canonical = random_canonical_state_dict("convnext_tiny", seed=2)
    folded = fold_layer_scale(canonical, arch="convnext_tiny")
    assert not any(k.endswith("layer_scale") for k in folded)
    assert set(folded) == {k for k in canonical_keys("convnext_tiny") if not k.endswith("layer_scale")}
    g = torch.Generator().manual_seed(0)
    for pre in ("features.1.0.", "features.5.8.", "features.7.2."):
        w, b = canonical[pre + "block.5.weight"].double(), canonical[pre + "block.5.bias"].double()
        gamma = canonical[pre + "layer_scale"].double().reshape(-1)
        h = torch.randn(7, w.shape[1], generator=g, dtype=torch.float64)
        want = F.linear(h, w, b) * gamma
        got = F.linear(h, folded[pre + "block.5.weight"].double(), folded[pre + "block.5.bias"].double())
        rel = float((got - want).norm() / want.norm())
        assert rel <= 1e-6, (pre, rel)      # the fold itself is float32
        assert torch.equal(folded[pre + "block.3.weight"], canonical[pre + "block.3.weight"])


def test_register_convnexts_names_and_dims():
    from atlaspatch_amd.encoders import PatchFeatureExtractorRegistry
    from atlaspatch_amd.encoders.convnext import ARCHS, register_convnexts
    reg = PatchFeatureExtractorRegistry()
    register_convnexts(reg, device="cpu", dtype=torch.float16, num_workers=0)
    names = ["convnext_tiny", "convnext_small", "convnext_base", "convnext_large"]
    assert reg.available() == sorted(names)
    assert [ARCHS[n]["embed_dim"] for n in names] == [768, 768, 1024, 1536]
    assert [ARCHS[n]["resize"] for n in names] == [236, 230, 232, 232]


def test_shipped_plugin_adds_the_four_names_and_the_default_registry_is_unchanged():
    import atlaspatch_amd.plugins.torchvision_convnexts as plugin
    import atlaspatch_amd.plugins.torchvision_resnets as resnets
    from atlaspatch_amd.encoders import build_default_registry, register_feature_extractors_from_module
    base = build_default_registry(device="cpu").available()
    assert len(base) == 40 and not any(n.startswith("convnext") for n in base)
    reg = build_default_registry(device="cpu")
    register_feature_extractors_from_module(plugin.__file__, reg, device=torch.device("cpu"), dtype=torch.float16)
    assert sorted(set(reg.available()) - set(base)) == ["convnext_base", "convnext_large", "convnext_small", "convnext_tiny"]
    register_feature_extractors_from_module(resnets.__file__, reg, device=torch.device("cpu"), dtype=torch.float16)
    assert len(set(reg.available()) - set(base)) == 9          # both plugins in one registry
    assert build_default_registry(device="cpu").available() == base


def test_builder_without_weights_or_seed_says_what_to_do(monkeypatch):
    from atlaspatch_amd.encoders.convnext import build_hip_convnext_extractor
    monkeypatch.delenv("ATLASPATCH_WEIGHTS_DIR", raising=False)
    with pytest.raises(FileNotFoundError, match="ATLASPATCH_RANDOM_INIT"):
        build_hip_convnext_extractor(name="convnext_tiny", arch="convnext_tiny", device="cpu", dtype=torch.float32)


@pytest.mark.parametrize("arch", ["convnext_tiny", "convnext_large"])
def test_seeded_random_init_is_deterministic_and_well_conditioned(arch):
    from atlaspatch_amd.encoders.convnext import ARCHS, random_canonical_state_dict
    a = random_canonical_state_dict(arch, seed=11)
    b = random_canonical_state_dict(arch, seed=11)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    c = random_canonical_state_dict(arch, seed=12)
    assert not torch.equal(a["features.0.0.weight"], c["features.0.0.weight"])
    spec = ARCHS[arch]
    rng = np.random.default_rng(0)
    tiles = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(2)]
    x = torch.stack([ref.preprocess(t, resize=spec["resize"]) for t in tiles])
    ratios = []
    with torch.no_grad():
        feat = ref.forward(a, x, depths=spec["depths"], branch_ratios=ratios)
    assert len(ratios) == sum(spec["depths"])
    assert 0.05 < min(ratios) and max(ratios) < 2.0, (min(ratios), max(ratios))   # every block's branch is visible
    assert feat.shape == (2, spec["embed_dim"]) and float(feat.abs().max()) < 100.0 and float(feat.std()) > 0.01
