"""ResNet encoders, CPU side: the restatement against transformers ResNetModel, the two checkpoint layouts, BatchNorm
folding, the registration through the shipped plugin, and the seeded random init."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resnet_reference as ref


def _hf_model(layer_type, depths, seed=0):
    from transformers import ResNetConfig, ResNetModel
    torch.manual_seed(seed)
    hidden = [64, 128, 256, 512] if layer_type == "basic" else [256, 512, 1024, 2048]
    model = ResNetModel(ResNetConfig(layer_type=layer_type, depths=depths, hidden_sizes=hidden, embedding_size=64)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):       # non-trivial eval statistics
                c = mod.num_features
                mod.weight.copy_(0.5 + torch.rand(c, generator=g))
                mod.bias.copy_(0.1 * torch.randn(c, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(c, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(c, generator=g))
    return model


def _hf_to_tv(model, arch):
    from atlaspatch_amd.encoders.resnet import canonical_state_dict
    return canonical_state_dict(model.state_dict(), arch=arch, source="auto")


@pytest.mark.parametrize("layer_type,depths,arch", [("basic", [2, 2, 2, 2], "resnet18"), ("bottleneck", [3, 4, 6, 3], "resnet50")])
def test_restatement_equals_transformers_resnet(layer_type, depths, arch):
    model = _hf_model(layer_type, depths)
    sd = _hf_to_tv(model, arch)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = model(pixel_values=x).pooler_output.flatten(1)
        got = ref.forward(sd, x, block=layer_type, depths=depths)
    rel = float((got - want).norm() / want.norm())
    assert got.shape == want.shape and rel <= 2e-6, rel


def _tv_keys_from(canonical, extra=True):
    sd = dict(canonical)
    if extra:
        sd["fc.weight"] = torch.zeros(1000, 2048)
        sd["fc.bias"] = torch.zeros(1000)
        sd["bn1.num_batches_tracked"] = torch.tensor(0)
    return sd


def _canonical_to_hf(canonical):
    """torchvision keys -> transformers ResNetModel keys (the inverse of the adapter, written independently)."""
    out = {}
    for k, v in canonical.items():
        if k.startswith("conv1."):
            out["embedder.embedder.convolution." + k[6:]] = v
        elif k.startswith("bn1."):
            out["embedder.embedder.normalization." + k[4:]] = v
        else:
            layer, blk, rest = k.split(".", 2)
            pre = f"encoder.stages.{int(layer[5:]) - 1}.layers.{blk}."
            if rest.startswith("downsample.0."):
                out[pre + "shortcut.convolution." + rest[13:]] = v
            elif rest.startswith("downsample.1."):
                out[pre + "shortcut.normalization." + rest[13:]] = v
            elif rest.startswith("conv"):
                out[pre + f"layer.{int(rest[4]) - 1}.convolution." + rest[6:]] = v
            else:
                out[pre + f"layer.{int(rest[2]) - 1}.normalization." + rest[4:]] = v
    return out


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_torchvision_and_hf_adapters_agree(arch):
    from atlaspatch_amd.encoders.resnet import canonical_state_dict, detect_source, random_canonical_state_dict
    canonical = random_canonical_state_dict(arch, seed=5)
    tv = _tv_keys_from(canonical, extra=arch == "resnet50")
    hf = {"resnet." + k: v for k, v in _canonical_to_hf(canonical).items()}
    hf["classifier.1.weight"] = torch.zeros(1000, 2048)
    assert detect_source(tv) == "torchvision" and detect_source(hf) == "hf"
    a = canonical_state_dict(tv, arch=arch)
    b = canonical_state_dict(hf, arch=arch)
    assert a.keys() == b.keys() == canonical.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], canonical[k]), k


def test_adapter_refuses_unknown_and_missing_keys():
    from atlaspatch_amd.encoders.resnet import canonical_state_dict, random_canonical_state_dict
    canonical = random_canonical_state_dict("resnet18", seed=0)
    bad = dict(canonical)
    bad["layer5.0.conv1.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="unknown key"):
        canonical_state_dict(bad, arch="resnet18")
    short = dict(canonical)
    del short["layer2.0.downsample.0.weight"]
    with pytest.raises(ValueError, match="missing key"):
        canonical_state_dict(short, arch="resnet18")
    with pytest.raises(ValueError, match="unknown key"):          # a resnet50 checkpoint is not a resnet18 one
        canonical_state_dict(random_canonical_state_dict("resnet50", seed=0), arch="resnet18")
    with pytest.raises(ValueError, match="neither torchvision"):
        canonical_state_dict({"blocks.0.weight": torch.zeros(1)}, arch="resnet18")


def test_batchnorm_folding_matches_conv_plus_bn_in_fp64():
    from atlaspatch_amd.encoders.resnet import conv_layers, fold_batchnorm, random_canonical_state_dict
    canonical = random_canonical_state_dict("resnet18", seed=2)
    folded = fold_batchnorm(canonical, arch="resnet18")
    g = torch.Generator().manual_seed(0)
    for name, cout, cin, k, stride in conv_layers("resnet18")[:6] + [l for l in conv_layers("resnet18") if "downsample" in l[0]]:
        x = torch.randn(1, cin, 9, 9, generator=g, dtype=torch.float64)
        wkey = name + (".0.weight" if name.endswith("downsample") else ".weight")
        bn = "bn1" if name == "conv1" else (name + ".1" if name.endswith("downsample") else name.rsplit(".", 1)[0] + ".bn" + name[-1])
        y = F.conv2d(x, canonical[wkey].double(), stride=stride, padding=k // 2)
        want = F.batch_norm(y, canonical[bn + ".running_mean"].double(), canonical[bn + ".running_var"].double(),
                            canonical[bn + ".weight"].double(), canonical[bn + ".bias"].double(), False, 0.0, 1e-5)
        got = F.conv2d(x, folded[name + ".weight"].double(), folded[name + ".bias"].double(), stride=stride, padding=k // 2)
        rel = float((got - want).norm() / want.norm())
        assert rel <= 1e-6, (name, rel)       # the fold itself is float32


def test_fold_refuses_weights_outside_the_compute_type():
    from atlaspatch_amd.encoders.resnet import fold_batchnorm, random_canonical_state_dict
    canonical = random_canonical_state_dict("resnet18", seed=0)
    canonical["layer1.0.bn1.running_var"] = torch.full_like(canonical["layer1.0.bn1.running_var"], 1e-12)
    canonical["layer1.0.bn1.weight"] = torch.full_like(canonical["layer1.0.bn1.weight"], 1e3)
    fold_batchnorm(canonical, arch="resnet18", dtype=torch.float32)             # 3e5-ish: fine in f32
    with pytest.raises(ValueError, match="not finite in torch.float16"):
        fold_batchnorm(canonical, arch="resnet18", dtype=torch.float16)


def test_register_resnets_names_and_dims():
    from atlaspatch_amd.encoders import PatchFeatureExtractorRegistry
    from atlaspatch_amd.encoders.resnet import ARCHS, register_resnets
    reg = PatchFeatureExtractorRegistry()
    register_resnets(reg, device="cpu", dtype=torch.float16, num_workers=0)
    assert reg.available() == sorted(["resnet18", "resnet34", "resnet50", "resnet101", "resnet152"])
    assert [ARCHS[n]["embed_dim"] for n in ("resnet18", "resnet34", "resnet50", "resnet101", "resnet152")] == \
        [512, 512, 2048, 2048, 2048]


def test_shipped_plugin_adds_the_five_names_and_the_default_registry_is_unchanged():
    import atlaspatch_amd.plugins.torchvision_resnets as plugin
    from atlaspatch_amd.encoders import build_default_registry, register_feature_extractors_from_module
    base = build_default_registry(device="cpu").available()
    assert len(base) == 40 and not any(n.startswith("resnet") for n in base)
    reg = build_default_registry(device="cpu")
    register_feature_extractors_from_module(plugin.__file__, reg, device=torch.device("cpu"), dtype=torch.float16)
    assert sorted(set(reg.available()) - set(base)) == ["resnet101", "resnet152", "resnet18", "resnet34", "resnet50"]
    assert build_default_registry(device="cpu").available() == base


def test_builder_without_weights_or_seed_says_what_to_do(monkeypatch):
    from atlaspatch_amd.encoders.resnet import build_hip_resnet_extractor
    monkeypatch.delenv("ATLASPATCH_WEIGHTS_DIR", raising=False)
    with pytest.raises(FileNotFoundError, match="ATLASPATCH_RANDOM_INIT"):
        build_hip_resnet_extractor(name="resnet18", arch="resnet18", device="cpu", dtype=torch.float32)


@pytest.mark.parametrize("arch", ["resnet18", "resnet50", "resnet152"])
def test_seeded_random_init_is_deterministic_and_well_conditioned(arch):
    from atlaspatch_amd.encoders.resnet import ARCHS, random_canonical_state_dict
    a = random_canonical_state_dict(arch, seed=11)
    b = random_canonical_state_dict(arch, seed=11)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    c = random_canonical_state_dict(arch, seed=12)
    assert not torch.equal(a["conv1.weight"], c["conv1.weight"])
    spec = ARCHS[arch]
    rng = np.random.default_rng(0)
    tiles = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(2)]
    x = torch.stack([ref.preprocess(t) for t in tiles])
    stages = []
    with torch.no_grad():
        feat = ref.forward(a, x, block=spec["block"], depths=spec["depths"], stages_out=stages)
    assert len(stages) == 5
    for i, s in enumerate(stages):
        peak = float(s.abs().max())
        assert 0.05 < peak < 200.0, (i, peak)       # O(1): far inside float16's 65504, far above its resolution
    assert feat.shape == (2, spec["embed_dim"]) and float(feat.std()) > 0.01
