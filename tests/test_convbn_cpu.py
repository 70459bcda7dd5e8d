"""The conv + BatchNorm host module shared by the ResNet, CLIP ResNet and Swin (stem) encoders: the fold against
conv2d + batch_norm in float64, its refusal through each family's ``fold_batchnorm``, and the stage enumeration against
lists written out here."""
import pytest
import torch
import torch.nn.functional as F


def test_fold_conv_bn_matches_conv_plus_bn_in_fp64():
    """A 3x3 stride-2 convolution, 5 -> 7 channels, on a 9x9 input.  The fold is float32, so the bound is float32's
    (the one test_resnet_cpu.py uses for the same comparison)."""
    from atlaspatch_amd.encoders.convbn import BN_EPS, fold_conv_bn
    g = torch.Generator().manual_seed(4)
    sd = {"c.conv2.weight": torch.randn(7, 5, 3, 3, generator=g) * 0.2,
          "c.bn2.weight": 0.5 + torch.rand(7, generator=g), "c.bn2.bias": 0.1 * torch.randn(7, generator=g),
          "c.bn2.running_mean": 0.1 * torch.randn(7, generator=g), "c.bn2.running_var": 0.5 + torch.rand(7, generator=g)}
    w, b = fold_conv_bn(sd, "c.conv2", "c.bn2", torch.float32, BN_EPS)
    assert w.shape == (7, 5, 3, 3) and b.shape == (7,) and w.dtype == b.dtype == torch.float32
    x = torch.randn(2, 5, 9, 9, generator=g, dtype=torch.float64)
    y = F.conv2d(x, sd["c.conv2.weight"].double(), stride=2, padding=1)
    want = F.batch_norm(y, sd["c.bn2.running_mean"].double(), sd["c.bn2.running_var"].double(), sd["c.bn2.weight"].double(),
                        sd["c.bn2.bias"].double(), False, 0.0, BN_EPS)
    got = F.conv2d(x, w.double(), b.double(), stride=2, padding=1)
    rel = float((got - want).norm() / want.norm())
    print(f"fold_conv_bn vs float64 conv + batch_norm: rel {rel:.3e}")
    assert got.shape == (2, 7, 5, 5) and rel <= 1e-6, rel


TINY_CLIP = {"depths": (1, 1, 1, 1), "width": 32, "image_size": 64, "output_dim": 64}


@pytest.mark.parametrize("family,arch,bn", [("resnet", "resnet18", "layer1.0.bn1"), ("clip_resnet", TINY_CLIP, "layer1.0.bn1"),
                                            ("swin", "chief-ctranspath", "patch_embed.proj.1")], ids=["resnet", "clip_resnet", "swin"])
def test_every_family_refuses_a_fold_outside_the_compute_type(family, arch, bn):
    import importlib
    mod = importlib.import_module(f"atlaspatch_amd.encoders.{family}")
    canonical = mod.random_canonical_state_dict(arch, seed=0)
    canonical[f"{bn}.running_var"] = torch.full_like(canonical[f"{bn}.running_var"], 1e-12)
    canonical[f"{bn}.weight"] = torch.full_like(canonical[f"{bn}.weight"], 1e3)
    folded = mod.fold_batchnorm(canonical, arch=arch, dtype=torch.float32)      # 3e5-ish: fine in float32
    assert all(bool(torch.isfinite(v).all()) for v in folded.values())
    with pytest.raises(ValueError, match="not finite in torch.float16"):
        mod.fold_batchnorm(canonical, arch=arch, dtype=torch.float16)


# (name, cout, cin, k, stride): the stem, stage 1 and the first block of stage 2
RESNET18 = [("conv1", 64, 3, 7, 2),
            ("layer1.0.conv1", 64, 64, 3, 1), ("layer1.0.conv2", 64, 64, 3, 1),
            ("layer1.1.conv1", 64, 64, 3, 1), ("layer1.1.conv2", 64, 64, 3, 1),
            ("layer2.0.conv1", 128, 64, 3, 2), ("layer2.0.conv2", 128, 128, 3, 1), ("layer2.0.downsample", 128, 64, 1, 2)]
RESNET50 = [("conv1", 64, 3, 7, 2),
            ("layer1.0.conv1", 64, 64, 1, 1), ("layer1.0.conv2", 64, 64, 3, 1), ("layer1.0.conv3", 256, 64, 1, 1),
            ("layer1.0.downsample", 256, 64, 1, 1),
            ("layer1.1.conv1", 64, 256, 1, 1), ("layer1.1.conv2", 64, 64, 3, 1), ("layer1.1.conv3", 256, 64, 1, 1),
            ("layer1.2.conv1", 64, 256, 1, 1), ("layer1.2.conv2", 64, 64, 3, 1), ("layer1.2.conv3", 256, 64, 1, 1),
            ("layer2.0.conv1", 128, 256, 1, 1), ("layer2.0.conv2", 128, 128, 3, 2), ("layer2.0.conv3", 512, 128, 1, 1),
            ("layer2.0.downsample", 512, 256, 1, 2)]
# CLIP: every block convolution has stride 1 (a 2x2 average pool carries the stride); the projection's entry names the block's
CLIP_RN50X4 = [("conv1", 40, 3, 3, 2), ("conv2", 40, 40, 3, 1), ("conv3", 80, 40, 3, 1),
               ("layer1.0.conv1", 80, 80, 1, 1), ("layer1.0.conv2", 80, 80, 3, 1), ("layer1.0.conv3", 320, 80, 1, 1),
               ("layer1.0.downsample", 320, 80, 1, 1),
               ("layer1.1.conv1", 80, 320, 1, 1), ("layer1.1.conv2", 80, 80, 3, 1), ("layer1.1.conv3", 320, 80, 1, 1),
               ("layer1.2.conv1", 80, 320, 1, 1), ("layer1.2.conv2", 80, 80, 3, 1), ("layer1.2.conv3", 320, 80, 1, 1),
               ("layer1.3.conv1", 80, 320, 1, 1), ("layer1.3.conv2", 80, 80, 3, 1), ("layer1.3.conv3", 320, 80, 1, 1),
               ("layer2.0.conv1", 160, 320, 1, 1), ("layer2.0.conv2", 160, 160, 3, 1), ("layer2.0.conv3", 640, 160, 1, 1),
               ("layer2.0.downsample", 640, 320, 1, 2)]


@pytest.mark.parametrize("family,arch,want,total", [("resnet", "resnet18", RESNET18, 20), ("resnet", "resnet50", RESNET50, 53),
                                                    ("clip_resnet", "clip_rn50x4", CLIP_RN50X4, 85)],
                         ids=["resnet18", "resnet50", "clip_rn50x4"])
def test_conv_layers_against_written_out_lists(family, arch, want, total):
    """``total``: the network's convolutions -- the stem's, two or three a block, one projection a stage (resnet18: stages
    2..4 only)."""
    import importlib
    mod = importlib.import_module(f"atlaspatch_amd.encoders.{family}")
    layers = mod.conv_layers(arch)
    assert layers[:len(want)] == want
    assert layers[len(want)][0] == "layer2.1.conv1" and len(layers) == total
    keys = mod.canonical_keys(arch)
    for name, cout, cin, k, _ in want:
        wkey = name + (".0.weight" if name.endswith("downsample") else ".weight")
        bn = name + ".1" if name.endswith("downsample") else name.replace("conv", "bn")
        assert keys[wkey] == (cout, cin, k, k), name
        assert [keys[f"{bn}.{p}"] for p in ("weight", "bias", "running_mean", "running_var")] == [(cout,)] * 4, name
