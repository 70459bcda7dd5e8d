"""CPU: the OpenAI CLIP ResNet encoders without a GPU -- the architecture table, the restatement's head against torch's
multi-head attention, the BatchNorm fold, the checkpoint key adapter, the channel padding and the plugin's registration."""
import pytest
import torch
import torch.nn.functional as F

from tests import clip_resnet_reference as ref

TINY80 = {"depths": (1, 1, 1, 1), "width": 80, "image_size": 96, "output_dim": 64}
TINY32 = {"depths": (1, 2, 1, 1), "width": 32, "image_size": 64, "output_dim": 64}


def test_architecture_table_and_parameter_shapes():
    from atlaspatch_amd.encoders.clip_resnet import ARCHS, MAX_BATCH, canonical_keys, conv_layers, embed_width, grid_size, stored_channels
    assert list(ARCHS) == ["clip_rn50", "clip_rn101", "clip_rn50x4", "clip_rn50x16", "clip_rn50x64"]
    assert [ARCHS[a]["output_dim"] for a in ARCHS] == [1024, 512, 640, 768, 1024]          # models/patch/clip.py
    assert [ARCHS[a]["image_size"] for a in ARCHS] == [224, 224, 288, 384, 448]
    for arch, spec in ARCHS.items():
        w, c, g = spec["width"], embed_width(arch), grid_size(arch)
        assert c == 32 * w and c // 64 == w // 2 and g * 32 == spec["image_size"]
        layers = conv_layers(arch)
        assert [l[:4] for l in layers[:3]] == [("conv1", w // 2, 3, 3), ("conv2", w // 2, w // 2, 3), ("conv3", w, w // 2, 3)]
        assert layers[0][4] == 2 and sum(1 for l in layers if l[0].endswith("downsample")) == 4
        assert len(layers) == 3 + 3 * sum(spec["depths"]) + 4
        inplanes = w
        for s, depth in enumerate(spec["depths"]):
            by_name = {l[0]: l for l in layers}
            for b in range(depth):
                pre = f"layer{s + 1}.{b}."
                planes = w << s
                assert by_name[pre + "conv1"][1:] == (planes, inplanes, 1, 1)
                assert by_name[pre + "conv2"][1:] == (planes, planes, 3, 1)                    # stride 1: the pool carries the stride
                assert by_name[pre + "conv3"][1:] == (4 * planes, planes, 1, 1)
                assert (pre + "downsample" in by_name) == (b == 0)
                if b == 0:
                    assert by_name[pre + "downsample"][1:] == (4 * planes, inplanes, 1, 2 if s else 1)
                inplanes = 4 * planes
        assert inplanes == c
        keys = canonical_keys(arch)
        assert keys["attnpool.positional_embedding"] == (g * g + 1, c)
        assert keys["attnpool.c_proj.weight"] == (spec["output_dim"], c) and keys["attnpool.k_proj.weight"] == (c, c)
        assert keys["layer2.0.downsample.0.weight"] == (8 * w, 4 * w, 1, 1) and keys["layer2.0.downsample.1.running_var"] == (8 * w,)
        assert len(keys) == 5 * len(layers) + 9
        # four buffers of the largest activation at MAX_BATCH stay below 2 GB in float16
        half = spec["image_size"] // 2
        biggest = max(half * half * stored_channels(w), (half // 2) ** 2 * 4 * w, spec["image_size"] ** 2 * 8)
        assert 4 * biggest * 2 * MAX_BATCH[arch] < 2e9
    assert [stored_channels(c) for c in (16, 40, 48, 80, 96, 64)] == [32, 64, 64, 96, 96, 64]


def test_head_equals_torch_multi_head_attention():
    """The restatement's explicit head against F.multi_head_attention_forward with separate projection weights and the mean
    token as the query -- the form OpenAI's AttentionPool2d uses."""
    g = torch.Generator().manual_seed(5)
    for c, grid, dim, n in ((128, 2, 64, 3), (256, 3, 96, 2)):
        x = torch.randn(n, c, grid, grid, generator=g)
        pos = torch.randn(grid * grid + 1, c, generator=g) * c ** -0.5
        w = {k: torch.randn(dim if k == "c" else c, c, generator=g) * c ** -0.5 for k in "qkvc"}
        b = {k: 0.1 * torch.randn(dim if k == "c" else c, generator=g) for k in "qkvc"}
        got = ref.attention_pool(x, pos, w["q"], b["q"], w["k"], b["k"], w["v"], b["v"], w["c"], b["c"])
        t = x.flatten(2).permute(2, 0, 1)                                        # [g g, n, C]
        t = torch.cat([t.mean(dim=0, keepdim=True), t], dim=0) + pos[:, None, :]
        want, _ = F.multi_head_attention_forward(
            query=t[:1], key=t, value=t, embed_dim_to_check=c, num_heads=c // 64, q_proj_weight=w["q"], k_proj_weight=w["k"],
            v_proj_weight=w["v"], in_proj_weight=None, in_proj_bias=torch.cat([b["q"], b["k"], b["v"]]), bias_k=None, bias_v=None,
            add_zero_attn=False, dropout_p=0.0, out_proj_weight=w["c"], out_proj_bias=b["c"], use_separate_proj_weight=True,
            training=False, need_weights=False)
        assert got.shape == (n, dim)
        assert float((got - want[0]).abs().max()) <= 1e-6


@pytest.mark.parametrize("arch", [TINY32, TINY80], ids=["width32", "width80"])
def test_fold_batchnorm_then_folded_forward_equals_the_unfolded_restatement(arch):
    from atlaspatch_amd.encoders.clip_resnet import fold_batchnorm, random_canonical_state_dict
    sd = random_canonical_state_dict(arch, seed=2)
    folded = fold_batchnorm(sd, arch=arch)
    x = torch.randn(2, 3, arch["image_size"], arch["image_size"], generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = ref.forward(sd, x, depths=arch["depths"])
        got = ref.forward_folded(folded, x, depths=arch["depths"])
    assert want.shape == (2, 64) and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 1e-2
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert folded["attnpool.kv.weight"].shape == (2 * 32 * arch["width"], 32 * arch["width"], 1, 1)


def test_key_adapter_round_trips_and_refuses():
    from atlaspatch_amd.encoders.clip_resnet import canonical_keys, canonical_state_dict, random_canonical_state_dict
    arch = TINY32
    sd = random_canonical_state_dict(arch, seed=4)
    same = lambda got: got.keys() == sd.keys() and all(torch.equal(got[k], sd[k]) for k in sd)
    assert sd.keys() == canonical_keys(arch).keys()
    assert same(canonical_state_dict(sd, arch=arch))
    visual = {"visual." + k: v for k, v in sd.items()}
    visual["visual.bn1.num_batches_tracked"] = torch.tensor(7)
    assert same(canonical_state_dict(visual, arch=arch))
    whole = dict(visual)                                                    # a whole CLIP model: text tower and scalars dropped
    whole.update({"positional_embedding": torch.zeros(77, 8), "text_projection": torch.zeros(8, 8), "logit_scale": torch.tensor(4.6),
                  "input_resolution": torch.tensor(64), "context_length": torch.tensor(77), "vocab_size": torch.tensor(49408),
                  "token_embedding.weight": torch.zeros(10, 8), "transformer.resblocks.0.ln_1.weight": torch.zeros(8),
                  "ln_final.bias": torch.zeros(8)})
    assert same(canonical_state_dict(whole, arch=arch))
    assert same(canonical_state_dict({"module." + k: v for k, v in whole.items()}, arch=arch))
    sd16 = {k: v.half().float() for k, v in sd.items()}                     # fp16-stored tensors come back as their float32 values
    got = canonical_state_dict({"visual." + k: v.half() for k, v in sd.items()}, arch=arch)
    assert all(got[k].dtype == torch.float32 and torch.equal(got[k], sd16[k]) for k in sd)
    missing = dict(visual)
    del missing["visual.layer2.0.downsample.1.running_mean"]
    with pytest.raises(ValueError, match="missing"):
        canonical_state_dict(missing, arch=arch)
    with pytest.raises(ValueError, match="unknown"):
        canonical_state_dict(dict(visual, **{"visual.layer1.0.downsample.2.weight": torch.zeros(3)}), arch=arch)
    with pytest.raises(ValueError, match="unknown"):
        canonical_state_dict(dict(sd, **{"fc.weight": torch.zeros(3)}), arch=arch)
    wrong = dict(visual)
    wrong["visual.attnpool.positional_embedding"] = torch.zeros(50, 32 * arch["width"])       # a 224-px checkpoint's rows
    with pytest.raises(ValueError, match="positional_embedding"):
        canonical_state_dict(wrong, arch=arch)


def _exact_folded(arch, seed):
    """Folded parameters of the convolutional part on which float64 arithmetic is exact whatever the summation order: three
    weights of +-1 per output channel, integer biases.  Every map is then an integer multiple of 2^-12 (six average pools) below
    2^40."""
    from atlaspatch_amd.encoders.clip_resnet import conv_layers
    g = torch.Generator().manual_seed(seed)
    p = {}
    for name, cout, cin, k, _ in conv_layers(arch):
        w = torch.zeros(cout, cin * k * k, dtype=torch.float64)
        for o in range(cout):
            idx = torch.randperm(cin * k * k, generator=g)[:3]
            w[o, idx] = torch.randint(0, 2, (3,), generator=g).double() * 2 - 1
        p[name + ".weight"] = w.view(cout, cin, k, k)
        p[name + ".bias"] = torch.randint(-1, 3, (cout,), generator=g).double()
    return p


def test_channel_padding_leaves_real_channels_bit_identical_and_padded_channels_zero():
    """Width 80: the stem's 40 channels are stored as 64, the 80 of the stem's output and of stage 0 as 96.  The padded parameter
    set (the restatement of the engine's parameter store) against the unpadded one, map by map."""
    from atlaspatch_amd.encoders.clip_resnet import conv_layers, padded_parameters, stored_channels
    arch = TINY80
    p = _exact_folded(arch, seed=9)
    pp = padded_parameters(p, arch=arch)
    shapes = {name: (cout, cin) for name, cout, cin, _, _ in conv_layers(arch)}
    assert pp["conv1.weight"].shape == (64, 8, 3, 3) and pp["conv3.weight"].shape == (96, 64, 3, 3)
    assert pp["layer1.0.conv1.weight"].shape == (96, 96, 1, 1) and pp["layer1.0.conv3.weight"].shape == (320, 96, 1, 1)
    assert pp["layer1.0.downsample.weight"].shape == (320, 96, 1, 1) and pp["layer2.0.conv1.weight"].shape == (160, 320, 1, 1)
    for name, (cout, cin) in shapes.items():
        assert pp[name + ".weight"].shape[0] == stored_channels(cout) == pp[name + ".bias"].shape[0]
        assert torch.equal(pp[name + ".weight"][:cout, :cin], p[name + ".weight"])
        assert not pp[name + ".weight"][cout:].any() and not pp[name + ".weight"][:, cin:].any() and not pp[name + ".bias"][cout:].any()
    x = torch.randint(-4, 5, (2, 3, 96, 96), generator=torch.Generator().manual_seed(3)).double()
    x8 = torch.cat([x, torch.zeros(2, 5, 96, 96, dtype=torch.float64)], dim=1)
    real, padded = [], []
    with torch.no_grad():
        ref.trunk_folded(p, x, depths=arch["depths"], maps=real)
        ref.trunk_folded(pp, x8, depths=arch["depths"], maps=padded)
    assert len(real) == len(padded) == 1 + 4 + 4 * 4 + 3 * 2
    widened = 0
    for a, b in zip(real, padded):
        c = a.shape[1]
        assert b.shape[1] == (8 if c == 3 else stored_channels(c)) and b.shape[2:] == a.shape[2:]
        assert torch.equal(b[:, :c], a) and not b[:, c:].any()
        assert float(a.abs().max()) < 2.0 ** 40 and bool((a * 4096 == (a * 4096).round()).all())     # the arithmetic was exact
        widened += b.shape[1] != c
    assert widened == 1 + 4 + 2 and float(real[-1].abs().max()) > 0


def test_plugin_registers_the_five_names_and_touches_no_gpu(monkeypatch):
    import atlaspatch_amd.plugins.openai_clip_resnets as plugin
    from atlaspatch_amd import _lib
    from atlaspatch_amd.encoders import build_default_registry, register_feature_extractors_from_module
    from atlaspatch_amd.encoders.clip_resnet import ARCHS, register_clip_resnets

    def no_gpu(*a, **k):
        raise AssertionError("the library was loaded before create")
    monkeypatch.setattr(_lib, "load", no_gpu)
    base = build_default_registry(device="cpu").available()
    assert not set(ARCHS) & set(base)
    reg = build_default_registry(device="cpu")
    register_feature_extractors_from_module(plugin.__file__, reg, device=torch.device("cpu"), dtype=torch.float16)
    assert sorted(set(reg.available()) - set(base)) == sorted(ARCHS)
    with pytest.raises(Exception, match="clip_rn50"):                        # registering twice
        register_clip_resnets(reg, device="cpu", dtype=torch.float16)
    assert build_default_registry(device="cpu").available() == base


def test_builder_without_weights_or_seed_says_what_to_do(monkeypatch):
    from atlaspatch_amd.encoders.clip_resnet import build_hip_clip_resnet_extractor
    monkeypatch.delenv("ATLASPATCH_WEIGHTS_DIR", raising=False)
    monkeypatch.delenv("ATLASPATCH_RANDOM_INIT", raising=False)
    with pytest.raises(FileNotFoundError, match="ATLASPATCH_RANDOM_INIT"):
        build_hip_clip_resnet_extractor(name="clip_rn50", arch="clip_rn50", device="cpu", dtype=torch.float32)


def test_engine_refuses_bad_configurations_before_any_device_call():
    """ap_clip_resnet_create's refusals come before any HIP call, so they run here."""
    import ctypes as C
    from atlaspatch_amd import _lib
    L = _lib.load()
    assert L.ap_sizeof_clip_resnet_config() == C.sizeof(_lib.ClipResnetConfig) == 36
    good = dict(depths=(1, 1, 1, 1), width=32, image_size=64, output_dim=64)
    for change, word in (({"image_size": 100}, "image_size"), ({"image_size": 32}, "image_size"), ({"image_size": 1056}, "image_size"),
                         ({"width": 24}, "width"), ({"depths": (1, 0, 1, 1)}, "depths"), ({"depths": (1, 1, 65, 1)}, "depths"),
                         ({"output_dim": 48}, "output_dim")):
        spec = dict(good, **change)
        cfg = _lib.ClipResnetConfig((C.c_int * 4)(*spec["depths"]), spec["width"], spec["image_size"], spec["output_dim"], 1)
        handle = C.c_void_p()
        assert L.ap_clip_resnet_create(C.byref(cfg), C.byref(handle)) == _lib.AP_ERR_INVALID and not handle.value, change
        assert word in L.ap_last_error().decode(), change
    cfg = _lib.ClipResnetConfig()
    assert L.ap_clip_resnet_config_init(C.byref(cfg), 32) == _lib.AP_ERR_INVALID
    assert L.ap_clip_resnet_config_init(C.byref(cfg), C.sizeof(cfg)) == 0 and cfg.struct_size == 36 and cfg.width == 0
