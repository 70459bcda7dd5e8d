"""The SigLIP vision tower off the GPU: the hf_siglip checkpoint adapter and the torch restatement of the canonical form
(tests/siglip_reference.py) against transformers' SiglipVisionModel itself, the padding rules, the acceptance check of the two new
operators (it can fail: every listed mistake is refused on the shapes tests/test_gpu_siglip.py uses), and the plugin's registry,
checkpoint and preprocess handling."""
import json
import math

import numpy as np
import pytest
import torch

from tests import siglip_reference as S

CONFIGS = {"tiny": dict(hidden=256, heads=4, inter=600, layers=2, image=64, patch=16),            # mlp stored 640
           "so400m-width": dict(hidden=1152, heads=16, inter=4304, layers=2, image=56, patch=14)}  # heads 72 -> 96, mlp -> 4352


@pytest.fixture(scope="module")
def models():
    """name -> (HF model, arch, x float32 [3, 3, S, S], its pooler_output): built once, shared, left unchanged."""
    out = {}
    for name, c in CONFIGS.items():
        model, arch = S.hf_siglip(**c)
        x = torch.randn(3, 3, c["image"], c["image"], generator=torch.Generator().manual_seed(2))
        with torch.inference_mode():
            want = model(pixel_values=x).pooler_output
        out[name] = (model, arch, x, want)
    return out


def _layouts(model, arch):
    """The three key layouts of a SigLIP checkpoint: bare, `vision_model.`-prefixed, a whole SiglipModel with its text tower."""
    from transformers import SiglipConfig, SiglipModel, SiglipTextConfig
    bare = dict(model.state_dict())
    yield "bare", bare
    yield "prefixed", {"vision_model." + k: v for k, v in bare.items()}
    text = SiglipTextConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1, vocab_size=100,
                            bos_token_id=1, eos_token_id=2, pad_token_id=0)
    whole = SiglipModel(SiglipConfig(text_config=text.to_dict(), vision_config=model.config.to_dict())).eval()
    sd = dict(whole.state_dict())
    assert any(k.startswith("text_model.") for k in sd) and "logit_scale" in sd and "logit_bias" in sd
    for k, v in bare.items():
        assert "vision_model." + k in sd and sd["vision_model." + k].shape == v.shape
        sd["vision_model." + k] = v
    yield "whole", sd


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_adapter_and_restatement_match_the_hf_model(models, name):
    """Adapter output -> stored padding -> the restatement in float64 == SiglipVisionModel.pooler_output (float32) to 1e-5
    norm-wise, from each of the three key layouts (which must give the same canonical tensors bit for bit)."""
    from atlaspatch_amd.encoders.vit import _detect_source, siglip_canonical_state_dict, stored_mlp_dim
    model, arch, x, want = models[name]
    first = None
    for layout, sd in _layouts(model, arch):
        assert _detect_source(sd) == "hf_siglip", layout
        canon = siglip_canonical_state_dict(sd, arch)
        if first is None:
            first = canon
            continue
        assert canon.keys() == first.keys() and all(S.same_bits(canon[k], first[k]) for k in first), layout
    stored = S.stored_state(first, arch)
    hd = arch["dim"] // arch["heads"]
    assert stored["blocks.0.fc1.weight"].shape[0] == stored["map.fc1.weight"].shape[0] == stored_mlp_dim(arch["mlp_dim"])
    got = S.siglip_forward(stored, x.double(), heads=arch["heads"], depth=arch["depth"], scale=1.0 / math.sqrt(hd))
    assert got.shape == want.shape == (3, arch["dim"])
    r = S.rel(got.numpy(), want.numpy())
    print(f"{name}: restatement (float64, stored form) vs HF float32: {r:.3e}")
    assert r <= 1e-5


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_head_and_mlp_padding_leave_the_function_unchanged(models, name):
    """Bit for bit in float64 on the restatement: zero q / k channels add exact zeros to q . k, zero v channels meet zero proj
    columns, padded fc1 rows give gelu_tanh(0) = 0 against zero fc2 columns.  (With every product summed in index order: a
    blocked sum regroups the non-zero terms when zeros are inserted, which is the sum's business, not the padding's.)"""
    from atlaspatch_amd.encoders.vit import siglip_canonical_state_dict
    model, arch, x, _ = models[name]
    canon = siglip_canonical_state_dict(dict(model.state_dict()), arch)
    stored = S.stored_state(canon, arch)
    scale = 1.0 / math.sqrt(arch["dim"] // arch["heads"])
    a = S.siglip_forward(canon, x.double(), heads=arch["heads"], depth=arch["depth"], scale=scale, mm=S.mm_sequential)
    b = S.siglip_forward(stored, x.double(), heads=arch["heads"], depth=arch["depth"], scale=scale, mm=S.mm_sequential)
    if name == "so400m-width":
        assert stored["map.q"].shape[0] == 16 * 96 and stored["blocks.0.qkv.weight"].shape[0] == 3 * 16 * 96
    assert stored["map.fc2.weight"].shape[1] % 128 == 0
    assert torch.equal(a, b)
    fast = S.siglip_forward(stored, x.double(), heads=arch["heads"], depth=arch["depth"], scale=scale)
    assert S.rel(fast.numpy(), a.numpy()) <= 1e-13               # the index-order sums and torch's are the same function
    assert float(S.gelu_tanh(torch.zeros(1, dtype=torch.float64))) == 0.0


def test_gelu_tanh_restatement_is_torchs():
    x = torch.cat([torch.linspace(-12, 12, 4801, dtype=torch.float64), torch.tensor([0.0, -0.0, 65504.0, -65504.0], dtype=torch.float64)])
    want = torch.nn.functional.gelu(x, approximate="tanh")
    assert float((S.gelu_tanh(x) - want).abs().max()) <= 1e-15
    # the sigmoid form the kernels evaluate is the same function
    z = 2.0 * S.SQRT_2_OVER_PI * (x + 0.044715 * x ** 3)
    assert float((x * torch.sigmoid(z) - want).abs().max()) <= 1e-14
    assert float(S.gelu_tanh(torch.tensor(65504.0, dtype=torch.float64))) == 65504.0
    assert float(S.gelu_tanh(torch.tensor(-65504.0, dtype=torch.float64))) == 0.0


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_hf_reference_refuses_every_listed_mistake(models, name):
    """At the shapes of the device test (n = 3, 16 tokens) the 16-bit bound of that test -- the loosest one used, bfloat16's 3e-2
    at the tiny shape, and the HF model's own half-precision error times 1.5 at the real width -- is far below what each mistake
    costs: every mutation of the restatement moves the features by more than 3e-2 norm-wise, except the erf GELU, which only
    the float32 bound (2e-5) can tell from the tanh form."""
    from atlaspatch_amd.encoders.vit import siglip_canonical_state_dict
    model, arch, x, want = models[name]
    stored = S.stored_state(siglip_canonical_state_dict(dict(model.state_dict()), arch), arch)
    hd = arch["dim"] // arch["heads"]
    hd_stored = stored["map.q"].shape[0] // arch["heads"]
    moved = {}
    for m in S.HEAD_MUTATIONS + S.EMBED_MUTATIONS:
        if m == "scale_of_stored_width" and hd_stored == hd:
            continue                                     # the tiny shape stores its 64-wide heads unpadded: nothing to confuse
        got = S.siglip_forward(stored, x.double(), heads=arch["heads"], depth=arch["depth"], scale=1.0 / math.sqrt(hd), mutate=m)
        moved[m] = S.rel(got.numpy(), want.numpy())
    print(name, {k: f"{v:.2e}" for k, v in moved.items()})
    for m, r in moved.items():
        assert r > (2e-5 if m == "erf_gelu" else 3e-2), (m, r)
    if name == "so400m-width":
        assert "scale_of_stored_width" in moved


MUTATIONS = {"gemm_gelu_tanh": S.GEMM_MUTATIONS, "attention_probe": S.PROBE_MUTATIONS}


def _as_output(outs):
    return {name: o.value.to(o.dtype) for name, o in outs.items()}


@pytest.mark.parametrize("op", sorted(S.REFS))
def test_float32_evaluation_passes_and_every_mutation_is_rejected(op):
    """The discipline of tests/test_vit_ops_reference.py for the two new operators, on the cases tests/test_gpu_siglip.py runs; also
    holds K_OP to its rule (constant = 4 x the float32 evaluation's measured error, rounded up)."""
    ref = S.REFS[op]
    seen, measured, measured_hot, count = set(), 0.0, 0.0, 0
    for case in S.CASES[op]():
        count += 1
        want = ref(case.args, torch.float64)
        got32 = ref(case.args, torch.float32)
        for name, o in want.items():
            measured = max(measured, S.measure_k(got32[name], o))
            measured_hot = max(measured_hot, S.measure_k(got32[name], o, hot=True))
            bad = S.failures(got32[name].value.to(o.dtype), o, S.k_of(op, o))
            assert bad == 0, f"{op} {case.id}: the float32 evaluation fails the check on `{name}` ({bad} elements)"
        for m in case.mutations:
            got = _as_output(ref(case.args, torch.float64, m))
            bad = sum(S.failures(got[name], o, S.k_of(op, o)) for name, o in want.items())
            assert bad > 0, f"{op} {case.id}: mutation {m} passes the check -- the inputs are too weak"
            seen.add(m)
    assert count > 0 and seen == set(MUTATIONS[op]), (op, set(MUTATIONS[op]) - seen)
    for key, value in ((op, measured), (op + "_hot", measured_hot)):
        if key in S.K_OP:
            recorded, constant = S.K_OP[key]
            print(f"k_op {key}: measured {value:.3f}, recorded {recorded}, constant {constant}")
            assert constant == math.ceil(4 * recorded), "the constant is 4 x the recorded measurement, rounded up"
            assert 0.67 * recorded <= value <= 1.5 * recorded, f"{key}: the float32 evaluation measures {value:.3f}: record it"
    assert (op + "_hot" in S.K_OP) == (measured_hot > 0)


def test_gemm_inputs_hold_what_the_contract_names():
    """Pre-activations out to +-12, an exact 0 and the 16-bit extremes, where the function is x and -0."""
    for case in S.cases_gemm_gelu_tanh():
        a = case.args
        C = a["A"].double() @ a["W"].double().T + a["bias"].double() if not a["norm"] else None
        out = S.ref_gemm_gelu_tanh(a)["out"].value
        ext = S.EXTREME[a["dtype"]]
        if C is not None:
            assert float(C[0, 0]) == 0.0 and float(C[1, 2]) == ext and float(C[1, 3]) == -ext
            body = C[2:]
            assert float(body.min()) < -12.0 and float(body.max()) > 12.0
        assert float(out[0, 0]) == 0.0 and float(out[1, 2]) == ext and float(out[1, 3]) == 0.0 and math.copysign(1.0, float(out[1, 3])) == -1.0
        assert bool(torch.isfinite(out).all())


# ----------------------------------------------------------------------------- plugin, registry, checkpoints, preprocess
def test_plugin_registers_exactly_medsiglip_and_leaves_the_default_registry_alone():
    from atlaspatch_amd.encoders import build_default_registry
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry as FeatureExtractorRegistry
    before = build_default_registry(device="cpu").available()
    import atlaspatch_amd.plugins.medsiglip as plugin
    reg = FeatureExtractorRegistry()
    plugin.register_feature_extractors(reg, torch.device("cpu"), torch.float16, 0)
    assert reg.available() == ["medsiglip"]
    assert build_default_registry(device="cpu").available() == before and "medsiglip" not in before
    # one registry shared with the three existing plugins
    import atlaspatch_amd.plugins.chief_ctranspath as chief
    import atlaspatch_amd.plugins.torchvision_convnexts as convnext
    import atlaspatch_amd.plugins.torchvision_resnets as resnet
    for other in (resnet, convnext, chief):
        other.register_feature_extractors(reg, torch.device("cpu"), torch.float16, 0)
    names = reg.available()
    assert "medsiglip" in names and "chief-ctranspath" in names and len(names) == len(set(names)) > 3


def test_float32_at_the_real_size_is_refused_at_create():
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry as FeatureExtractorRegistry
    import atlaspatch_amd.plugins.medsiglip as plugin
    reg = FeatureExtractorRegistry()
    plugin.register_feature_extractors(reg, torch.device("cpu"), torch.float32, 0)
    with pytest.raises(ValueError, match="float32.*float16 or bfloat16"):
        reg.create("medsiglip")


def test_checkpoint_mistakes_name_the_key(models):
    from atlaspatch_amd.encoders.vit import siglip_canonical_state_dict
    model, arch, _, _ = models["tiny"]
    sd = dict(model.state_dict())
    with pytest.raises(ValueError, match=r"unknown key.*head\.extra\.weight"):
        siglip_canonical_state_dict({**sd, "head.extra.weight": torch.zeros(1)}, arch)
    with pytest.raises(ValueError, match=r"missing key.*blocks\.1\.ln2\.bias.*encoder\.layers\.1\.layer_norm2\.bias"):
        siglip_canonical_state_dict({k: v for k, v in sd.items() if k != "encoder.layers.1.layer_norm2.bias"}, arch)
    with pytest.raises(ValueError, match=r"missing key.*map\.q.*head\.probe"):
        siglip_canonical_state_dict({k: v for k, v in sd.items() if k != "head.probe"}, arch)
    with pytest.raises(ValueError, match=r"map\.fc2\.weight has shape \(256, 601\)"):
        siglip_canonical_state_dict({**sd, "head.mlp.fc2.weight": torch.zeros(256, 601)}, arch)
    with pytest.raises(ValueError, match=r"pos_embed has shape \(17, 256\)"):
        siglip_canonical_state_dict({**sd, "embeddings.position_embedding.weight": torch.zeros(17, 256)}, arch)


def test_random_init_builds_the_canonical_shapes():
    from atlaspatch_amd.encoders.vit import ARCHS, random_canonical_state_dict, siglip_canonical_shapes
    arch = dict(ARCHS["medsiglip"], depth=2)
    assert (ARCHS["medsiglip"]["dim"], ARCHS["medsiglip"]["depth"], ARCHS["medsiglip"]["heads"], ARCHS["medsiglip"]["mlp_dim"],
            ARCHS["medsiglip"]["image_size"], ARCHS["medsiglip"]["patch_size"]) == (1152, 27, 16, 4304, 448, 14)
    sd = random_canonical_state_dict(arch, seed=5)
    want = siglip_canonical_shapes(arch)
    assert sd.keys() == want.keys() and "cls_token" not in sd
    assert all(tuple(sd[k].shape) == shape for k, shape in want.items())
    assert want["pos_embed"] == (1024, 1152)
    again = random_canonical_state_dict(arch, seed=5)
    assert all(S.same_bits(sd[k], again[k]) for k in sd)


def test_preprocessor_json_overrides_the_filter_and_the_constants(tmp_path):
    from atlaspatch_amd.encoders.vit import medsiglip_transform
    assert medsiglip_transform(str(tmp_path)) == (448, "bilinear", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    (tmp_path / "medsiglip.preprocessor_config.json").write_text(json.dumps(
        {"size": {"height": 448, "width": 448}, "resample": 3, "image_mean": [0.4, 0.5, 0.6], "image_std": [0.2, 0.3, 0.4],
         "do_rescale": True}))
    assert medsiglip_transform(str(tmp_path)) == (448, "bicubic", (0.4, 0.5, 0.6), (0.2, 0.3, 0.4))
    (tmp_path / "medsiglip.preprocessor_config.json").write_text(json.dumps({"resample": 0}))
    with pytest.raises(ValueError, match="resample 0"):
        medsiglip_transform(str(tmp_path))
