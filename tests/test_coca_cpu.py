"""omiclip and conch_v15 on the host: the restatements of tests/coca_reference.py against the checkpoint adapters and the
independent canonical forward, every checkpoint layout, the mistakes a checkpoint can hold, the plugin and the registry, the
seeded random init, the 112-byte structure -- and the check that makes the device test mean something: each of the four fields
of ``ap_vit_config_ex2`` changes the reference output by more than ten times the loosest device tolerance."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import coca_reference as R


@pytest.fixture(scope="module")
def towers():
    """name -> (module, arch, x, the module's own float32 output, canonical state dict): computed once, left unchanged."""
    from atlaspatch_amd.encoders.vit import coca_canonical_state_dict, conch_v15_canonical_state_dict
    out = {}
    model, arch = R.tiny_coca()
    x = R.images(3, arch["image_size"])
    with torch.inference_mode():
        want = model.encode_image(x)
    out["omiclip"] = (model, arch, x, want, coca_canonical_state_dict(dict(model.state_dict()), arch))
    model, arch = R.tiny_conch()
    x = R.images(3, arch["image_size"])
    with torch.inference_mode():
        want = model(x)
    canon, layer_scale = conch_v15_canonical_state_dict(dict(model.state_dict()), arch)
    assert layer_scale is True
    out["conch_v15"] = (model, arch, x, want, canon)
    return out


@pytest.mark.parametrize("name", ["omiclip", "conch_v15"])
def test_module_forward_equals_adapter_plus_canonical_forward(towers, name):
    """Two independent statements of the same network: nn.MultiheadAttention on the packages' key names against plain matrix
    products on the canonical names the adapter produced.  float32 both, norm-wise; and float64 against float64 far below."""
    model, arch, x, want, canon = towers[name]
    got = R.canonical_forward(canon, x, arch, torch.float32)
    r = R.rel(got, want)
    print(f"{name}: module vs adapter + canonical forward, float32: {r:.3e}")
    assert tuple(got.shape) == tuple(want.shape) == (3, 384) and r <= 1e-5
    m64 = copy.deepcopy(model).double()
    with torch.inference_mode():
        want64 = m64.encode_image(x.double()) if name == "omiclip" else m64(x.double())
    assert R.rel(R.canonical_forward(canon, x, arch), want64) <= 1e-6     # the float32 checkpoint's query fold is float64 -> float32


def test_omiclip_rows_have_unit_norm_and_ignore_the_caption_queries(towers):
    from atlaspatch_amd.encoders.vit import coca_canonical_state_dict
    model, arch, x, want, canon = towers["omiclip"]
    assert torch.allclose(want.norm(dim=-1), torch.ones(3), atol=1e-6)
    got = R.canonical_forward(canon, x, arch, torch.float32)
    assert torch.allclose(got.norm(dim=-1), torch.ones(3), atol=1e-6)
    sd = dict(model.state_dict())
    assert sd["visual.attn_pool.query"].shape[0] > 1
    other = dict(sd)
    q = sd["visual.attn_pool.query"].clone()
    q[1:] = torch.randn(q[1:].shape, generator=torch.Generator().manual_seed(9)) * 3.0
    other["visual.attn_pool.query"] = q
    canon2 = coca_canonical_state_dict(other, arch)
    assert canon2.keys() == canon.keys() and all(torch.equal(canon2[k], canon[k]) for k in canon)
    again = R.canonical_forward(canon2, x, arch, torch.float32)
    assert np.array_equal(again.numpy().view(np.uint32), got.numpy().view(np.uint32))
    # ... while the module itself does read them (its second output), so the rows are not dead weight in the restatement
    changed = copy.deepcopy(model)
    changed.load_state_dict(other)
    with torch.inference_mode():
        assert torch.equal(changed.encode_image(x), want) and not torch.equal(changed.visual(x)[1], model.visual(x)[1])


def test_every_key_layout_loads(towers):
    from atlaspatch_amd.encoders.vit import coca_canonical_state_dict, conch_state_dicts, conch_v15_canonical_state_dict
    model, arch, _, _, canon = towers["omiclip"]
    whole = dict(model.state_dict())
    assert any(k.startswith("text.") for k in whole) and any(k.startswith("text_decoder.") for k in whole) and "logit_scale" in whole
    prefixed = {k: v for k, v in whole.items() if k.startswith("visual.")}
    bare = {k[len("visual."):]: v for k, v in prefixed.items()}
    for layout in (whole, prefixed, bare):
        got = coca_canonical_state_dict(layout, arch)
        assert got.keys() == canon.keys() and all(torch.equal(got[k], canon[k]) for k in canon)
    assert "norm.weight" not in canon and float(canon["patch_embed.bias"].abs().max()) == 0.0
    assert torch.equal(canon["attn_pool.proj.weight"], whole["visual.proj"].t())
    model, arch, _, _, canon = towers["conch_v15"]
    bare = dict(model.state_dict())
    for prefix in ("", "visual.", "vision_encoder."):
        layout = {prefix + k: v for k, v in bare.items()}
        got, layer_scale = conch_v15_canonical_state_dict(layout, arch)
        assert layer_scale and got.keys() == canon.keys() and all(torch.equal(got[k], canon[k]) for k in canon)
        trunk, pool = conch_state_dicts(layout)
        assert "blocks.0.attn.qkv.weight" in trunk and "query" in pool and "ln_out.weight" in pool


def test_a_checkpoint_without_layerscale_builds_a_model_without_it():
    from atlaspatch_amd.encoders.vit import conch_v15_canonical_state_dict
    model, arch = R.tiny_conch(layer_scale=False)
    assert arch["layer_scale"] is False and not any("gamma" in k for k in model.state_dict())
    x = R.images(2, arch["image_size"])
    canon, layer_scale = conch_v15_canonical_state_dict(dict(model.state_dict()), dict(arch, layer_scale=True))
    assert layer_scale is False and "blocks.0.ls1" not in canon
    with torch.inference_mode():
        want = model(x)
    assert R.rel(R.canonical_forward(canon, x, arch, torch.float32), want) <= 1e-5


def test_checkpoint_mistakes_name_the_key(towers):
    from atlaspatch_amd.encoders.vit import coca_canonical_state_dict, conch_v15_canonical_state_dict
    model, arch, _, _, _ = towers["omiclip"]
    sd = dict(model.state_dict())
    with pytest.raises(ValueError, match=r"unknown key.*extra\.weight"):
        coca_canonical_state_dict({**sd, "visual.extra.weight": torch.zeros(1)}, arch)
    with pytest.raises(ValueError, match=r"missing key.*blocks\.1\.ln2\.bias.*transformer\.resblocks\.1\.ln_2\.bias"):
        coca_canonical_state_dict({k: v for k, v in sd.items() if k != "visual.transformer.resblocks.1.ln_2.bias"}, arch)
    with pytest.raises(ValueError, match=r"missing key.*attn_pool\.q.*attn_pool\.ln_q\.weight"):
        coca_canonical_state_dict({k: v for k, v in sd.items() if k != "visual.attn_pool.ln_q.weight"}, arch)
    with pytest.raises(ValueError, match=r"missing key.*attn_pool\.proj\.weight.*proj"):
        coca_canonical_state_dict({k: v for k, v in sd.items() if k != "visual.proj"}, arch)
    with pytest.raises(ValueError, match=r"attn_pool\.attn\.k_proj_weight has shape \(384, 255\)"):
        coca_canonical_state_dict({**sd, "visual.attn_pool.attn.k_proj_weight": torch.zeros(384, 255)}, arch)
    with pytest.raises(ValueError, match=r"pos_embed has shape \(6, 256\)"):
        coca_canonical_state_dict({**sd, "visual.positional_embedding": torch.zeros(6, 256)}, arch)
    model, arch, _, _, _ = towers["conch_v15"]
    sd = dict(model.state_dict())
    with pytest.raises(ValueError, match=r"missing key.*norm\.weight.*trunk\.norm\.weight"):
        conch_v15_canonical_state_dict({k: v for k, v in sd.items() if k != "trunk.norm.weight"}, arch)
    with pytest.raises(ValueError, match=r"missing key.*blocks\.1\.ls2.*trunk\.blocks\.1\.ls2\.gamma"):
        conch_v15_canonical_state_dict({k: v for k, v in sd.items() if k != "trunk.blocks.1.ls2.gamma"}, arch)
    with pytest.raises(ValueError, match=r"ln_contrast\.weight has shape \(383,\)"):
        conch_v15_canonical_state_dict({**sd, "ln_contrast.weight": torch.zeros(383)}, arch)
    with pytest.raises(ValueError, match=r"unknown key.*attn_pool_caption\.query"):
        conch_v15_canonical_state_dict({**sd, "attn_pool_caption.query": torch.zeros(1)}, arch)


def test_plugin_registers_exactly_the_two_names_and_leaves_the_default_registry_alone():
    from atlaspatch_amd.encoders import build_default_registry
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry as FeatureExtractorRegistry
    before = build_default_registry(device="cpu").available()
    import atlaspatch_amd.plugins.coca_towers as plugin
    reg = FeatureExtractorRegistry()
    plugin.register_feature_extractors(reg, torch.device("cpu"), torch.float16, 0)
    assert set(reg.available()) == {"omiclip", "conch_v15"}
    assert build_default_registry(device="cpu").available() == before and not {"omiclip", "conch_v15"} & set(before)
    # all six plugins in one registry
    import atlaspatch_amd.plugins.chief_ctranspath as chief
    import atlaspatch_amd.plugins.medsiglip as medsiglip
    import atlaspatch_amd.plugins.openai_clip_resnets as clip_resnets
    import atlaspatch_amd.plugins.torchvision_convnexts as convnext
    import atlaspatch_amd.plugins.torchvision_resnets as resnet
    for other in (resnet, convnext, chief, medsiglip, clip_resnets):
        other.register_feature_extractors(reg, torch.device("cpu"), torch.float16, 0)
    names = reg.available()
    assert {"omiclip", "conch_v15", "medsiglip", "chief-ctranspath", "clip_rn50"} <= set(names) and len(names) == len(set(names))


def test_conch_v15_float32_is_refused_before_any_device_work(monkeypatch):
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry as FeatureExtractorRegistry
    import atlaspatch_amd.plugins.coca_towers as plugin
    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "3")
    reg = FeatureExtractorRegistry()
    plugin.register_feature_extractors(reg, torch.device("cpu"), torch.float32, 0)       # a CPU device: device work would raise another error
    with pytest.raises(ValueError, match=r"conch_v15.*float32.*785 tokens.*float16 or bfloat16"):
        reg.create("conch_v15")


def test_random_init_builds_the_canonical_shapes():
    from atlaspatch_amd.encoders.vit import ARCHS, TRANSFORM_NORM, TRANSFORM_RESIZE, attn_tower_canonical_shapes, random_canonical_state_dict
    o, c = ARCHS["omiclip"], ARCHS["conch_v15"]
    assert (o["dim"], o["depth"], o["heads"], o["mlp_dim"], o["image_size"], o["patch_size"]) == (1024, 24, 16, 4096, 224, 14)
    assert (c["dim"], c["depth"], c["heads"], c["mlp_dim"], c["image_size"], c["patch_size"]) == (1024, 24, 16, 4096, 448, 16)
    for a in (o, c):
        assert (a["pool_dim"], a["pool_heads"], a["pool_head_dim"], a["pool_ln_eps"]) == (768, 8, 96, 1e-5)
    assert o["pre_norm"] and o["pool_skip_final_norm"] and o["pool_proj_dim"] == 768 and o["out_normalize"] and o["ln_eps"] == 1e-5
    assert c["layer_scale"] and c["ln_eps"] == 1e-6 and not any(c.get(k) for k in ("pre_norm", "pool_skip_final_norm", "pool_proj_dim", "out_normalize"))
    assert TRANSFORM_RESIZE["omiclip"] == (224, "bicubic") and TRANSFORM_RESIZE["conch_v15"] == (448, "bicubic")
    assert TRANSFORM_NORM["omiclip"][0][0] == pytest.approx(0.48145466) and TRANSFORM_NORM["conch_v15"][0][0] == pytest.approx(0.485)
    for name in ("omiclip", "conch_v15"):
        arch = dict(ARCHS[name], depth=2)
        sd = random_canonical_state_dict(arch, seed=5)
        want = attn_tower_canonical_shapes(arch)
        assert sd.keys() == want.keys() and all(tuple(sd[k].shape) == shape for k, shape in want.items())
        again = random_canonical_state_dict(arch, seed=5)
        assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert want["pos_embed"] == (785, 1024) and "blocks.1.ls2" in want and "attn_pool.proj.weight" not in want


def test_the_second_extension_is_112_bytes_and_the_others_keep_their_sizes():
    from atlaspatch_amd import _lib
    assert C.sizeof(_lib.VitConfig) == 92 and C.sizeof(_lib.VitConfigEx) == 96 and C.sizeof(_lib.VitConfigEx2) == 112
    cfg = _lib.VitConfigEx2(image_size=28, pool_head_dim=96, out_normalize=1)
    assert cfg.struct_size == 112 and cfg.image_size == 28 and cfg.no_class_token == 0 and cfg.pool_head_dim == 96
    assert [n for n, _ in _lib.VitConfigEx2._fields_] == list(R.FIELDS)
    assert _lib.VitConfigEx2.pool_head_dim.offset == 96 and _lib.VitConfigEx2.out_normalize.offset == 108


@pytest.mark.parametrize("form", ["coca", "conch"])
@pytest.mark.parametrize("width", [64, 96, 128])
def test_each_new_field_shows_in_the_reference_far_above_the_device_tolerance(form, width):
    """A field the engine silently ignored would give the untoggled output: with these weights (``R.full_state``) that is more than
    10 x the loosest device bound (bfloat16: 3e-2) away from the reference, for each field, form and pool head width."""
    _, arch = R.tiny_coca() if form == "coca" else R.tiny_conch()
    arch = dict(arch, pool_head_dim=width, pool_heads=arch["pool_dim"] // width)
    state = R.full_state(arch, seed=11 if form == "coca" else 12)
    x = R.images(3, arch["image_size"])
    base = R.canonical_forward(state, x, arch)
    floor = 10 * max(R.TOL.values())
    for field in R.FIELDS:
        r = R.rel(R.canonical_forward(state, x, R.toggled(arch, field)), base)
        print(f"{form} width {width}: {field} toggled moves the reference by {r:.3f} (floor {floor})")
        assert r > floor, (form, width, field, r)


# ----------------------------------------------------------------------------- head_dim and the class readouts of the reference
def _narrow_arch(head_dim, pool):
    arch = dict(image_size=64, patch_size=16, dim=512, depth=2, heads=2, head_dim=head_dim, mlp_dim=512, ln_eps=1e-6, layer_scale=False)
    if pool == "attn":
        arch.update(pool="attn", pool_dim=256, pool_heads=4, pool_ln_eps=1e-5, pool_head_dim=64)
    elif pool:
        arch["pool"] = pool
    return arch


@pytest.mark.parametrize("pool", [None, "cls_mean", "attn"])
def test_reference_moves_with_head_dim(pool):
    """tests/test_gpu_engine_workspace.py compares the engine at heads * head_dim < dim with ``canonical_forward``: the reference
    must use the field.  Two heads of 64 in a 512-wide stream against the same tensors read as four heads of 32 (head_dim is all
    that tells them apart): more than 0.3 apart norm-wise, ten times the loosest device bound.  head_dim = dim / heads
    spelled out is the old forward bit for bit, and the class-token readout is the first half of "cls_mean"."""
    x = R.images(3, 64)
    narrow = _narrow_arch(64, pool)
    full = R.full_state(narrow, seed=41)
    assert tuple(full["blocks.0.qkv.weight"].shape) == (384, 512) and tuple(full["blocks.1.proj.weight"].shape) == (512, 128)
    want = R.canonical_forward(R.select(full, narrow), x, narrow)
    assert tuple(want.shape) == (3, {None: 512, "cls_mean": 1024, "attn": 256}[pool]) and bool(torch.isfinite(want).all())
    regrouped = dict(narrow, heads=4, head_dim=32)       # the same tensors read as four heads of 32: other groups, other scale
    moved = R.rel(R.canonical_forward(R.select(full, regrouped), x, regrouped), want)
    print(f"2 heads of 64 -> 4 heads of 32 on the same tensors, pool {pool}: the reference moves by {moved:.3f}")
    assert moved > 0.3
    implicit = {k: v for k, v in _narrow_arch(256, pool).items() if k != "head_dim"}
    st = R.full_state(implicit, seed=42)
    a = R.canonical_forward(R.select(st, implicit), x, implicit)
    b = R.canonical_forward(R.select(st, implicit), x, dict(implicit, head_dim=256))
    assert torch.equal(a, b)
    if pool == "cls_mean":
        cls = R.canonical_forward(R.select(full, narrow), x, {k: v for k, v in narrow.items() if k != "pool"})
        assert torch.equal(want[:, :512], cls)
