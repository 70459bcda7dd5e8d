"""omiclip and conch_v15 on the device: ap_l2_normalize_rows per element against float64; the engine with the fields of
ap_vit_config_ex2 (pool head widths 64 / 96 / 128 on the one-query kernel, ln_k straight on the residual stream, the projection
after the pooler, normalised rows, the pooler in float32) against the float64 restatements of tests/coca_reference.py at the
smallest sizes that reach every path; conch_v1 bit for bit through the old and the new structure; ap_vit_create's refusals;
the real width against the restatement's own 16-bit error; and the plugin end to end."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import coca_reference as R
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu

TOL = R.TOL

# Width 1024, 2 blocks, pool 768 = 8 x 96, n = 3, against the restatement in float32 on the CPU, norm-wise: (name, dtype) -> (the
# restatement ITSELF in that 16-bit type on the CPU, this engine on the MI355X).  The bound is 1.5 x the first.
MEASURED = {
    ("omiclip", "float16"): (9.486e-4, 6.647e-4),
    ("omiclip", "bfloat16"): (7.426e-3, 5.368e-3),
    ("conch_v15", "float16"): (1.109e-3, 7.521e-4),
    ("conch_v15", "bfloat16"): (8.203e-3, 5.718e-3),
}


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    return _lib, _lib.load(), dev, _lib.current_stream_ptr(dev)


# ----------------------------------------------------------------------------- ap_l2_normalize_rows
def _l2_input(rows, dim, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, dim, generator=g) * torch.logspace(-3, 3, rows).reshape(rows, 1)      # norms over six decades
    return x


@pytest.mark.parametrize("dim", R.L2_DIMS)
@pytest.mark.parametrize("rows", R.L2_ROWS)
def test_l2_normalize_rows_per_element(env, rows, dim):
    """Dense, strided and in place; every element within 4 * 2^-24 relative of the float64 quotient (the norm's rounding and the
    division's are 2 * 2^-24 together); the guard bands around the output stay as they were."""
    _lib, lib, dev, stream = env
    eps = 1e-12
    x = _l2_input(rows, dim, 100 * rows + dim)
    want = R.l2_normalize_ref(x, eps)
    for stride in (dim, dim + 12):
        src = torch.full((rows, stride), float("nan"))
        src[:, :dim] = x
        xs = src.to(dev)
        out = Guarded((rows, dim), torch.float32, dev)
        _lib.check(lib.ap_l2_normalize_rows(xs.data_ptr(), stride, rows, dim, eps, out.ptr(), stream), "ap_l2_normalize_rows")
        torch.cuda.synchronize()
        got = out.cpu().double()
        err = ((got - want).abs() / want.abs().clamp_min(1e-300)).max()
        print(f"l2_normalize rows {rows} dim {dim} stride {stride}: worst relative error {float(err) / 2.0 ** -24:.2f} x 2^-24")
        assert float(err) <= 4 * 2.0 ** -24
        assert torch.equal(xs.cpu()[:, :dim], x)                        # the input is read only
    inplace = Guarded((rows, dim), torch.float32, dev, init=x)
    _lib.check(lib.ap_l2_normalize_rows(inplace.ptr(), dim, rows, dim, eps, inplace.ptr(), stream), "ap_l2_normalize_rows")
    torch.cuda.synchronize()
    assert torch.equal(inplace.cpu().double(), got)                     # the same bits as the out-of-place call


def test_l2_normalize_zero_and_tiny_rows_never_become_nan(env):
    _lib, lib, dev, stream = env
    x = torch.zeros(3, 128)
    x[1, 5] = 1e-20                                                     # norm below eps: divided by eps
    x[2] = torch.randn(128, generator=torch.Generator().manual_seed(1))
    out = Guarded((3, 128), torch.float32, dev)
    _lib.check(lib.ap_l2_normalize_rows(x.to(dev).data_ptr(), 128, 3, 128, 1e-12, out.ptr(), stream), "ap_l2_normalize_rows")
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[0] == 0).all()) and not bool(torch.isnan(got).any())
    assert float(got[1, 5]) == pytest.approx(1e-8, rel=1e-6) and float(got[1].abs().sum()) == float(got[1, 5])
    assert float(got[2].double().norm()) == pytest.approx(1.0, abs=1e-6)


def test_l2_normalize_refusals_launch_nothing(env):
    _lib, lib, dev, stream = env
    x = torch.ones(4, 128, device=dev)
    out = Guarded((4, 128), torch.float32, dev)
    call = lambda **kw: lib.ap_l2_normalize_rows(*[{**dict(x=x.data_ptr(), stride=128, rows=4, dim=128, eps=1e-12, out=out.ptr(), stream=stream), **kw}[k]
                                                   for k in ("x", "stride", "rows", "dim", "eps", "out", "stream")])
    for what, kw in (("null x", dict(x=None)), ("null out", dict(out=None)), ("misaligned x", dict(x=x.data_ptr() + 4)),
                     ("misaligned out", dict(out=out.ptr() + 8)), ("dim % 4", dict(dim=126)), ("dim 0", dict(dim=0)),
                     ("negative rows", dict(rows=-1)), ("stride below dim", dict(stride=64)), ("stride % 4", dict(stride=130)),
                     ("eps 0", dict(eps=0.0)), ("in place on strided rows", dict(out=x.data_ptr(), stride=256, rows=2))):
        rc = call(**kw)
        msg = lib.ap_last_error().decode()
        assert rc == _lib.AP_ERR_INVALID and "ap_l2_normalize_rows" in msg, (what, rc, msg)
    assert call(rows=0) == 0                                           # an empty launch
    torch.cuda.synchronize()
    assert out.untouched()
    assert call() == 0
    torch.cuda.synchronize()
    assert not out.untouched() and float(out.cpu()[0, 0]) == pytest.approx(128 ** -0.5, rel=1e-6)


# ----------------------------------------------------------------------------- the engine at the smallest sizes
def _device_features(arch, state, x, dtype, **options):
    from atlaspatch_amd.encoders.vit import HipViT
    dev = torch.device("cuda:0")
    vit = HipViT(arch, state, device=dev, dtype=dtype)
    assert vit.embed_dim == (arch.get("pool_proj_dim") or arch["pool_dim"])
    assert int(vit.lib.ap_vit_embed_dim(vit._handle)) == vit.embed_dim
    for name, on in options.items():
        vit.set_option(name, on)
    got = vit.forward_chw(x.to(dev).contiguous())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    vit.release()
    return got


@pytest.fixture(scope="module")
def forms():
    """form -> (arch, canonical state dict from the adapter, x [3, 3, S, S], the restatement module's float64 output)."""
    from atlaspatch_amd.encoders.vit import coca_canonical_state_dict, conch_v15_canonical_state_dict
    out = {}
    model, arch = R.tiny_coca()
    x = R.images(3, arch["image_size"])
    with torch.inference_mode():
        want = copy.deepcopy(model).double().encode_image(x.double()).numpy()
    out["coca"] = (arch, coca_canonical_state_dict(dict(model.state_dict()), arch), x, want)
    model, arch = R.tiny_conch()
    x = R.images(3, arch["image_size"])
    with torch.inference_mode():
        want = copy.deepcopy(model).double()(x.double()).numpy()
    out["conch"] = (arch, conch_v15_canonical_state_dict(dict(model.state_dict()), arch)[0], x, want)
    return out


DATAFLOWS = [(torch.float32, False), (torch.float16, False), (torch.float16, True), (torch.bfloat16, False), (torch.bfloat16, True)]


@pytest.mark.parametrize("dtype,f32_stream", DATAFLOWS, ids=str)
@pytest.mark.parametrize("form", ["coca", "conch"])
def test_tiny_towers_vs_the_float64_restatement(forms, form, dtype, f32_stream):
    """CoCa form: dim 256, 4 heads, MLP 768, 2 blocks, 5 tokens, pre_norm, pool 384 = 4 x 96, no final norm, projection 384,
    normalised.  CONCH v1.5 form: the same trunk with LayerScale, 17 tokens, final norm kept, neither projection nor normalisation.
    n = 3, checkpoint -> adapter -> HipViT -> forward_chw, both dataflows of the 16-bit types."""
    arch, state, x, want = forms[form]
    got = _device_features(arch, state, x, dtype, **({"f32_stream": True} if f32_stream else {}))
    r = R.rel(got, want)
    print(f"PARITY {form} tiny {dtype} {'f32_stream' if f32_stream else 'default'}: norm-wise {r:.3e} (bound {TOL[dtype]:.0e})")
    assert got.shape == want.shape == (3, 384) and np.isfinite(got).all() and r <= TOL[dtype]
    if form == "coca":
        assert np.allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)


def _field_cases(width):
    """(label, arch) for one pool head width: every field off and each one alone on (CONCH v1.5's trunk), every field on and each
    one alone off (CoCa's trunk); width 64 also with pool_head_dim 0, the kernel conch_v1 runs on."""
    _, conch = R.tiny_conch()
    _, coca = R.tiny_coca()
    heads = conch["pool_dim"] // width
    off = dict(conch, pool_head_dim=width, pool_heads=heads)
    on = dict(coca, pool_head_dim=width, pool_heads=heads)
    cases = [("all off", off), ("all on", on)]
    for field in R.FIELDS[1:]:
        cases.append((f"only {field}", R.toggled(off, field)))
        cases.append((f"all but {field}", R.toggled(on, field)))
    if width == 64:
        cases.append(("pool_head_dim 0, others off", dict(off, pool_head_dim=0)))
        cases.append(("pool_head_dim 0, others on", dict(on, pool_head_dim=0)))
    return cases


@pytest.mark.parametrize("dtype,f32_stream", DATAFLOWS, ids=str)
@pytest.mark.parametrize("width", [64, 96, 128])
def test_each_field_alone_on_and_off(width, dtype, f32_stream):
    """tests/test_coca_cpu.py shows that each field moves the reference by more than 0.3 with these weights, so a field the engine
    ignored fails here.  pool_head_dim 0 (the 64-wide kernel of conch_v1) stays float16 / bfloat16 only."""
    failed = []
    for label, arch in _field_cases(width):
        if dtype == torch.float32 and not arch["pool_head_dim"]:
            continue
        full = R.full_state(arch, seed=11 if arch.get("pre_norm") else 12)
        x = R.images(3, arch["image_size"])
        want = R.canonical_forward(full, x, arch).numpy()
        got = _device_features(arch, R.select(full, arch), x, dtype, **({"f32_stream": True} if f32_stream else {}))
        r = R.rel(got, want)
        print(f"PARITY width {width} {label} {dtype} {'f32_stream' if f32_stream else 'default'}: {r:.3e} (bound {TOL[dtype]:.0e})")
        if not (got.shape == want.shape and r <= TOL[dtype]):
            failed.append((label, r))
    assert not failed, failed


@pytest.mark.parametrize("form,image,patch", [("coca", 224, 14), ("conch", 448, 16)])
def test_real_token_counts_at_depth_1(form, image, patch):
    """257 tokens (224 / 14) and 785 tokens (448 / 16), depth 1, float16: more than one pass of the one-query kernel's score loop
    (256 threads, 16 row slots) and the tiled trunk attention."""
    _, arch = R.tiny_coca() if form == "coca" else R.tiny_conch()
    arch = dict(arch, image_size=image, patch_size=patch, depth=1)
    full = R.full_state(arch, seed=21)
    x = R.images(3, image)
    want = R.canonical_forward(full, x, arch).numpy()
    got = _device_features(arch, R.select(full, arch), x, torch.float16)
    r = R.rel(got, want)
    print(f"PARITY {form} {1 + (image // patch) ** 2} tokens depth 1 float16: {r:.3e} (bound {TOL[torch.float16]:.0e})")
    assert got.shape == want.shape == (3, 384) and r <= TOL[torch.float16]


def test_omiclip_form_float32_at_257_tokens():
    """The pooler in float32 inside the float32 limits (288 tokens, 64-wide trunk heads): the f32 GEMMs and the float
    instantiation of the one-query kernel over more than one pass."""
    _, arch = R.tiny_coca()
    arch = dict(arch, image_size=224, patch_size=14, depth=1)
    full = R.full_state(arch, seed=21)
    x = R.images(3, 224)
    want = R.canonical_forward(full, x, arch).numpy()
    got = _device_features(arch, R.select(full, arch), x, torch.float32)
    r = R.rel(got, want)
    print(f"PARITY coca 257 tokens depth 1 float32: {r:.3e} (bound {TOL[torch.float32]:.0e})")
    assert r <= TOL[torch.float32]


# ----------------------------------------------------------------------------- conch_v1 is untouched
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_conch_v1_bit_identical_through_the_old_and_the_new_structure(monkeypatch, dtype):
    """A reduced conch_v1 (dim 256, 4 heads, pool 256 = 4 x 64, 17 tokens) through the 92-byte structure and through the 112-byte
    one with the four new fields zero: the same bits."""
    from atlaspatch_amd import _lib
    from atlaspatch_amd.encoders.vit import ARCHS, random_canonical_state_dict
    arch = dict(ARCHS["conch_v1"], image_size=64, dim=256, depth=2, heads=4, mlp_dim=768, pool_dim=256, pool_heads=4)
    state = random_canonical_state_dict(arch, seed=4)
    x = R.images(3, 64)
    old = _device_features(arch, state, x, dtype)
    sizes = []

    class Ex2(_lib.VitConfigEx2):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            sizes.append(self.struct_size)

    monkeypatch.setattr(_lib, "VitConfig", Ex2)
    new = _device_features(arch, state, x, dtype)
    monkeypatch.undo()
    assert sizes == [112]
    assert np.isfinite(old).all() and old.shape == (3, 256)
    assert np.array_equal(old.view(np.uint32), new.view(np.uint32))


# ----------------------------------------------------------------------------- ap_vit_create
def test_create_refuses_what_is_not_built(env):
    _lib, lib, dev, stream = env
    base = dict(image_size=64, patch_size=16, dim=256, depth=1, heads=4, mlp_dim=768, ln_eps=1e-6, compute_dtype=1, pool=1, pool_dim=384,
                pool_heads=4, pool_ln_eps=1e-5, pool_head_dim=96)
    cases = (("pool_head_dim without AP_POOL_ATTN", dict(pool=0), "pool_head_dim"),
             ("pool_skip_final_norm without AP_POOL_ATTN", dict(pool=0, pool_head_dim=0, pool_skip_final_norm=1), "pool_skip_final_norm"),
             ("pool_proj_dim without AP_POOL_ATTN", dict(pool=2, pool_head_dim=0, pool_proj_dim=128), "pool_proj_dim"),
             ("out_normalize without AP_POOL_ATTN", dict(pool=0, pool_head_dim=0, out_normalize=1), "out_normalize"),
             ("head width 80", dict(pool_head_dim=80), "pool_head_dim"),
             ("head width 32", dict(pool_head_dim=32, pool_heads=12), "pool_head_dim"),
             ("pool_dim != heads x width", dict(pool_heads=3), "pool_head_dim"),
             ("pool_dim != heads x width (128)", dict(pool_head_dim=128), "pool_dim"),
             ("pool_dim != heads x 64 (legacy)", dict(pool_head_dim=0), "pool_dim"),
             ("projection no multiple of 128", dict(pool_proj_dim=200), "pool_proj_dim"),
             ("projection wider than the pooler", dict(pool_proj_dim=512), "pool_proj_dim"),
             ("negative projection", dict(pool_proj_dim=-128), "pool_proj_dim"),
             ("workspace reuse: 2 pool_dim > mlp_dim", dict(mlp_dim=640), "pool_dim"),
             ("out_normalize 2", dict(out_normalize=2), "out_normalize"),
             ("float32 on the 64-wide legacy kernel", dict(compute_dtype=0, pool_head_dim=0, pool_dim=256), "float16 / bfloat16 only"),
             ("float32 beyond 288 tokens", dict(compute_dtype=0, image_size=16 * 17), "float32"))
    for what, kw, word in cases:
        cfg = _lib.VitConfigEx2(**{**base, **kw})
        h = C.c_void_p()
        rc = lib.ap_vit_create(C.byref(cfg), C.byref(h))
        msg = lib.ap_last_error().decode()
        assert rc == _lib.AP_ERR_INVALID and not h.value and "vit_create" in msg and word in msg, (what, rc, msg)
    # the three sizes the structure has had, and nothing in between
    raw = bytes(_lib.VitConfigEx2(**base))
    for size, rc_want, word in ((100, _lib.AP_ERR_UNSUPPORTED, "newer"), (104, _lib.AP_ERR_UNSUPPORTED, "newer"), (108, _lib.AP_ERR_UNSUPPORTED, "newer"),
                                (116, _lib.AP_ERR_UNSUPPORTED, "newer")):
        buf = C.create_string_buffer(int(size).to_bytes(4, "little") + raw[4:] + b"\0" * 8, 120)
        h = C.c_void_p()
        rc = lib.ap_vit_create(C.cast(buf, C.POINTER(_lib.VitConfig)), C.byref(h))
        assert rc == rc_want and not h.value and word in lib.ap_last_error().decode(), (size, rc)
    # what is built: the pooler at each width, in float32 too, with pre_norm, and every field at once
    for kw, dim in ((dict(), 384), (dict(pool_head_dim=64, pool_heads=6), 384), (dict(pool_head_dim=128, pool_heads=3), 384),
                    (dict(compute_dtype=0), 384), (dict(pre_norm=1, pool_skip_final_norm=1, pool_proj_dim=256, out_normalize=1), 256),
                    (dict(pool_head_dim=0, pool_dim=256), 256)):
        cfg = _lib.VitConfigEx2(**{**base, **kw})
        assert cfg.struct_size == 112
        h = C.c_void_p()
        assert lib.ap_vit_create(C.byref(cfg), C.byref(h)) == 0 and h.value, (kw, lib.ap_last_error().decode())
        assert lib.ap_vit_embed_dim(h) == dim
        lib.ap_vit_destroy(h)
    init = _lib.VitConfigEx2(**base)
    assert lib.ap_vit_config_init(C.byref(init), C.sizeof(init)) == 0 and init.struct_size == 112 and init.pool_head_dim == 0


def test_skip_final_norm_has_no_norm_parameters(env):
    _lib, lib, dev, stream = env
    cfg = _lib.VitConfigEx2(image_size=64, patch_size=16, dim=256, depth=1, heads=4, mlp_dim=768, ln_eps=1e-6, compute_dtype=1, pool=1,
                            pool_dim=384, pool_heads=4, pool_ln_eps=1e-5, pool_head_dim=96, pool_skip_final_norm=1, pool_proj_dim=256)
    h = C.c_void_p()
    assert lib.ap_vit_create(C.byref(cfg), C.byref(h)) == 0
    ones = np.ones(256 * 384, np.float32)
    assert lib.ap_vit_set_param(h, b"norm.weight", ones.ctypes.data, 256) != 0 and b"norm.weight" in lib.ap_last_error()
    assert lib.ap_vit_set_param(h, b"attn_pool.proj.weight", ones.ctypes.data, 256 * 384) == 0
    assert lib.ap_vit_set_param(h, b"attn_pool.proj.weight", ones.ctypes.data, 384 * 384) != 0
    lib.ap_vit_destroy(h)


# ----------------------------------------------------------------------------- the real width
@pytest.fixture(scope="module")
def real():
    """name -> (module, arch, canonical state dict, x [3, 3, S, S], the module's float32 output on the CPU), 2 blocks of width 1024."""
    from atlaspatch_amd.encoders.vit import coca_canonical_state_dict, conch_v15_canonical_state_dict
    out = {}
    model = R.seed_module(R.CocaModel(layers=2, n_queries=4), 31)
    arch = R.coca_arch(dict(width=1024, layers=2, heads=16, mlp=4096, image=224, patch=14, pool_dim=768, pool_heads=8, output_dim=768))
    x = R.images(3, 224, seed=5)
    with torch.inference_mode():
        want = model.encode_image(x).numpy()
    out["omiclip"] = (model, arch, coca_canonical_state_dict(dict(model.state_dict()), arch), x, want)
    model = R.seed_module(R.ConchV15(layers=2), 32)
    arch = R.conch_arch(dict(width=1024, layers=2, heads=16, mlp=4096, image=448, patch=16, pool_dim=768, pool_heads=8))
    x = R.images(3, 448, seed=6)
    with torch.inference_mode():
        want = model(x).numpy()
    out["conch_v15"] = (model, arch, conch_v15_canonical_state_dict(dict(model.state_dict()), arch)[0], x, want)
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("name", ["omiclip", "conch_v15"])
def test_real_width_vs_the_restatement_and_its_own_half_precision(real, name, dtype):
    """Width 1024, 16 heads, MLP 4096, pool 768 = 8 x 96, 2 blocks, 257 (omiclip) / 785 (conch_v15) tokens, n = 3.  The bound is the
    restatement's own: the same module run in this 16-bit type on the CPU, measured here against its float32 run, times 1.5 (a
    different summation order on three samples).  MEASURED holds both figures."""
    model, arch, state, x, want = real[name]
    with torch.inference_mode():
        half = copy.deepcopy(model).to(dtype)
        own = (half.encode_image(x.to(dtype)) if name == "omiclip" else half(x.to(dtype))).float().numpy()
    own_err = R.rel(own, want)
    got = _device_features(arch, state, x, dtype)
    ours = R.rel(got, want)
    print(f"PARITY {name} width 1024 depth 2 {dtype}: restatement in {dtype} on the CPU {own_err:.3e}, this engine {ours:.3e} "
          f"(bound 1.5 x = {1.5 * own_err:.3e}); recorded {MEASURED[(name, str(dtype).replace('torch.', ''))]}")
    assert got.shape == want.shape == (3, 768)
    assert ours <= 1.5 * own_err


def test_real_width_omiclip_float32(real):
    model, arch, state, x, want = real["omiclip"]
    with torch.inference_mode():
        want64 = copy.deepcopy(model).double().encode_image(x.double()).numpy()
    got = _device_features(arch, state, x, torch.float32)
    r = R.rel(got, want64)
    print(f"PARITY omiclip width 1024 depth 2 float32 vs the float64 restatement: {r:.3e} (bound {TOL[torch.float32]:.0e})")
    assert got.shape == (3, 768) and r <= TOL[torch.float32]


# ----------------------------------------------------------------------------- the plugin, end to end
@pytest.mark.parametrize("name", ["omiclip", "conch_v15"])
def test_plugin_extract_batch(monkeypatch, name):
    """ATLASPATCH_RANDOM_INIT, depth 2 (an arch override), float16: three 256-px uint8 tiles -> device resize to 224 / 448 ->
    [3, 768] float32, against the canonical forward (float32 on the CPU) on the same resized input within the float16 bound."""
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry
    from atlaspatch_amd.encoders.vit import ARCHS, TRANSFORM_NORM, random_canonical_state_dict, register_coca_towers
    import atlaspatch_amd.plugins.coca_towers as plugin
    assert plugin.register_coca_towers is register_coca_towers
    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "11")
    monkeypatch.delenv("ATLASPATCH_WEIGHTS_DIR", raising=False)
    dev = torch.device("cuda:0")
    reg = PatchFeatureExtractorRegistry()
    register_coca_towers(reg, device=dev, dtype=torch.float16, depth=2)
    ex = reg.create(name)
    size = ARCHS[name]["image_size"]
    assert ex.embedding_dim == 768 and 1 <= ex.max_batch <= 256 and ex.resize == (size, "bicubic")
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, size=(3, 32, 32, 3), dtype=np.uint8)
    tiles = [np.ascontiguousarray(np.kron(t, np.ones((8, 8, 1), dtype=np.uint8))) for t in base]     # 256 x 256, blocky: the resize matters
    got = ex.extract_batch(tiles, batch_size=4)
    assert got.shape == (3, 768) and got.dtype == np.float32 and np.isfinite(got).all()
    resized = ex.resized(torch.from_numpy(np.stack(tiles)).to(dev)).cpu()
    assert tuple(resized.shape) == (3, size, size, 3)
    ex.cleanup()
    arch = dict(ARCHS[name], depth=2)
    mean, std = (torch.tensor(v, dtype=torch.float64).reshape(1, 3, 1, 1) for v in TRANSFORM_NORM[name])
    x = ((resized.permute(0, 3, 1, 2).double() / 255.0 - mean) / std).float()
    want = R.canonical_forward(random_canonical_state_dict(arch, seed=11), x, arch, torch.float32).numpy()
    r = R.rel(got, want)
    print(f"PARITY {name} plugin depth 2 float16 vs the float32 restatement: norm-wise {r:.3e} (bound {TOL[torch.float16]:.0e})")
    assert r <= TOL[torch.float16]
    if name == "omiclip":
        assert np.allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-3)
