"""The SigLIP vision tower on the device, through the C ABI (include/atlaspatch_hip.h): the tanh-GELU epilogues of ap_gemm /
ap_gemm_fused and ap_attention_probe against the float64 restatements of tests/siglip_reference.py under the acceptance check of
tests/vit_ops_reference.py (outputs between NaN-pattern guard bands, compared bit for bit), the engine (no_class_token,
AP_ACT_GELU_TANH, AP_POOL_MAP) against transformers' SiglipVisionModel itself, ap_vit_create's refusals, and the medsiglip plugin
end to end at the real token count."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import siglip_reference as S
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.float16: 4e-3, torch.bfloat16: 3e-2}      # tests/test_encoder_zoo.py's device-vs-HF bounds

# The real width (hidden 1152, 16 heads of 72, MLP 4304, 2 layers, n = 5) against the HF model in float32 on the CPU, norm-wise:
# (image, dtype) -> (the HF model ITSELF in that 16-bit type on the CPU, this engine on the MI355X).  The bound is 1.5 x the first.
MEASURED = {
    (56, "float16"): (2.277e-3, 1.954e-3),
    (56, "bfloat16"): (1.937e-2, 1.682e-2),
    (70, "float16"): (2.337e-3, 2.064e-3),
    (70, "bfloat16"): (1.834e-2, 1.649e-2),
}


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    return _lib, _lib.load(), dev, _lib.current_stream_ptr(dev)


def _verify(op, case_results):
    failed, worst = [], 0.0
    for cid, got, want in case_results:
        for name, o in want.items():
            k = S.k_of(op, o)
            bad = S.failures(got[name], o, k)
            tol = S.U[o.dtype] * o.value.abs() + S.FLOOR[o.dtype] + k * 2.0 ** -24 * o.A.double()
            ratio = (got[name].double() - o.value).abs() / tol
            worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
            if bad:
                failed.append((cid, name, bad))
    print(f"{op}: {len(case_results)} cases, worst |got - ref64| / bound = {worst:.3f}")
    assert not failed, f"{op}: {len(failed)} failing outputs, first {failed[:8]}"


# ----------------------------------------------------------------------------- GEMM + tanh GELU
@pytest.mark.parametrize("dt", S.ALL, ids=str)
def test_gemm_gelu_tanh_epilogues(env, dt):
    """AP_EPI_BIAS_GELU_TANH through ap_gemm (f16, bf16, f32) and AP_EPI_NORM_GELU_TANH through ap_gemm_fused (f16, bf16) on both
    kernels wherever each takes the shape: (300, 256, 128) reaches the 256 x 256 kernel, every shape the 128 x 128 one, with row
    tails in both.  Pre-activations out to +-12, an exact 0, the 16-bit extremes."""
    _lib, lib, dev, stream = env
    results = []
    for case in S.cases_gemm_gelu_tanh(dtypes=(dt,)):
        a = case.args
        M, N, K = a["M"], a["N"], a["K"]
        A, W, bias = a["A"].to(dev), a["W"].to(dev), a["bias"].to(dev)
        want = S.ref_gemm_gelu_tanh(a)
        impls = [128] + ([256] if dt != torch.float32 and N % 256 == 0 and K % 128 == 0 else [])
        for impl in impls:
            out = Guarded((M, N), dt, dev)
            if a["norm"]:
                cs, rs = a["colsum"].to(dev), a["rowstats"].to(dev)
                _lib.check(lib.ap_gemm_fused(S.CODE[dt], S.AP_EPI_NORM_GELU_TANH, A.data_ptr(), K, W.data_ptr(), K, M, N, K, bias.data_ptr(),
                                             cs.data_ptr(), rs.data_ptr(), None, out.ptr(), N, impl, stream), "ap_gemm_fused")
            else:
                _lib.check(lib.ap_gemm(S.CODE[dt], S.AP_EPI_BIAS_GELU_TANH, A.data_ptr(), K, W.data_ptr(), K, M, N, K, bias.data_ptr(), None,
                                       out.ptr(), N, impl, 0, stream), "ap_gemm")
            torch.cuda.synchronize()
            got = out.cpu()
            assert not bool(torch.isnan(got).any())
            ext = S.EXTREME[dt]
            assert float(got[0, 0]) == 0.0 and float(got[1, 2]) == ext and float(got[1, 3]) == 0.0
            assert math.copysign(1.0, float(got[1, 3])) == -1.0, "the function tends to -0 for large negative inputs"
            results.append((f"{case.id}-impl{impl}", {"out": got}, want))
    assert any(cid.endswith("impl256") for cid, _, _ in results) == (dt != torch.float32)
    _verify("gemm_gelu_tanh", results)


# ----------------------------------------------------------------------------- attention with one shared float32 query
@pytest.mark.parametrize("hd", [64, 96, 128])
@pytest.mark.parametrize("dt", S.ALL, ids=str)
def test_attention_probe(env, dt, hd):
    """Tokens around the row-slot count, around one pass of the 256 threads and the real model's 1024; n in {1, 3} x heads in {1, 5};
    packed k | v rows and a wider layout with v in front of k; at width 96 also 1 / sqrt(72) on zero-padded 72-wide heads; one
    head per case whose scores reach 95."""
    _lib, lib, dev, stream = env
    results, hot = [], False
    for case in S.cases_attention_probe(dtypes=(dt,), widths=(hd,)):
        a = case.args
        q, kv = a["q"].to(dev), a["kv"].to(dev)
        assert q.dtype == torch.float32
        out = Guarded((a["n"], a["heads"] * hd), dt, dev)
        _lib.check(lib.ap_attention_probe(S.CODE[dt], q.data_ptr(), kv.data_ptr(), a["ld"], a["koff"], a["voff"], out.ptr(), a["n"], a["tokens"],
                                          a["heads"], hd, a["scale"], stream), "ap_attention_probe")
        torch.cuda.synchronize()
        want = S.ref_attention_probe(a)
        hot = hot or bool(want["out"].hot.any())
        results.append((case.id, {"out": out.cpu()}, want))
    assert hot, "no case reached the overflow range"
    _verify("attention_probe", results)


def test_attention_probe_refusals_launch_nothing(env):
    _lib, lib, dev, stream = env
    q = torch.zeros(128, device=dev)
    kv = torch.zeros(4, 256, dtype=torch.float16, device=dev)
    out = Guarded((1, 128), torch.float16, dev)
    call = lambda **kw: lib.ap_attention_probe(*[{**dict(dtype=1, q=q.data_ptr(), kv=kv.data_ptr(), ld=256, koff=0, voff=128, out=out.ptr(), n=1,
                                                         tokens=4, heads=1, hd=128, scale=0.1, stream=stream), **kw}[k]
                                                 for k in ("dtype", "q", "kv", "ld", "koff", "voff", "out", "n", "tokens", "heads", "hd", "scale", "stream")])
    for what, kw in (("head width", dict(hd=72)), ("misaligned ld", dict(ld=260)), ("tokens 0", dict(tokens=0)),
                     ("misaligned koff", dict(koff=4)), ("v outside the row", dict(voff=192)), ("dtype", dict(dtype=7)),
                     ("null query", dict(q=None))):
        rc = call(**kw)
        msg = lib.ap_last_error().decode()
        assert rc in (_lib.AP_ERR_INVALID, _lib.AP_ERR_UNSUPPORTED) and "ap_attention_probe" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert out.untouched()
    assert call() == 0
    torch.cuda.synchronize()
    assert not out.untouched()


# ----------------------------------------------------------------------------- the engine against the HF model
@pytest.fixture(scope="module")
def tiny():
    """image -> (HF model float32, arch, x [3, 3, S, S], pooler_output): the reference, computed once and left unchanged."""
    out = {}
    for image, patch in ((64, 16), (238, 14)):
        model, arch = S.hf_siglip(hidden=256, heads=4, inter=600, layers=2, image=image, patch=patch)
        x = torch.randn(3, 3, image, image, generator=torch.Generator().manual_seed(2))
        with torch.inference_mode():
            want = model(pixel_values=x).pooler_output.numpy()
        out[image] = (model, arch, x, want)
    return out


def _device_features(model, arch, x, dtype, **options):
    from atlaspatch_amd.encoders.vit import build_hip_vit_extractor
    dev = torch.device("cuda:0")
    ex = build_hip_vit_extractor(name="medsiglip", arch=arch, state_dict=dict(model.state_dict()), device=dev, dtype=dtype,
                                 resize=None, expect_size=None, max_batch=16)
    assert ex.embedding_dim == arch["dim"]
    for name, on in options.items():
        ex.vit.set_option(name, on)
    got = ex.vit.forward_chw(x.to(dev).contiguous())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    ex.cleanup()
    return got


@pytest.mark.parametrize("dtype,f32_stream", [(torch.float32, False), (torch.float16, False), (torch.float16, True),
                                              (torch.bfloat16, False), (torch.bfloat16, True)], ids=str)
def test_tiny_tower_vs_the_hf_model(tiny, dtype, f32_stream):
    """hidden 256, 4 heads, MLP 600 (stored 640), 2 layers, 16 tokens, n = 3: HF checkpoint -> adapter -> HipViT -> forward_chw, both
    dataflows of the 16-bit types (float32 has the one)."""
    model, arch, x, want = tiny[64]
    got = _device_features(model, arch, x, dtype, **({"f32_stream": True} if f32_stream else {}))
    r = S.rel(got, want)
    print(f"PARITY medsiglip tiny 16 tokens {dtype} {'f32_stream' if f32_stream else 'default'}: norm-wise {r:.3e} (bound {TOL[dtype]:.0e})")
    assert got.shape == want.shape == (3, 256) and r <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_tiny_tower_at_289_tokens_vs_the_hf_model(tiny, dtype):
    """image 238 / patch 14: 289 tokens, M = 867 -- a row tail in every GEMM and more than one pass of the pooling kernel."""
    model, arch, x, want = tiny[238]
    got = _device_features(model, arch, x, dtype)
    r = S.rel(got, want)
    print(f"PARITY medsiglip tiny 289 tokens {dtype}: norm-wise {r:.3e} (bound {TOL[dtype]:.0e})")
    assert got.shape == want.shape == (3, 256) and r <= TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_exact_cls_is_inert_without_a_class_row(tiny, dtype):
    model, arch, x, _ = tiny[64]
    on = _device_features(model, arch, x, dtype, exact_cls=True)
    off = _device_features(model, arch, x, dtype, exact_cls=False)
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))


@pytest.mark.parametrize("image", [56, 70])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_real_width_vs_the_hf_model_and_its_own_half_precision(dtype, image):
    """hidden 1152, 16 heads of 72 (stored 96, scale 1 / sqrt(72)), MLP 4304 (stored 4352), 2 layers, 16 / 25 tokens, n = 5.  The
    bound is the HF model's own: the same model run in this 16-bit type on the CPU, measured here against its float32 run,
    times 1.5 (a different summation order on five samples).  MEASURED holds both figures."""
    model, arch = S.hf_siglip(hidden=1152, heads=16, inter=4304, layers=2, image=image, patch=14)
    x = torch.randn(5, 3, image, image, generator=torch.Generator().manual_seed(3))
    with torch.inference_mode():
        want = model(pixel_values=x).pooler_output.numpy()
        own = copy.deepcopy(model).to(dtype)(pixel_values=x.to(dtype)).pooler_output.float().numpy()
    hf_half = S.rel(own, want)
    got = _device_features(model, arch, x, dtype)
    ours = S.rel(got, want)
    print(f"PARITY medsiglip width 1152 image {image} {dtype}: HF {dtype} on the CPU {hf_half:.3e}, this engine {ours:.3e} "
          f"(bound 1.5 x = {1.5 * hf_half:.3e}); recorded {MEASURED[(image, str(dtype).replace('torch.', ''))]}")
    assert got.shape == want.shape == (5, 1152)
    assert ours <= 1.5 * hf_half


# ----------------------------------------------------------------------------- ap_vit_create
def test_create_refuses_what_is_not_built(env):
    _lib, lib, dev, stream = env
    base = dict(image_size=64, patch_size=16, dim=256, depth=1, heads=4, mlp_dim=640, ln_eps=1e-6, compute_dtype=1, pool=3, act=2,
                no_class_token=1)
    cases = (("no_class_token with AP_POOL_CLS", dict(pool=0), "no_class_token"),
             ("no_class_token with register tokens", dict(reg_tokens=4), "reg_tokens"),
             ("AP_POOL_MAP with a class token", dict(no_class_token=0), "AP_POOL_MAP"),
             ("tanh GELU with SwiGLU", dict(mlp_type=1), "act 2"),
             ("float32 beyond 288 tokens", dict(compute_dtype=0, image_size=16 * 17), "float32"),
             ("no_class_token with pre_norm", dict(pre_norm=1), "pre_norm"),
             ("no_class_token with rope", dict(rope=1), "rope"))
    for what, kw, word in cases:
        cfg = _lib.VitConfigEx(**{**base, **kw})
        h = C.c_void_p()
        rc = lib.ap_vit_create(C.byref(cfg), C.byref(h))
        msg = lib.ap_last_error().decode()
        assert rc == _lib.AP_ERR_INVALID and not h.value and "vit_create" in msg and word in msg, (what, rc, msg)
    # what is built: the 92-byte structure of ABI v20 opens a class-token model as before, the longer one the SigLIP form -- and,
    # its appended fields zero, the same class-token model
    assert C.sizeof(_lib.VitConfig) == 92 == lib.ap_sizeof_vit_config() and C.sizeof(_lib.VitConfigEx) == 96
    v20 = {k: v for k, v in {**base, "pool": 0, "act": 0}.items() if k != "no_class_token"}
    for cfg in (_lib.VitConfig(**v20), _lib.VitConfigEx(**v20), _lib.VitConfigEx(**base)):
        assert cfg.struct_size == C.sizeof(cfg)
        h = C.c_void_p()
        assert lib.ap_vit_create(C.byref(cfg), C.byref(h)) == 0 and h.value, lib.ap_last_error().decode()
        assert lib.ap_vit_embed_dim(h) == 256
        lib.ap_vit_destroy(h)
    init = _lib.VitConfigEx(**base)
    assert lib.ap_vit_config_init(C.byref(init), C.sizeof(init)) == 0 and init.struct_size == 96 and init.no_class_token == 0


# ----------------------------------------------------------------------------- the plugin, end to end at the real token count
def test_plugin_extract_batch_at_1024_tokens(monkeypatch):
    """ATLASPATCH_RANDOM_INIT, depth 2 (an arch override), float16: three 256-px uint8 tiles -> device resize to 448 -> 1024 tokens
    -> [3, 1152] float32, against the torch restatement (float32 on the CPU: its own error is ~1e-6) on the same resized input
    within the float16 bound."""
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry
    from atlaspatch_amd.encoders.vit import ARCHS, random_canonical_state_dict, register_medsiglip
    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "11")
    monkeypatch.delenv("ATLASPATCH_WEIGHTS_DIR", raising=False)
    dev = torch.device("cuda:0")
    reg = PatchFeatureExtractorRegistry()
    register_medsiglip(reg, device=dev, dtype=torch.float16, depth=2)
    ex = reg.create("medsiglip")
    assert ex.embedding_dim == 1152 and 1 <= ex.max_batch <= 128 and ex.resize == (448, "bilinear")
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, size=(3, 32, 32, 3), dtype=np.uint8)
    tiles = [np.ascontiguousarray(np.kron(t, np.ones((8, 8, 1), dtype=np.uint8))) for t in base]     # 256 x 256, blocky: the resize matters
    got = ex.extract_batch(tiles, batch_size=4)
    assert got.shape == (3, 1152) and got.dtype == np.float32 and np.isfinite(got).all()
    resized = ex.resized(torch.from_numpy(np.stack(tiles)).to(dev)).cpu()
    assert tuple(resized.shape) == (3, 448, 448, 3)
    ex.cleanup()
    arch = dict(ARCHS["medsiglip"], depth=2)
    stored = S.stored_state(random_canonical_state_dict(arch, seed=11), arch)
    x = ((resized.permute(0, 3, 1, 2).double() / 255.0 - 0.5) / 0.5).float()
    want = S.siglip_forward(stored, x, heads=16, depth=2, scale=1.0 / math.sqrt(72.0)).numpy()
    r = S.rel(got, want)
    print(f"PARITY medsiglip plugin 1024 tokens depth 2 float16 vs the float32 restatement: norm-wise {r:.3e} (bound {TOL[torch.float16]:.0e})")
    assert r <= TOL[torch.float16]
