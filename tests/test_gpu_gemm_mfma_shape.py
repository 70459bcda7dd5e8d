"""The 16-bit ViT GEMMs on v_mfma_f32_16x16x32 (gemm256.hip) beside the 128x128 kernel, which stays on 32x32x16:
accuracy against float64 with a bound derived from the arithmetic, bitwise agreement of the two kernels at the benchmark's
own shapes with the fused epilogues, and the depth-12 encoder end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from atlaspatch_amd import _lib
    dev = torch.device("cuda:0")
    return _lib, _lib.load(), dev, _lib.current_stream_ptr(dev)


def _ulp(v, dt):
    """Spacing of dt's numbers at magnitude v (float64 tensor)."""
    p, emin = (10, -14) if dt == torch.float16 else (7, -126)
    _, e = torch.frexp(v)                       # v = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), torch.clamp(e - 1, min=emin) - p)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("impl", [256, 128])
@pytest.mark.parametrize("shape", [(3941, 768, 3072), (5000, 2304, 768), (300, 256, 128)])
def test_gemm_16bit_within_the_f32_accumulation_bound_of_float64(env, dt, impl, shape):
    """x = the float64 product plus bias.  Every output must satisfy
        |out - x| <= ulp_T(max(|x|, |out|)) / 2 + (K + 1) 2^-23 (sum_k |a_k w_k| + |bias|):
    half an output ulp for the final rounding plus the standard bound on K + 1 f32 additions of products that are exact in
    f32 (f16 x f16 has 22 significant bits, bf16 x bf16 16), with 2^-23 per addition so that a truncating adder tree is
    covered as well.  It holds for any summation order, hence for either MFMA shape; a wrong fragment or accumulator map
    gives errors of order one."""
    _lib, lib, dev, stream = env
    M, N, K = shape
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A = (torch.rand((M, K), device=dev, generator=g) * 2 - 1).to(dt)
    W = ((torch.rand((N, K), device=dev, generator=g) * 2 - 1) * (2.0 / K ** 0.5)).to(dt)
    bias = torch.rand(N, device=dev, generator=g) - 0.5
    out = torch.full((M, N), float("nan"), device=dev, dtype=dt)
    _lib.check(lib.ap_gemm(_lib.torch_dtype_code(dt), 0, A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), M, N, K,
                           bias.data_ptr(), None, out.data_ptr(), out.stride(0), impl, 0, stream), "ap_gemm")
    torch.cuda.synchronize()
    x = A.double() @ W.double().t() + bias.double()
    mag = A.double().abs() @ W.double().abs().t() + bias.double().abs()
    o = out.double()
    assert torch.isfinite(o).all()
    err = (o - x).abs()
    bound = _ulp(torch.maximum(x.abs(), o.abs()), dt) / 2 + (K + 1) * 2.0 ** -23 * mag
    worst = (err / bound).max().item()
    print(f"GEMM64 impl {impl} {str(dt)[6:]} {shape}: max |err| {err.max().item():.3e}, max err / bound {worst:.3f}")
    assert (err <= bound).all(), (impl, dt, shape, worst, int((err > bound).sum()))


def _fused(env, epi, A, W, bias, colsum, rowstats, partial, out, impl):
    _lib, lib, dev, stream = env
    M, K = A.shape
    _lib.check(lib.ap_gemm_fused(_lib.torch_dtype_code(A.dtype), epi, A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), M,
                                 W.shape[0], K, bias.data_ptr(), colsum.data_ptr() if colsum is not None else None,
                                 rowstats.data_ptr() if rowstats is not None else None,
                                 partial.data_ptr() if partial is not None else None, out.data_ptr(), out.stride(0), impl, stream),
               "ap_gemm_fused")


@pytest.mark.parametrize("case", [("qkv", 2304, 768, 4), ("proj", 768, 768, 6), ("fc1", 3072, 768, 5), ("fc2", 768, 3072, 6)])
def test_the_two_gemm_kernels_agree_bitwise_at_the_benchmark_shapes(env, case):
    """300 images x 197 tokens (230 full 256-row tiles and a ragged one), the (N, K) of the four ViT-B linears with the fused
    epilogue each runs in the forward and real operands: row statistics of the activation rows, column sums of the weight,
    a 16-bit stream window under RESID_STATS.  float16: impl 256 bit-equal impl 128, and each bit-equal itself."""
    _lib, lib, dev, stream = env
    name, N, K, epi = case
    M = 197 * 300
    g = torch.Generator(device=dev).manual_seed(N + K + epi)
    A = ((torch.rand((M, K), device=dev, generator=g) * 2 - 1) * (0.5 + torch.rand((M, 1), device=dev, generator=g))
         + (torch.rand((M, 1), device=dev, generator=g) - 0.5)).half()
    W = ((torch.rand((N, K), device=dev, generator=g) * 2 - 1) * (2.0 / K ** 0.5)).half()
    bias = torch.rand(N, device=dev, generator=g) - 0.5
    colsum = W.float().sum(-1).contiguous()
    mean = A.float().mean(-1)
    rstd = torch.rsqrt(A.float().var(-1, unbiased=False) + 1e-6)
    rowstats = torch.stack([rstd, -mean * rstd], -1).contiguous()
    stream0 = (torch.rand((M, N), device=dev, generator=g) * 4 - 2).half()

    def run(impl):
        if epi == 6:
            out = stream0.clone()
            part = torch.full((M, N // 64, 2), float("nan"), device=dev)
            _fused(env, epi, A, W, bias, None, None, part, out, impl)
            torch.cuda.synchronize()
            return out, part
        out = torch.full((M, N), float("nan"), device=dev, dtype=torch.float16)
        _fused(env, epi, A, W, bias, colsum, rowstats, None, out, impl)
        torch.cuda.synchronize()
        return (out,)

    r256, r256b, r128, r128b = run(256), run(256), run(128), run(128)
    for t in r256 + r128:
        assert torch.isfinite(t.float()).all()
    for a, b in zip(r256, r256b):
        assert torch.equal(a, b), (name, "impl 256 differs from itself")
    for a, b in zip(r128, r128b):
        assert torch.equal(a, b), (name, "impl 128 differs from itself")
    for a, b in zip(r256, r128):
        assert torch.equal(a, b), (name, int((a != b).sum()))


def test_vit_b16_depth_12_float16_end_to_end():
    """64 seeded tiles through the seeded depth-12 ViT-B/16: inside the existing bounds against the fp32 CPU oracle, and
    bit-equal between one batch of 64 and cuts of 1 / 7 / 33."""
    from oracle import vit_oracle
    from tests.test_gpu_parity import _check, _hf_extractor
    ex, sd = _hf_extractor(12, torch.float16)
    rng = np.random.default_rng(64)
    tiles = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(64)]
    want = vit_oracle.extract_batch(sd, tiles, heads=12, batch_size=32)
    got = ex.extract_batch(tiles, batch_size=64)
    _check(got, want, torch.float16, "vit_b_16 L12 vs oracle")
    for cut in (1, 7, 33):
        assert np.array_equal(ex.extract_batch(tiles, batch_size=cut), got), cut
    ex.cleanup()
