"""ConvNeXt encoders on the MI355X: the single operators (fused depthwise 7x7 + LayerNorm, LayerNorm rows, the implicit GEMM's
32-wide N tail and GELU epilogue) against torch, the full networks against the CPU restatement (tests/convnext_reference.py),
batch-cut invariance, the device resize of a 512-px tile, and `process` with the shipped plugin.

Bounds: float32 products are exact f32 MFMA chains / f32 FMAs (bound 1e-5 everywhere).  float16 / bfloat16 network bounds are
the first MI355X run's measured error x 1.2 (the measured value is next to each bound)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import convnext_reference as ref
from tests.helpers import DT, _lib, _record, _rel, _tiles, _tiles33

pytestmark = pytest.mark.gpu

# one operator: the output's rounding to T (and a 1-ulp different rounding of an intermediate) is the error
OP_TOL = {"float32": 1e-5, "float16": 1e-3, "bfloat16": 8e-3}
# network features against the CPU float32 restatement (measured on the first MI355X run; bound = measured x 1.2)
NET_TOL = {("convnext_tiny", "float32"): 1e-5,                                              # measured 3.03e-7
           ("convnext_tiny", "float16"): 6.7e-4, ("convnext_tiny", "bfloat16"): 5.5e-3,       # measured 5.58e-4 / 4.62e-3
           ("convnext_small", "float16"): 7.2e-4, ("convnext_base", "float16"): 7.3e-4,       # measured 5.99e-4 / 6.11e-4
           ("convnext_large", "float16"): 7.2e-4}                                             # measured 5.97e-4
MEASURED = "ATLASPATCH_CONVNEXT_MEASURED"      # optional: names the path to record the measured errors in (bound updates)
EPS = 1e-6


def _dw_shapes():
    """{(C, H)} of every depthwise layer of the four networks."""
    from atlaspatch_amd.encoders.convnext import ARCHS
    return sorted({(spec["widths"][s], 56 >> s) for spec in ARCHS.values() for s in range(4)})


DEV = torch.device("cuda")


# ----------------------------------------------------------------------------- operators
@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", _dw_shapes(), ids=lambda s: "c%d_h%d" % s)
def test_dwconv7_ln_every_shape(shape, n, dtype_name):
    c, h = shape
    lib, L = _lib()
    dt, code = DT[dtype_name]
    g = torch.Generator().manual_seed(c + h + n)
    x = torch.randn(n, c, h, h, generator=g).to(dt)
    w = torch.randn(c, 1, 7, 7, generator=g) / 7.0
    b = 0.1 * torch.randn(c, generator=g)
    lw = 0.8 + 0.4 * torch.rand(c, generator=g)
    lb = 0.1 * torch.randn(c, generator=g)
    y = F.conv2d(x.float(), w, b, padding=3, groups=c).to(dt).float()           # the conv output is rounded to T
    want = F.layer_norm(y.permute(0, 2, 3, 1), (c,), lw, lb, EPS)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = w.reshape(c, 49).t().contiguous().to(DEV)                              # tap-major [49][C]
    bd, lwd, lbd = b.to(DEV), lw.to(DEV), lb.to(DEV)                            # held: the pointers must stay valid
    out = torch.empty_like(xd)
    lib.check(L.ap_dwconv7_ln_nhwc(code, xd.data_ptr(), n, h, h, c, wd.data_ptr(), bd.data_ptr(), lwd.data_ptr(), lbd.data_ptr(),
                                   EPS, out.data_ptr(), lib.current_stream_ptr(DEV)), "dwconv7_ln")
    torch.cuda.synchronize()
    rel = _rel(out.float().cpu(), want)
    assert rel <= OP_TOL[dtype_name], rel


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("rows,c", [(1000, 96), (147, 192), (33, 768), (5, 1536)])
def test_layernorm_rows(rows, c, dtype_name):
    lib, L = _lib()
    dt, code = DT[dtype_name]
    g = torch.Generator().manual_seed(rows + c)
    x = (3.0 * torch.randn(rows, c, generator=g) + 1.0).to(dt)
    lw = 0.8 + 0.4 * torch.rand(c, generator=g)
    lb = 0.1 * torch.randn(c, generator=g)
    want = F.layer_norm(x.float(), (c,), lw, lb, EPS)
    xd, lwd, lbd = x.to(DEV), lw.to(DEV), lb.to(DEV)
    out = torch.empty_like(xd)
    lib.check(L.ap_layernorm_rows(code, xd.data_ptr(), rows, c, lwd.data_ptr(), lbd.data_ptr(), EPS, out.data_ptr(),
                                  lib.current_stream_ptr(DEV)), "layernorm_rows")
    torch.cuda.synchronize()
    rel = _rel(out.float().cpu(), want)
    assert rel <= OP_TOL[dtype_name], rel


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("case", [(1, 1, 384, 96, 7, 3, True, 0), (1, 1, 96, 384, 7, 3, False, 2),
                                  (1, 1, 768, 192, 14, 2, True, 0), (1, 1, 192, 96, 28, 1, True, 2),
                                  (4, 4, 8, 96, 224, 1, False, 0), (2, 2, 96, 192, 56, 1, False, 0),
                                  (1, 1, 64, 64, 7, 2, True, 1)],
                         ids=["fc2_96_resid", "fc1_384_gelu", "fc2_192_resid", "tail96_gelu_resid", "stem4x4", "down2x2",
                              "relu_64"])
def test_conv2d_ex_tail_and_gelu(case, dtype_name):
    k, stride, cin, cout, h, n, resid, act = case
    lib, L = _lib()
    dt, code = DT[dtype_name]
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(n, cin, h, h, generator=g).to(dt)
    w = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).to(dt)
    b = 0.1 * torch.randn(cout, generator=g)
    ho = (h - k) // stride + 1
    r = torch.randn(n, cout, ho, ho, generator=g).to(dt) if resid else None
    want = F.conv2d(x.float(), w.float(), b, stride=stride)
    if r is not None:
        want = want + r.float()
    want = {0: want, 1: F.relu(want), 2: F.gelu(want)}[act]
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    rd = r.permute(0, 2, 3, 1).contiguous().to(DEV) if r is not None else None
    bd = b.to(DEV)
    # a guard row of sentinels after the output: the masked tail must not write past Cout
    buf = torch.full((n * ho * ho * cout + 64,), 7.0, dtype=dt, device=DEV)
    lib.check(L.ap_conv2d_nhwc_ex(code, xd.data_ptr(), n, h, h, cin, wd.data_ptr(), bd.data_ptr(), cout, k, stride, 0,
                                  rd.data_ptr() if rd is not None else None, act, buf.data_ptr(), lib.current_stream_ptr(DEV)),
              "conv2d_nhwc_ex")
    torch.cuda.synchronize()
    got = buf[:n * ho * ho * cout].view(n, ho, ho, cout).float().cpu().permute(0, 3, 1, 2)
    assert torch.all(buf[n * ho * ho * cout:].float().cpu() == 7.0)
    rel = _rel(got, want)
    assert rel <= OP_TOL[dtype_name], rel


def test_conv2d_ex_refuses_bad_arguments():
    lib, L = _lib()
    x = torch.zeros(1, 7, 7, 96, dtype=torch.float16, device=DEV)
    w = torch.zeros(80, 1, 1, 96, dtype=torch.float16, device=DEV)
    b = torch.zeros(96, device=DEV)
    out = torch.zeros(1, 7, 7, 96, dtype=torch.float16, device=DEV)
    s = lib.current_stream_ptr(DEV)
    assert L.ap_conv2d_nhwc_ex(1, x.data_ptr(), 1, 7, 7, 96, w.data_ptr(), b.data_ptr(), 80, 1, 1, 0, None, 0,
                               out.data_ptr(), s) == lib.AP_ERR_INVALID                    # Cout % 32
    assert L.ap_conv2d_nhwc_ex(1, x.data_ptr(), 1, 7, 7, 96, w.data_ptr(), b.data_ptr(), 96, 1, 1, 0, None, 3,
                               out.data_ptr(), s) == lib.AP_ERR_INVALID                    # activation code
    # the ResNet entry point keeps its Cout % 64 rule
    assert L.ap_conv2d_nhwc(1, x.data_ptr(), 1, 7, 7, 96, w.data_ptr(), b.data_ptr(), 96, 1, 1, 0, None, 0,
                            out.data_ptr(), s) == lib.AP_ERR_INVALID


# ----------------------------------------------------------------------------- full networks
_REF_CACHE = {}


def _canonical(arch, seed=3):
    from atlaspatch_amd.encoders.convnext import random_canonical_state_dict
    key = (arch, seed)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = random_canonical_state_dict(arch, seed)
    return _REF_CACHE[key]


def _reference(arch, tiles, tag):
    from atlaspatch_amd.encoders.convnext import ARCHS
    key = (arch, tag)
    if key not in _REF_CACHE:
        spec = ARCHS[arch]
        _REF_CACHE[key] = ref.extract_batch(_canonical(arch), tiles, depths=spec["depths"], resize=spec["resize"])
    return _REF_CACHE[key]


def _extractor(arch, dtype_name, **kw):
    from atlaspatch_amd.encoders.convnext import build_hip_convnext_extractor
    return build_hip_convnext_extractor(name=arch, arch=arch, device="cuda", dtype=DT[dtype_name][0],
                                        state_dict=_canonical(arch), **kw)


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
def test_convnext_tiny_against_the_restatement(dtype_name):
    arch = "convnext_tiny"
    tiles = _tiles33()
    want_all = _reference(arch, tiles, "t33")
    ex = _extractor(arch, dtype_name)
    try:
        empty = ex.extract_batch([])
        assert empty.shape == (0, 768) and empty.dtype == np.float32
        worst = 0.0
        for n in (1, 5, 32, 33):
            got = ex.extract_batch(tiles[:n], batch_size=32)
            assert got.shape == (n, 768) and got.dtype == np.float32 and np.isfinite(got).all()
            rel = _rel(got, want_all[:n])
            worst = max(worst, rel)
            assert rel <= NET_TOL[(arch, dtype_name)], (n, rel)
        _record(MEASURED, f"{arch}/{dtype_name}", worst)
        # the same rows whatever the batch cut: 33 tiles in one call == three calls, bit for bit
        whole = ex.extract_batch(tiles)
        parts = np.concatenate([ex.extract_batch(tiles[i:i + 11]) for i in (0, 11, 22)])
        assert np.array_equal(whole, parts)
    finally:
        ex.cleanup()


@pytest.mark.parametrize("arch", ["convnext_small", "convnext_base", "convnext_large"])
def test_deep_convnexts_float16(arch):
    tiles = _tiles(5, seed=4)
    want = _reference(arch, tiles, "t5")
    ex = _extractor(arch, "float16")
    try:
        got = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    rel = _rel(got, want)
    _record(MEASURED, f"{arch}/float16", rel)
    from atlaspatch_amd.encoders.convnext import ARCHS
    assert got.shape == (5, ARCHS[arch]["embed_dim"]) and rel <= NET_TOL[(arch, "float16")], rel


@pytest.mark.parametrize("arch", ["convnext_tiny", "convnext_small"], ids=["resize236_offset6", "resize230_offset3"])
def test_512px_tile_goes_through_the_device_resize(arch):
    from atlaspatch_amd.encoders.convnext import ARCHS
    spec = ARCHS[arch]
    tiles = _tiles(2, size=512, seed=6)
    want = ref.extract_batch(_canonical(arch), tiles, depths=spec["depths"], resize=spec["resize"])
    ex = _extractor(arch, "float32")
    try:
        got = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    rel = _rel(got, want)
    assert got.shape == (2, spec["embed_dim"]) and rel <= 1e-5, rel


def test_cli_process_with_the_shipped_plugin(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import atlaspatch_amd.plugins.torchvision_convnexts as plugin
    import atlaspatch_amd.plugins.torchvision_resnets as resnets
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, render_region
    from atlaspatch_amd.encoders.convnext import build_hip_convnext_extractor
    from atlaspatch_amd.utils.h5 import h5

    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "7")
    raw = {"width": 6000, "height": 5000, "seed": 9, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16]}
    slide = tmp_path / "s9.synth"
    slide.write_text(json.dumps(raw))
    out = tmp_path / "out"
    args = ["process", str(slide), "-o", str(out), "--patch-size", "256", "--target-mag", "20",
            "--feature-plugin", plugin.__file__, "--feature-plugin", resnets.__file__,
            "--feature-extractors", "convnext_tiny", "--feature-precision", "float16"]
    res = CliRunner().invoke(cli, args, catch_exceptions=False)
    assert res.exit_code == 0 and "failures: 0" in res.output, res.output
    with h5.File(out / "patches" / "s9.h5", "r") as f:
        coords = f["coords"][:]
        feats = f["features"]["convnext_tiny"][:]
    assert coords.shape[0] > 0 and feats.shape == (coords.shape[0], 768) and feats.dtype == np.float32
    assert np.isfinite(feats).all()
    spec = SynthSpec(width=raw["width"], height=raw["height"], seed=raw["seed"])
    rows = np.linspace(0, coords.shape[0] - 1, min(12, coords.shape[0])).astype(int)
    tiles = [render_region(spec, int(coords[r, 0]), int(coords[r, 1]), 256, 256, 0) for r in rows]
    ex = build_hip_convnext_extractor(name="convnext_tiny", arch="convnext_tiny", device="cuda", dtype=torch.float16,
                                      random_init_seed=7)
    try:
        direct = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    assert np.array_equal(feats[rows], direct)
