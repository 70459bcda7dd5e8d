"""ResNet encoders on the MI355X: the single operators (implicit-GEMM convolution, max / average pool) against torch, the
full networks against the CPU restatement (tests/resnet_reference.py), batch-cut invariance, the device resize of a
512-px tile, and `process` with the shipped plugin.

Bounds: float32 products are exact f32 MFMA chains (bound 1e-5 everywhere).  float16 / bfloat16 network bounds are the
first MI355X run's measured error x 1.2 (the measured value is next to each bound)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resnet_reference as ref
from tests.helpers import DT, _conv_bound_ratio, _lib, _record, _rel, _tiles, _tiles33

pytestmark = pytest.mark.gpu

# element-type rounding of the stored output is the only error of one convolution besides f32 summation order
CONV_TOL = {"float32": 1e-5, "float16": 1e-3, "bfloat16": 8e-3}
# network features against the CPU float32 restatement (measured on the first MI355X run; bound = measured x 1.2)
NET_TOL = {("resnet18", "float32"): 1e-5, ("resnet50", "float32"): 1e-5,                 # measured 5.6e-7 / 5.4e-7
           ("resnet18", "float16"): 1.05e-3, ("resnet50", "float16"): 9.8e-4,             # measured 8.76e-4 / 8.20e-4
           ("resnet18", "bfloat16"): 1.34e-2, ("resnet50", "bfloat16"): 9.0e-3,           # measured 1.115e-2 / 7.50e-3
           ("resnet101", "float16"): 1.1e-3, ("resnet152", "float16"): 6.3e-4}            # measured 9.16e-4 / 5.23e-4
MEASURED = "ATLASPATCH_RESNET_MEASURED"      # optional: names the path to record the measured errors in (bound updates)


def _layer_shapes():
    """{(k, stride, cin, cout, h)} of every convolution of the five networks (the stem's cin padded to 8)."""
    from atlaspatch_amd.encoders.resnet import ARCHS, conv_layers
    shapes = set()
    for arch, spec in ARCHS.items():
        hw = 56
        cur = None
        for name, cout, cin, k, stride in conv_layers(arch):
            if name == "conv1":
                shapes.add((7, 2, 8, cout, 224))
                continue
            blk = name.rsplit(".", 1)[0]
            if blk != cur:
                if cur is not None:
                    hw = hw_out
                cur = blk
                bstride = 2 if (name.startswith(("layer2", "layer3", "layer4")) and ".0." in name) else 1
                hw_out = (hw - 1) // bstride + 1
            conv_in = hw
            if spec["block"] == "bottleneck" and name.endswith("conv3"):
                conv_in = hw_out
            if spec["block"] == "basic" and name.endswith("conv2"):
                conv_in = hw_out
            shapes.add((k, stride, cin, cout, conv_in))
    return sorted(shapes)


SHAPES = _layer_shapes()


def _conv(dtype_name, x, w, b, stride, pad, resid=None, relu=False):
    """x [n, h, w, cin] T, w [cout, k, k, cin] T, b f32 [cout] (device) -> out [n, ho, wo, cout] T via ap_conv2d_nhwc."""
    lib, L = _lib()
    n, h, wd, cin = x.shape
    cout, k = w.shape[0], w.shape[1]
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    out = torch.empty((n, ho, wo, cout), dtype=x.dtype, device=x.device)
    lib.check(L.ap_conv2d_nhwc(DT[dtype_name][1], x.data_ptr(), n, h, wd, cin, w.data_ptr(), b.data_ptr(), cout, k, stride, pad,
                               resid.data_ptr() if resid is not None else None, 1 if relu else 0, out.data_ptr(),
                               lib.current_stream_ptr(x.device)), "ap_conv2d_nhwc")
    torch.cuda.synchronize()
    return out


def _conv_case(dtype_name, k, stride, cin, cout, h, n, resid, relu, seed=0, elementwise=False):
    dt = DT[dtype_name][0]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, h, generator=g).to(dt)
    w = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).to(dt)
    b = 0.1 * torch.randn(cout, generator=g)
    pad = k // 2
    ho = (h + 2 * pad - k) // stride + 1
    r = torch.randn(n, cout, ho, ho, generator=g).to(dt) if resid else None
    want = F.conv2d(x.float(), w.float(), b, stride=stride, padding=pad)        # CPU, on the operands as rounded to T
    if r is not None:
        want = want + r.float()
    if relu:
        want = F.relu(want)
    dev = torch.device("cuda")
    got = _conv(dtype_name, x.permute(0, 2, 3, 1).contiguous().to(dev), w.permute(0, 2, 3, 1).contiguous().to(dev), b.to(dev),
                stride, pad, r.permute(0, 2, 3, 1).contiguous().to(dev) if r is not None else None, relu)
    got = got.float().cpu().permute(0, 3, 1, 2)
    if elementwise:                 # the sharper check: every element inside the derived bound (tests/helpers.py::_conv_bound_ratio)
        ratio = _conv_bound_ratio(got, x, w, b, stride, pad, r, 1 if relu else 0, dtype_name)
        assert ratio <= 1.0, ratio
    return _rel(got, want)


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d_s%d_cin%d_cout%d_h%d" % s)
def test_conv2d_every_layer_shape(shape, dtype_name):
    k, stride, cin, cout, h = shape
    rel = _conv_case(dtype_name, k, stride, cin, cout, h, n=1, resid=False, relu=False, elementwise=True)
    assert rel <= CONV_TOL[dtype_name], rel


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("case", [(3, 1, 512, 512, 7, True, True), (1, 1, 512, 2048, 7, True, True), (3, 2, 256, 256, 14, False, True),
                                  (1, 2, 1024, 2048, 14, False, False), (3, 1, 64, 64, 56, True, False)],
                         ids=["3x3_7px_resid_relu", "1x1_7px_resid_relu", "3x3s2_relu", "1x1s2_proj", "3x3_56px_resid"])
def test_conv2d_m_tails_and_epilogues(case, n, dtype_name):
    k, stride, cin, cout, h, resid, relu = case
    if n == 33 and h == 56:
        n = 5
    rel = _conv_case(dtype_name, k, stride, cin, cout, h, n=n, resid=resid, relu=relu, seed=n)
    assert rel <= CONV_TOL[dtype_name], rel


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("hw,c,n", [(112, 64, 3), (15, 64, 2), (7, 128, 1)])
def test_maxpool_and_avgpool(hw, c, n, dtype_name):
    lib, L = _lib()
    dt, code = DT[dtype_name]
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(hw)
    x = torch.randn(n, c, hw, hw, generator=g).abs().to(dt)          # post-ReLU activations: no cancellation in the mean
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    ho = (hw - 1) // 2 + 1
    mp = torch.empty((n, ho, ho, c), dtype=dt, device=dev)
    lib.check(L.ap_maxpool3x3s2_nhwc(code, xd.data_ptr(), n, hw, hw, c, mp.data_ptr(), lib.current_stream_ptr(dev)), "maxpool")
    ap = torch.empty((n, c), dtype=torch.float32, device=dev)
    lib.check(L.ap_avgpool_nhwc(code, xd.data_ptr(), n, hw * hw, c, ap.data_ptr(), lib.current_stream_ptr(dev)), "avgpool")
    torch.cuda.synchronize()
    want_mp = F.max_pool2d(x.float(), 3, 2, 1).to(dt)
    assert torch.equal(mp.cpu().permute(0, 3, 1, 2), want_mp)
    want_ap = x.double().mean(dim=(2, 3))
    assert _rel(ap.cpu(), want_ap) <= 1e-5                          # a sequential f32 sum of hw * hw terms


# ----------------------------------------------------------------------------- full networks
_REF_CACHE = {}


def _canonical(arch, seed=3):
    from atlaspatch_amd.encoders.resnet import random_canonical_state_dict
    key = (arch, seed)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = random_canonical_state_dict(arch, seed)
    return _REF_CACHE[key]


def _reference(arch, tiles, tag):
    from atlaspatch_amd.encoders.resnet import ARCHS
    key = (arch, tag)
    if key not in _REF_CACHE:
        spec = ARCHS[arch]
        _REF_CACHE[key] = ref.extract_batch(_canonical(arch), tiles, block=spec["block"], depths=spec["depths"])
    return _REF_CACHE[key]


def _extractor(arch, dtype_name, **kw):
    from atlaspatch_amd.encoders.resnet import build_hip_resnet_extractor
    return build_hip_resnet_extractor(name=arch, arch=arch, device="cuda", dtype=DT[dtype_name][0],
                                      state_dict=_canonical(arch), **kw)


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_extract_batch_full_depth_against_the_restatement(arch, dtype_name):
    tiles = _tiles33()
    want_all = _reference(arch, tiles, "t33")
    ex = _extractor(arch, dtype_name)
    try:
        dim = 512 if arch == "resnet18" else 2048
        empty = ex.extract_batch([])
        assert empty.shape == (0, dim) and empty.dtype == np.float32
        worst = 0.0
        for n in (1, 5, 32, 33):
            got = ex.extract_batch(tiles[:n], batch_size=32)
            assert got.shape == (n, dim) and got.dtype == np.float32 and np.isfinite(got).all()
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


@pytest.mark.parametrize("arch", ["resnet101", "resnet152"])
def test_extract_batch_deep_bottlenecks_float16(arch):
    tiles = _tiles(5, seed=4)
    want = _reference(arch, tiles, "t5")
    ex = _extractor(arch, "float16")
    try:
        got = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    rel = _rel(got, want)
    _record(MEASURED, f"{arch}/float16", rel)
    assert got.shape == (5, 2048) and rel <= NET_TOL[(arch, "float16")], rel


def test_512px_tile_goes_through_the_device_resize():
    tiles = _tiles(3, size=512, seed=6)
    from atlaspatch_amd.encoders.resnet import ARCHS
    spec = ARCHS["resnet18"]
    want = ref.extract_batch(_canonical("resnet18"), tiles, block=spec["block"], depths=spec["depths"])
    ex = _extractor("resnet18", "float32")
    try:
        got = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    rel = _rel(got, want)
    assert got.shape == (3, 512) and rel <= 1e-5, rel


def test_cli_process_with_the_shipped_plugin(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import atlaspatch_amd.plugins.torchvision_resnets as plugin
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, render_region
    from atlaspatch_amd.encoders.resnet import build_hip_resnet_extractor
    from atlaspatch_amd.utils.h5 import h5

    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "7")
    raw = {"width": 6000, "height": 5000, "seed": 9, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16]}
    slide = tmp_path / "s9.synth"
    slide.write_text(json.dumps(raw))
    out = tmp_path / "out"
    args = ["process", str(slide), "-o", str(out), "--patch-size", "256", "--target-mag", "20",
            "--feature-plugin", plugin.__file__, "--feature-extractors", "resnet50", "--feature-precision", "float16"]
    res = CliRunner().invoke(cli, args, catch_exceptions=False)
    assert res.exit_code == 0 and "failures: 0" in res.output, res.output
    with h5.File(out / "patches" / "s9.h5", "r") as f:
        coords = f["coords"][:]
        feats = f["features"]["resnet50"][:]
    assert coords.shape[0] > 0 and feats.shape == (coords.shape[0], 2048) and feats.dtype == np.float32
    assert np.isfinite(feats).all()
    spec = SynthSpec(width=raw["width"], height=raw["height"], seed=raw["seed"])
    rows = np.linspace(0, coords.shape[0] - 1, min(12, coords.shape[0])).astype(int)
    tiles = [render_region(spec, int(coords[r, 0]), int(coords[r, 1]), 256, 256, 0) for r in rows]
    ex = build_hip_resnet_extractor(name="resnet50", arch="resnet50", device="cuda", dtype=torch.float16, random_init_seed=7)
    try:
        direct = ex.extract_batch(tiles)
    finally:
        ex.cleanup()
    assert np.array_equal(feats[rows], direct)
