"""A plugin's torch module on the tile ring: the device transform against the host chain (bit for bit), the two routes of one
registered model against each other, and ``process`` end to end through both tile sources.

The host chain is stated here with Pillow, numpy and torch on the CPU, never with the code under test: ``PIL.resize``, the crop,
``((x.float() / 255) - mean) / std`` in float32, ``.to(dtype)``.  The resampler gives Pillow's bytes and the preprocess kernel
performs torchvision's arithmetic, so float32 / float16 / bfloat16 results are compared as bit patterns.

Route bounds: the same torch kernels on bit-equal inputs of the same shape give the same bits (model chunk = n on both
routes).  Where the chunk shapes differ (32 + 32 + 3 against 67) torch may pick other kernels per shape: a 3 x 3 x 3 convolution,
a mean over < 2^10 values and an 8-term dot product in float32 differ by a few ulp of the largest term, bounded here by
1e-5 of the row's largest magnitude (float32 eps is 6e-8); a wrong chunk offset or a dropped tail is O(1)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PIL_CODE = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}
INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _tiles(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _host_chain(tile, resized_hw, filt, box, dtype, mean=MEAN, std=STD):
    """One tile uint8 [H, W, 3] -> dtype [3, oh, ow]; ``resized_hw`` None = no resize; ``box`` = (top, left, oh, ow)."""
    image = Image.fromarray(tile)
    if resized_hw is not None:
        image = image.resize((resized_hw[1], resized_hw[0]), PIL_CODE[filt])
    top, left, oh, ow = box
    arr = np.asarray(image)[top:top + oh, left:left + ow].copy()
    x = torch.from_numpy(arr).permute(2, 0, 1)
    y = ((x.float() / 255) - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    return y.to(dtype)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(INT_VIEW[a.dtype]), b.contiguous().view(INT_VIEW[b.dtype]))


# (tile h x w, DeviceTransform arguments, resized h x w or None, (top, left, oh, ow)): sizes and offsets derived by hand --
# 37 x 53, Resize(24): 24 x int(24 * 53 / 37) = 24 x 34; CenterCrop(16): round(8 / 2) = 4, round(18 / 2) = 9
TRANSFORM_CASES = [
    ((37, 53), dict(resize=24, crop=16), (24, 34), (4, 9, 16, 16)),
    ((64, 64), dict(resize=(20, 28)), (20, 28), (0, 0, 20, 28)),                 # a width that is no multiple of 8
    ((37, 53), dict(crop=(16, 21)), None, (10, 16, 16, 21)),                     # round(21 / 2) = round(10.5) = 10 (half to even); 32 / 2 = 16
    ((64, 64), dict(crop=32), None, (16, 16, 32, 32)),
    ((37, 53), dict(), None, (0, 0, 37, 53)),                                    # identity, five bands of rows, the last one of 5
    ((64, 64), dict(), None, (0, 0, 64, 64)),
    ((16, 20), dict(resize=32, crop=(32, 40)), (32, 40), (0, 0, 32, 40)),        # upscaling
]


@pytest.mark.parametrize("filt", ["bilinear", "bicubic", "lanczos"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["float32", "float16", "bfloat16"])
def test_transform_is_the_host_chain_bit_for_bit(dtype, filt):
    from atlaspatch_amd.encoders.device_transform import DeviceTransform
    for (h, w), kw, resized, box in TRANSFORM_CASES:
        t = DeviceTransform(interpolation=filt, mean=MEAN, std=STD, **kw)
        assert t.plan((h, w)) == (resized or (h, w), box[0], box[1], (box[2], box[3]))
        tiles = _tiles(3, h, w, seed=h * w)
        got = t(torch.from_numpy(tiles).to(DEV), dtype)
        want = torch.stack([_host_chain(tile, resized, filt, box, dtype) for tile in tiles])
        assert got.device.type == "cuda" and got.is_contiguous()
        got = got.cpu()
        diff = int((got.view(INT_VIEW[dtype]) != want.view(INT_VIEW[dtype])).sum()) if got.shape == want.shape else -1
        assert diff == 0, f"{(h, w)} {kw} {filt} {dtype}: {diff} of {want.numel()} elements differ"
        assert t(torch.empty((0, h, w, 3), dtype=torch.uint8, device=DEV), dtype).shape == (0, 3, box[2], box[3])


def test_transform_runs_on_the_current_stream_and_takes_views():
    """A side stream, and a non-contiguous batch (every other tile): the same bits."""
    from atlaspatch_amd.encoders.device_transform import DeviceTransform
    t = DeviceTransform(resize=24, interpolation="bicubic", crop=16, mean=MEAN, std=STD)
    tiles = _tiles(6, 37, 53, seed=3)
    dev = torch.from_numpy(tiles).to(DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = t(dev[::2], torch.float32)
    side.synchronize()
    want = torch.stack([_host_chain(tile, (24, 34), "bicubic", (4, 9, 16, 16), torch.float32) for tile in tiles[::2]])
    assert _same_bits(got.cpu(), want)
    with pytest.raises(ValueError, match="uint8"):
        t(dev.float(), torch.float32)
    with pytest.raises(ValueError, match="larger than the resized image"):
        DeviceTransform(crop=64)(dev, torch.float32)


def test_preproc_chw_any_through_the_c_abi():
    """ap_preproc_u8hwc_to_chw_any: any output width in torchvision's arithmetic; a multiple of 8 gives the bits of
    ap_preproc_u8hwc_to_chw, which keeps refusing every other width; windows outside the image are refused before a launch."""
    from atlaspatch_amd import _lib
    lib = _lib.load()
    n, h, w = 5, 29, 43
    tiles = _tiles(n, h, w, seed=11)
    src = torch.from_numpy(tiles).to(DEV)
    stream = _lib.current_stream_ptr(DEV)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        code = _lib.torch_dtype_code(dtype)
        for top, left, oh, ow in ((0, 0, 29, 43), (3, 5, 19, 27), (28, 42, 1, 1), (2, 1, 17, 40)):
            out = torch.full((n, 3, oh, ow), -7.0, dtype=dtype, device=DEV)
            _lib.check(lib.ap_preproc_u8hwc_to_chw_any(src.data_ptr(), n, h, w, top, left, oh, ow, _lib.f3(MEAN), _lib.f3(STD),
                                                       out.data_ptr(), code, stream), "ap_preproc_u8hwc_to_chw_any")
            want = torch.stack([_host_chain(tile, None, None, (top, left, oh, ow), dtype) for tile in tiles])
            assert _same_bits(out.cpu(), want), (dtype, top, left, oh, ow)
            if ow % 8 == 0:
                ref = torch.empty_like(out)
                _lib.check(lib.ap_preproc_u8hwc_to_chw(src.data_ptr(), n, h, w, top, left, oh, ow, _lib.f3(MEAN), _lib.f3(STD),
                                                       ref.data_ptr(), code, stream), "ap_preproc_u8hwc_to_chw")
                assert _same_bits(out.cpu(), ref.cpu())
    out = torch.zeros((n, 3, 29, 43), dtype=torch.float32, device=DEV)
    head = (src.data_ptr(), n, h, w)
    tail = (_lib.f3(MEAN), _lib.f3(STD), out.data_ptr(), 0, stream)
    assert lib.ap_preproc_u8hwc_to_chw(*head, 0, 0, 29, 43, *tail) == _lib.AP_ERR_INVALID and b"multiple of 8" in lib.ap_last_error()
    for window in ((0, 0, 30, 43), (0, 1, 29, 43), (-1, 0, 29, 43), (1, 0, 29, 43), (0, 0, 29, 0), (0, 0, 0, 43)):
        assert lib.ap_preproc_u8hwc_to_chw_any(*head, *window, *tail) == _lib.AP_ERR_INVALID, window
        assert b"preproc_chw_any" in lib.ap_last_error()
    assert lib.ap_preproc_u8hwc_to_chw_any(*head, 0, 0, 29, 43, _lib.f3(MEAN), _lib.f3(STD), out.data_ptr(), 3, stream) == _lib.AP_ERR_INVALID
    assert lib.ap_preproc_u8hwc_to_chw_any(src.data_ptr(), 0, h, w, 0, 0, 29, 43, *tail) == 0
    torch.cuda.synchronize(DEV)
    assert float(out.abs().max()) == 0.0                                          # no refused or empty call wrote


# ----------------------------------------------------------------------------- the two routes of one registered model
class Tiny(torch.nn.Module):
    """conv 3 -> 8 (3 x 3), ReLU, global mean, linear 8 -> 16; ``shape`` = what forward returns per tile."""

    def __init__(self, shape=(16,), width=16):
        super().__init__()
        gen = torch.Generator().manual_seed(1234)
        self.conv = torch.nn.Conv2d(3, 8, 3)
        self.head = torch.nn.Linear(8, width)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
        self.shape = shape

    def forward(self, x):
        y = self.head(torch.relu(self.conv(x)).mean(dim=(2, 3)))
        return y.reshape(y.shape[0], *self.shape)


def _pil_preprocess(image):
    """Resize(24, bicubic) -> CenterCrop(16) -> ToTensor -> Normalize with Pillow and numpy (torch only carries the result)."""
    w, h = image.size
    if min(w, h) != 24:
        image = image.resize((24, int(24 * h / w)) if w <= h else (int(24 * w / h), 24), Image.Resampling.BICUBIC)
    w, h = image.size
    top, left = int(round((h - 16) / 2.0)), int(round((w - 16) / 2.0))
    arr = np.asarray(image, dtype=np.uint8)[top:top + 16, left:left + 16].astype(np.float32)
    arr = (arr / np.float32(255) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


def _fixed_preprocess(image):
    """Any tile -> 16 x 16 bilinear, ToTensor: a host transform that takes tiles smaller than the crop."""
    arr = np.asarray(image.resize((16, 16), Image.Resampling.BILINEAR), dtype=np.uint8).astype(np.float32) / np.float32(255)
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


def _pair(dtype=torch.float32, model=None, device_batch=32, preprocess=_pil_preprocess, transform=None):
    """The same model registered twice through register_custom_encoder: (host route, ring route)."""
    from atlaspatch_amd.encoders.custom import CustomEncoderComponents, register_custom_encoder
    from atlaspatch_amd.encoders.device_transform import DeviceTransform
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry
    transform = transform or DeviceTransform(resize=24, interpolation="bicubic", crop=16, mean=MEAN, std=STD)
    model = model or Tiny()
    registry = PatchFeatureExtractorRegistry()
    register_custom_encoder(registry=registry, name="tiny_host", embedding_dim=16, device=DEV, dtype=dtype,
                            loader=lambda d, t: CustomEncoderComponents(model, preprocess))
    register_custom_encoder(registry=registry, name="tiny_ring", embedding_dim=16, device=DEV, dtype=dtype, device_batch=device_batch,
                            loader=lambda d, t: CustomEncoderComponents(model, preprocess, device_transform=transform))
    return registry.create("tiny_host"), registry.create("tiny_ring")


def _within_row_bound(got, want, rel=1e-5):
    bound = rel * np.abs(want).max(axis=1, keepdims=True)
    return got.shape == want.shape and bool((np.abs(got - want) <= bound).all())


@pytest.fixture(scope="module")
def patches():
    return {hw: list(_tiles(67, *hw, seed=sum(hw))) for hw in ((37, 53), (64, 64))}


def test_registration_picks_the_class_by_the_loaders_answer():
    from atlaspatch_amd.encoders.base import DeviceTorchFeatureExtractor, PatchFeatureExtractor
    from atlaspatch_amd.services.feature_embedding import _speaks_ring
    host, ring = _pair()
    assert type(host) is PatchFeatureExtractor and not _speaks_ring(host)
    assert type(ring) is DeviceTorchFeatureExtractor and _speaks_ring(ring) and ring.max_batch == 32 and ring.embedding_dim == 16


@pytest.mark.parametrize("hw", [(37, 53), (64, 64)], ids=["37x53", "64x64"])
@pytest.mark.parametrize("n", [1, 3, 67])
def test_routes_agree_bit_for_bit_at_the_same_chunk(patches, n, hw):
    host, ring = _pair()
    part = patches[hw][:n]
    want = host.extract_batch(part, batch_size=n)
    ring.max_batch = n
    out = torch.full((n, 16), float("nan"), dtype=torch.float32, device=DEV)
    got = ring.forward_device(torch.from_numpy(np.stack(part)).to(DEV), out)
    assert got is out and want.shape == (n, 16) and np.abs(want).max() > 0.1
    assert np.array_equal(got.cpu().numpy(), want)
    # extract_batch of the ring extractor: the pinned upload in front of the same forward; batch_size is the model chunk
    assert np.array_equal(ring.extract_batch(part, batch_size=n), want)
    assert np.array_equal(ring.extract_device(torch.from_numpy(np.stack(part)).to(DEV)).cpu().numpy(), want)


def test_routes_agree_in_float16():
    host, ring = _pair(dtype=torch.float16)
    part = list(_tiles(3, 37, 53, seed=8))
    want = host.extract_batch(part, batch_size=3)
    ring.max_batch = 3
    got = ring.extract_batch(part)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_chunks_of_32_cover_67_tiles(patches):
    host, ring = _pair(device_batch=32)
    part = patches[(37, 53)]
    want = host.extract_batch(part, batch_size=67)
    out = torch.full((67, 16), float("nan"), dtype=torch.float32, device=DEV)
    got = ring.forward_device(torch.from_numpy(np.stack(part)).to(DEV), out).cpu().numpy()
    worst = float((np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True)).max())
    print(f"chunks 32 + 32 + 3 against one chunk of 67: worst element {worst:.3e} of its row's largest magnitude")
    assert _within_row_bound(got, want)
    chunked = ring.extract_batch(part, batch_size=32)                # the operator's batch_size: 32 + 32 + 3 through the pinned upload
    assert _within_row_bound(chunked, want) and np.array_equal(chunked, got)
    assert len({row.tobytes() for row in got}) == 67                 # 67 different tiles, 67 different rows: nothing repeated


def test_empty_batches():
    _, ring = _pair()
    assert ring.extract_batch([]).shape == (0, 16) and ring.extract_batch([]).dtype == np.float32
    out = torch.empty((0, 16), dtype=torch.float32, device=DEV)
    assert ring.forward_device(torch.empty((0, 37, 53, 3), dtype=torch.uint8, device=DEV), out).shape == (0, 16)


def test_spatial_outputs_are_flattened_and_a_wrong_width_raises_before_a_write():
    tiles = torch.from_numpy(_tiles(3, 37, 53, seed=4)).to(DEV)
    _, flat = _pair()
    _, spatial = _pair(model=Tiny(shape=(16, 1, 1)))
    a = flat.forward_device(tiles, torch.empty((3, 16), dtype=torch.float32, device=DEV))
    b = spatial.forward_device(tiles, torch.empty((3, 16), dtype=torch.float32, device=DEV))
    assert torch.equal(a, b)
    _, wrong = _pair(model=Tiny(shape=(12,), width=12))
    out = torch.full((3, 16), 5.0, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match=r"returned \(3, 12\).*\[3, 16\]"):
        wrong.forward_device(tiles, out)
    assert bool((out == 5.0).all())
    with pytest.raises(ValueError, match="embedding_dim"):
        wrong.extract_batch(list(_tiles(3, 37, 53, seed=4)))
    # forward_fn takes the place of the model's forward on both routes
    from atlaspatch_amd.encoders.custom import CustomEncoderComponents, register_custom_encoder
    from atlaspatch_amd.encoders.device_transform import DeviceTransform
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry
    model = Tiny()
    registry = PatchFeatureExtractorRegistry()
    register_custom_encoder(registry=registry, name="doubled", embedding_dim=16, device=DEV, dtype=torch.float32,
                            loader=lambda d, t: CustomEncoderComponents(model, _pil_preprocess, lambda x: model(x) * 2,
                                                                        DeviceTransform(resize=24, interpolation=3, crop=16, mean=MEAN, std=STD)))
    c = registry.create("doubled").forward_device(tiles, torch.empty((3, 16), dtype=torch.float32, device=DEV))
    assert torch.equal(c, a * 2)


def test_tiles_the_plan_refuses_take_the_host_route():
    """8 x 12 tiles under CenterCrop(16): the device transform refuses (torchvision would pad), so the extractor is a
    PatchFeatureExtractor for them -- the plugin's own preprocess on the host -- and still returns features."""
    from atlaspatch_amd.encoders.device_transform import DeviceTransform
    host, ring = _pair(preprocess=_fixed_preprocess, transform=DeviceTransform(crop=16))
    small = list(_tiles(5, 8, 12, seed=6))
    want = host.extract_batch(small, batch_size=32)
    assert np.array_equal(ring.extract_batch(small, batch_size=32), want)
    out = torch.full((5, 16), float("nan"), dtype=torch.float32, device=DEV)
    got = ring.forward_device(torch.from_numpy(np.stack(small)).to(DEV), out)
    assert np.array_equal(got.cpu().numpy(), want) and np.isfinite(want).all()
    # PIL images go to the plugin's preprocess as they are
    assert np.array_equal(ring.extract_batch([Image.fromarray(p) for p in small], batch_size=32), want)


# ----------------------------------------------------------------------------- process, end to end
PLUGIN = '''
import numpy as np
import torch
from PIL import Image
from atlaspatch_amd.encoders.custom import CustomEncoderComponents, register_custom_encoder
from atlaspatch_amd.encoders.device_transform import DeviceTransform

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(1234)
        self.conv = torch.nn.Conv2d(3, 8, 3)
        self.head = torch.nn.Linear(8, 16)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)

    def forward(self, x):
        return self.head(torch.relu(self.conv(x)).mean(dim=(2, 3)))


def preprocess(image):                       # Resize(32, bicubic) -> CenterCrop(24) -> ToTensor -> Normalize, Pillow and numpy
    w, h = image.size
    if min(w, h) != 32:
        image = image.resize((32, int(32 * h / w)) if w <= h else (int(32 * w / h), 32), Image.Resampling.BICUBIC)
    arr = np.asarray(image, dtype=np.uint8)[4:28, 4:28].astype(np.float32)
    arr = (arr / np.float32(255) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


def register_feature_extractors(registry, device, dtype, num_workers):
    transform = DeviceTransform(resize=32, interpolation="bicubic", crop=24, mean=MEAN, std=STD)
    for name, described in (("tiny_ring", transform), ("tiny_host", None)):
        register_custom_encoder(registry=registry, name=name, embedding_dim=16, device=device, dtype=dtype, num_workers=num_workers,
                                device_batch=96,
                                loader=lambda d, t, described=described: CustomEncoderComponents(Tiny(), preprocess, device_transform=described))
'''


@pytest.mark.parametrize("case", ["device tile source", "pinned ring", "read size 512"])
def test_process_runs_the_plugin_on_the_ring(case, tmp_path, monkeypatch):
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services.feature_embedding import PatchFeatureEmbeddingService
    from atlaspatch_amd.utils.h5 import h5

    if case == "pinned ring":
        monkeypatch.setenv("ATLASPATCH_HOST_TILES", "1")
    ring_runs = []
    inner = PatchFeatureEmbeddingService.embed_matrix

    def counted(self, result, wsi, extractor, **kw):
        ring_runs.append(extractor.name)
        return inner(self, result, wsi, extractor, **kw)

    monkeypatch.setattr(PatchFeatureEmbeddingService, "embed_matrix", counted)
    plugin = tmp_path / "tiny_plugin.py"
    plugin.write_text(PLUGIN)
    slide = tmp_path / "s9.synth"
    slide.write_text(json.dumps({"width": 6000, "height": 5000, "seed": 9, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16]}))
    out = tmp_path / "out"

    def process(name):
        args = ["process", str(slide), "-o", str(out), "--patch-size", "256", "--target-mag", "10" if case == "read size 512" else "20",
                "--feature-plugin", str(plugin), "--feature-extractors", name, "--feature-precision", "float32"]
        res = CliRunner().invoke(cli, args, catch_exceptions=False)
        assert res.exit_code == 0 and "failures: 0" in res.output, res.output

    h5_path = out / "patches" / "s9.h5"
    process("tiny_ring")
    assert ring_runs == ["tiny_ring"] and not (out / "patches" / "s9.lock").exists()
    with h5.File(h5_path, "r") as f:
        coords = f["coords"][:]
        ring = f["features"]["tiny_ring"][:]
    assert coords.shape[0] > 8 and ring.shape == (coords.shape[0], 16) and ring.dtype == np.float32 and np.isfinite(ring).all()
    assert int(coords[0, 2]) == (512 if case == "read size 512" else 256)          # 512-px reads: cv2-exact resize to 256 in front of the transform

    process("tiny_host")                                                           # the same coordinates, the host route
    assert ring_runs == ["tiny_ring"]
    with h5.File(h5_path, "r") as f:
        host = f["features"]["tiny_host"][:]
        assert np.array_equal(f["features"]["tiny_ring"][:], ring)
    worst = float((np.abs(ring - host) / np.abs(host).max(axis=1, keepdims=True)).max())
    print(f"{case}: {coords.shape[0]} tiles, worst element {worst:.3e} of its row's largest magnitude between the routes")
    assert _within_row_bound(ring, host)
    assert len({row.tobytes() for row in ring}) > coords.shape[0] // 2             # rows follow their tiles

    before = os.path.getmtime(h5_path)
    process("tiny_ring")                                                           # --skip-existing is the default: nothing embeds
    assert ring_runs == ["tiny_ring"] and os.path.getmtime(h5_path) == before


def test_gather_blocks_are_kept_for_a_plugin_on_the_ring(tmp_path, monkeypatch):
    """``_keep_blocks`` (the rank-sharded gather's cache) holds the ring's matrix of a plugin encoder as of a native one."""
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services.feature_embedding import PatchFeatureEmbeddingService
    from atlaspatch_amd.utils.h5 import h5
    kept = {}
    inner = PatchFeatureEmbeddingService.embed_all

    def spying(self, results, **kw):
        self._keep_blocks = True
        try:
            return inner(self, results, **kw)
        finally:
            kept.update(self.feature_blocks)

    monkeypatch.setattr(PatchFeatureEmbeddingService, "embed_all", spying)
    plugin = tmp_path / "tiny_plugin.py"
    plugin.write_text(PLUGIN)
    slide = tmp_path / "s9.synth"
    slide.write_text(json.dumps({"width": 6000, "height": 5000, "seed": 9, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16]}))
    out = tmp_path / "out"
    res = CliRunner().invoke(cli, ["process", str(slide), "-o", str(out), "--patch-size", "256", "--target-mag", "20", "--feature-plugin",
                                   str(plugin), "--feature-extractors", "tiny_ring", "--feature-precision", "float16"], catch_exceptions=False)
    assert res.exit_code == 0 and "failures: 0" in res.output, res.output
    with h5.File(out / "patches" / "s9.h5", "r") as f:
        feats = f["features"]["tiny_ring"][:]
    assert [(os.path.realpath(path), name) for path, name in kept] == [(os.path.realpath(out / "patches" / "s9.h5"), "tiny_ring")]
    assert np.array_equal(next(iter(kept.values())), feats) and feats.shape[1] == 16
