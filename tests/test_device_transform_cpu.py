"""The device transform of plugin encoders, as far as it is host logic (no GPU): the plan (torchvision's size and crop rules,
derived by hand below), the three Pillow filter tables added for it (box, hamming, lanczos) against ``PIL.Image.resize`` byte
for byte, ``DeviceTransform.from_torchvision`` on stand-in classes (torchvision is not a dependency), and the plugin API's
unchanged defaults."""
import enum

import numpy as np
import pytest
import torch

from atlaspatch_amd.encoders.device_transform import DeviceTransform


# ----------------------------------------------------------------------------- plan
def test_plan_resize_rules_by_hand():
    # Resize(int): shorter side -> size, the other side int(size * long / short); untouched when the shorter side is size already
    assert DeviceTransform(resize=224).plan((256, 256)) == ((224, 224), 0, 0, (224, 224))
    assert DeviceTransform(resize=256).plan((256, 256)) == ((256, 256), 0, 0, (256, 256))
    # 37 x 53 (h x w), size 24: h is the shorter side -> 24; w -> int(24 * 53 / 37) = int(34.378...) = 34
    assert DeviceTransform(resize=24).plan((37, 53)) == ((24, 34), 0, 0, (24, 34))
    assert DeviceTransform(resize=24).plan((53, 37)) == ((34, 24), 0, 0, (34, 24))
    # the shorter side already is 24: no resize, whatever the other side
    assert DeviceTransform(resize=24).plan((24, 100))[0] == (24, 100)
    assert DeviceTransform(resize=24).plan((100, 24))[0] == (100, 24)
    # (h, w): exactly that; None: untouched; [s] is s
    assert DeviceTransform(resize=(20, 28)).plan((64, 64)) == ((20, 28), 0, 0, (20, 28))
    assert DeviceTransform(resize=[20, 28]).plan((37, 53))[0] == (20, 28)
    assert DeviceTransform().plan((37, 53)) == ((37, 53), 0, 0, (37, 53))
    assert DeviceTransform(resize=[24]).plan((37, 53))[0] == (24, 34)
    # upscaling follows the same rule: 16 x 20 -> size 32: 32 x int(32 * 20 / 16) = 40
    assert DeviceTransform(resize=32).plan((16, 20))[0] == (32, 40)


def test_plan_crop_offsets_round_half_to_even():
    # offsets int(round((H - h) / 2.0)): (H - h) even
    assert DeviceTransform(resize=24, crop=16).plan((37, 53)) == ((24, 34), 4, 9, (16, 16))
    # (H - h) odd: 1 / 2 = 0.5 -> 0 (half to even, not up); 3 / 2 = 1.5 -> 2; 5 / 2 = 2.5 -> 2; 7 / 2 = 3.5 -> 4
    assert DeviceTransform(crop=(16, 16)).plan((17, 19))[1:3] == (0, 2)
    assert DeviceTransform(crop=(16, 16)).plan((19, 17))[1:3] == (2, 0)
    assert DeviceTransform(crop=16).plan((21, 23))[1:3] == (2, 4)
    # crop (h, w) with different sides; crop equal to the image
    assert DeviceTransform(crop=(10, 20)).plan((37, 53)) == ((37, 53), 14, 16, (10, 20))      # 27 / 2 = 13.5 -> 14; 33 / 2 = 16.5 -> 16
    assert DeviceTransform(crop=(37, 53)).plan((37, 53)) == ((37, 53), 0, 0, (37, 53))
    # the crop follows the resize
    assert DeviceTransform(resize=256, crop=224).plan((300, 512)) == ((256, 436), 16, 106, (224, 224))   # int(256 * 512 / 300) = 436


def test_plan_refuses_an_oversized_crop_by_name():
    with pytest.raises(ValueError, match=r"crop 16x16 .* larger than the resized image 8x12"):
        DeviceTransform(crop=16).plan((8, 12))
    with pytest.raises(ValueError, match="larger than the resized image 24x34"):
        DeviceTransform(resize=24, crop=(16, 40)).plan((37, 53))
    # made when the plan is made, not at construction: the same transform is fine for larger tiles
    assert DeviceTransform(crop=16).plan((16, 16))[3] == (16, 16)


def test_interpolation_spellings_and_refusals():
    class Mode(enum.Enum):
        NEAREST = "nearest"
        BILINEAR = "bilinear"
        BICUBIC = "bicubic"
        LANCZOS = "lanczos"

    for spelling, want in ((2, "bilinear"), (3, "bicubic"), (1, "lanczos"), (4, "box"), (5, "hamming"), ("bilinear", "bilinear"),
                           ("BICUBIC", "bicubic"), ("lanczos", "lanczos"), ("box", "box"), ("hamming", "hamming"),
                           (Mode.BILINEAR, "bilinear"), (Mode.BICUBIC, "bicubic"), (Mode.LANCZOS, "lanczos")):
        assert DeviceTransform(resize=8, interpolation=spelling).filter == want, spelling
    from PIL import Image
    assert DeviceTransform(resize=8, interpolation=Image.Resampling.LANCZOS).filter == "lanczos"      # an IntEnum of Pillow's codes
    for nearest in (0, "nearest", Mode.NEAREST, "nearest-exact"):
        with pytest.raises(ValueError, match="nearest"):
            DeviceTransform(resize=8, interpolation=nearest)
    for bad in (6, "cubic", None, 2.0):
        with pytest.raises(ValueError, match="interpolation"):
            DeviceTransform(resize=8, interpolation=bad)
    with pytest.raises(ValueError, match="std"):
        DeviceTransform(std=(1, 0, 1))
    assert DeviceTransform(mean=0.5, std=[0.25]).mean == (0.5, 0.5, 0.5)
    assert DeviceTransform(mean=torch.tensor([0.1, 0.2, 0.3])).mean == tuple(float(np.float32(v)) for v in (0.1, 0.2, 0.3))


def test_resized_rule_is_shared_with_the_native_extractor():
    """One statement of Resize(int): the native extractor's ``resized`` and the plan call the same function."""
    import inspect
    from atlaspatch_amd.encoders import base, device_transform
    from atlaspatch_amd.utils.resample import shorter_side_hw
    assert shorter_side_hw((256, 256), 224) == (224, 224) and shorter_side_hw((131, 97), 224) == (302, 224)
    assert "shorter_side_hw" in inspect.getsource(base.HipViTFeatureExtractor.resized)
    assert "shorter_side_hw" in inspect.getsource(device_transform.DeviceTransform.plan)


# ----------------------------------------------------------------------------- the new filter tables
def _apply_tables(img, oh, ow, f):
    """Pillow's two passes (ImagingResampleHorizontal_8bpc / Vertical_8bpc): 22-bit fixed point, a uint8 intermediate."""
    from atlaspatch_amd.utils.resample import pillow_resample_tables
    h, w, c = img.shape
    bx, kx, _ = pillow_resample_tables(w, ow, f)
    by, ky, _ = pillow_resample_tables(h, oh, f)
    a = img.astype(np.int64)
    tmp = np.zeros((h, ow, c), np.uint8)
    for xx in range(ow):
        s = np.full((h, c), 1 << 21, np.int64)
        for x in range(bx[xx, 1]):
            s += a[:, bx[xx, 0] + x, :] * int(kx[xx, x])
        tmp[:, xx] = np.clip(s >> 22, 0, 255)
    t = tmp.astype(np.int64)
    out = np.zeros((oh, ow, c), np.uint8)
    for yy in range(oh):
        s = np.full((ow, c), 1 << 21, np.int64)
        for y in range(by[yy, 1]):
            s += t[by[yy, 0] + y] * int(ky[yy, y])
        out[yy] = np.clip(s >> 22, 0, 255)
    return out


@pytest.mark.parametrize("name", ["box", "hamming", "lanczos"])
def test_new_filter_tables_reproduce_pil(name):
    from PIL import Image
    from atlaspatch_amd.utils.resample import _FILTER_SUPPORT, _pillow_resample_tables_scalar, pillow_resample_tables
    assert _FILTER_SUPPORT[name] == {"box": 0.5, "hamming": 1.0, "lanczos": 3.0}[name]
    assert _FILTER_SUPPORT["bicubic"] == 2.0 and _FILTER_SUPPORT["bilinear"] == 1.0
    code = {"box": Image.Resampling.BOX, "hamming": Image.Resampling.HAMMING, "lanczos": Image.Resampling.LANCZOS}[name]
    rng = np.random.default_rng(5)
    for (h, w), (oh, ow) in (((37, 53), (24, 34)), ((16, 16), (29, 37)), ((256, 256), (224, 224))):   # 53 x 37 -> 34 x 24 (w x h) down, up, the usual
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(img).resize((ow, oh), code))
        assert np.array_equal(_apply_tables(img, oh, ow, name), want), (name, h, w)
        for size_in, size_out in ((h, oh), (w, ow)):                # the vector form and the loop form agree
            a, b = pillow_resample_tables(size_in, size_out, name), _pillow_resample_tables_scalar(size_in, size_out, name)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ----------------------------------------------------------------------------- from_torchvision on stand-ins
class InterpolationMode(enum.Enum):
    NEAREST = "nearest"
    BILINEAR = "bilinear"
    BICUBIC = "bicubic"
    LANCZOS = "lanczos"


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms


class Resize:
    def __init__(self, size, interpolation=InterpolationMode.BILINEAR, max_size=None, antialias=True):
        self.size, self.interpolation, self.max_size, self.antialias = size, interpolation, max_size, antialias


class CenterCrop:
    def __init__(self, size):
        self.size = (int(size), int(size)) if isinstance(size, int) else tuple(size)      # torchvision stores the pair


class ToTensor:
    pass


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std


class ColorJitter:
    pass


def _state(t):
    return t.resize, t.filter, t.crop, t.mean, t.std


def test_from_torchvision_reads_the_reference_chains():
    half = (0.5, 0.5, 0.5)
    # MUSK: Resize(384, interpolation=3, antialias=True), CenterCrop((384, 384)), ToTensor, Normalize(inception mean / std)
    musk = Compose([Resize(384, interpolation=3, antialias=True), CenterCrop((384, 384)), ToTensor(), Normalize(mean=half, std=half)])
    assert _state(DeviceTransform.from_torchvision(musk)) == (384, "bicubic", (384, 384), half, half)
    # Prov-GigaPath: Resize(256, BICUBIC), CenterCrop(224), ToTensor, Normalize(ImageNet)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    giga = Compose([Resize(256, interpolation=InterpolationMode.BICUBIC), CenterCrop(224), ToTensor(), Normalize(mean=mean, std=std)])
    t = DeviceTransform.from_torchvision(giga)
    assert _state(t) == (256, "bicubic", (224, 224), mean, std)
    assert t.plan((256, 256)) == ((256, 256), 16, 16, (224, 224)) and t.plan((512, 512)) == ((256, 256), 16, 16, (224, 224))
    # H-optimus: Resize((224, 224)) (bilinear by default), ToTensor, Normalize
    hmean, hstd = (0.707223, 0.578729, 0.703617), (0.211883, 0.230117, 0.177517)
    hopt = Compose([Resize((224, 224)), ToTensor(), Normalize(mean=hmean, std=hstd)])
    t = DeviceTransform.from_torchvision(hopt)
    assert _state(t) == ((224, 224), "bilinear", None, hmean, hstd) and t.plan((256, 300))[3] == (224, 224)
    # Midnight: Resize(224), CenterCrop(224), ToTensor, Normalize(0.5)
    mid = Compose([Resize(224), CenterCrop(224), ToTensor(), Normalize(mean=half, std=half)])
    assert _state(DeviceTransform.from_torchvision(mid)) == (224, "bilinear", (224, 224), half, half)
    # the shortest chain, and tensors for mean / std
    assert _state(DeviceTransform.from_torchvision(Compose([ToTensor()]))) == (None, "bilinear", None, (0.0,) * 3, (1.0,) * 3)
    t = DeviceTransform.from_torchvision(Compose([ToTensor(), Normalize(torch.tensor([0.5, 0.25, 0.125]), torch.tensor([2.0, 4.0, 8.0]))]))
    assert t.mean == (0.5, 0.25, 0.125) and t.std == (2.0, 4.0, 8.0)
    # antialias None / "warn" (older torchvision's defaults) are Pillow's behaviour too
    for aa in (None, "warn"):
        assert DeviceTransform.from_torchvision(Compose([Resize(8, antialias=aa), ToTensor()])).resize == 8


def test_from_torchvision_refuses_by_name():
    norm = Normalize((0.5,) * 3, (0.5,) * 3)
    cases = (([Resize(8), ColorJitter(), ToTensor()], "ColorJitter"),
             ([Resize(8, max_size=16), ToTensor()], "max_size"),
             ([Resize(8, antialias=False), ToTensor()], "antialias=False"),
             ([Resize(8), CenterCrop(4)], "ToTensor is missing"),
             ([Resize(8), norm, ToTensor()], "Normalize before ToTensor"),
             ([Resize(8), norm], "Normalize before ToTensor"),
             ([Resize(8, interpolation=InterpolationMode.NEAREST), ToTensor()], "nearest"),
             ([Resize(8, interpolation=0), ToTensor()], "nearest"),
             ([CenterCrop(4), Resize(8), ToTensor()], "Resize after CenterCrop"),
             ([ToTensor(), Resize(8)], "Resize after ToTensor"),
             ([Resize(8), Resize(4), ToTensor()], "Resize after Resize"))
    for ops, needle in cases:
        with pytest.raises(ValueError, match=needle):
            DeviceTransform.from_torchvision(Compose(ops))
    with pytest.raises(ValueError, match="transforms"):
        DeviceTransform.from_torchvision(lambda image: image)


# ----------------------------------------------------------------------------- the host statement of the chain
def test_host_chain_is_pillow_then_torchvisions_arithmetic():
    from PIL import Image
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    got = DeviceTransform(resize=24, interpolation="bicubic", crop=16, mean=mean, std=std).host(Image.fromarray(img))
    res = np.asarray(Image.fromarray(img).resize((34, 24), Image.Resampling.BICUBIC))[4:20, 9:25]
    x = torch.from_numpy(res.copy()).permute(2, 0, 1).float() / 255
    want = (x - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    assert got.dtype == torch.float32 and got.shape == (3, 16, 16) and torch.equal(got, want)
    assert torch.equal(DeviceTransform().host(img), torch.from_numpy(img).permute(2, 0, 1).float() / 255)


# ----------------------------------------------------------------------------- the plugin API keeps its defaults
def _tiny_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(),
                               torch.nn.Linear(8, 16))


def test_components_and_registration_keep_the_host_route_by_default():
    import dataclasses
    from atlaspatch_amd.encoders.base import DeviceTorchFeatureExtractor, PatchFeatureExtractor
    from atlaspatch_amd.encoders.custom import CustomEncoderComponents, register_custom_encoder
    from atlaspatch_amd.encoders.registry import PatchFeatureExtractorRegistry
    model = _tiny_model()
    transform = DeviceTransform(mean=(0.5,) * 3, std=(0.5,) * 3)
    parts = CustomEncoderComponents(model, transform.host)                                  # positional, as the reference's plugins write it
    assert parts.forward_fn is None and parts.device_transform is None
    assert [f.name for f in dataclasses.fields(CustomEncoderComponents)] == ["model", "preprocess", "forward_fn", "device_transform"]
    assert CustomEncoderComponents(model, transform.host, None, transform).device_transform is transform

    registry = PatchFeatureExtractorRegistry()
    cpu = torch.device("cpu")
    register_custom_encoder(registry=registry, name="plain", embedding_dim=16, loader=lambda d, t: parts, device=cpu, dtype=torch.float32)
    register_custom_encoder(registry=registry, name="described", embedding_dim=16, device=cpu, dtype=torch.float32, device_batch=64,
                            loader=lambda d, t: CustomEncoderComponents(model, transform.host, device_transform=transform))
    plain, described = registry.create("plain"), registry.create("described")
    assert type(plain) is PatchFeatureExtractor
    assert type(described) is PatchFeatureExtractor                  # a CPU device: today's class, whatever the loader describes
    rng = np.random.default_rng(0)
    patches = [rng.integers(0, 256, (20, 24, 3), dtype=np.uint8) for _ in range(5)]
    a, b = plain.extract_batch(patches, batch_size=2), described.extract_batch(patches, batch_size=2)
    assert a.shape == (5, 16) and a.dtype == np.float32 and np.array_equal(a, b)
    with torch.inference_mode():
        want = model(torch.stack([transform.host(p) for p in patches[:2]])).numpy()
    assert np.array_equal(a[:2], want)

    # the device class on a CPU device behaves exactly as PatchFeatureExtractor
    direct = DeviceTorchFeatureExtractor(name="d", model=model, embedding_dim=16, preprocess=transform.host, device=cpu,
                                         dtype=torch.float32, device_transform=transform, max_batch=2)
    assert np.array_equal(direct.extract_batch(patches, batch_size=2), a)
    assert direct.extract_batch([]).shape == (0, 16)
    with pytest.raises(TypeError, match="device_transform must be a DeviceTransform"):
        register_custom_encoder(registry=registry, name="wrong", embedding_dim=16, device=torch.device("cuda"), dtype=torch.float32,
                                loader=lambda d, t: CustomEncoderComponents(model, transform.host, device_transform=object()))
        registry.create("wrong")


def test_the_service_asks_for_the_capability_not_for_a_class():
    from atlaspatch_amd.services.feature_embedding import _speaks_ring

    class Speaks:
        name, embedding_dim, device = "x", 4, torch.device("cuda:0")

        def forward_device(self, tiles, out):
            return out

    class Host(Speaks):
        forward_device = None

    class OnCpu(Speaks):
        device = torch.device("cpu")

    assert _speaks_ring(Speaks()) and not _speaks_ring(Host()) and not _speaks_ring(OnCpu()) and not _speaks_ring(object())
