"""Device half of the split JPEG decode: ap_host_jpeg_coefficients -> H2D -> ap_jpeg_decode_tiles -> D2H equals Pillow in
every byte (ap_host_jpeg_probe and ap_jpeg_slot_bytes supply the geometry), and the tile ring with ATLASPATCH_JPEG_DEVICE=1
produces the host path's features exactly."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import jpeg_reference as ref
from tests import jpeg_streams as js

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes of poison in front of and behind rgb (keeps rgb 16-byte aligned)
POISON = 0xCD


@pytest.fixture(scope="module")
def lib():
    from atlaspatch_amd import _lib
    return _lib.load()


def _host_slots(lib, paths, side, sampling):
    from atlaspatch_amd import _lib
    rc, slots = js.read_slots(lib, paths, side, sampling)
    if rc == _lib.AP_ERR_UNSUPPORTED:
        pytest.skip("no usable libjpeg.so.8 on this host: " + lib.ap_last_error().decode())
    assert rc == 0, lib.ap_last_error()
    # what the kernel must not read: the padding behind the tables, and the tables a greyscale slot does not use
    slots[:, (128 if sampling == ref.GRAY else 384):512] = 0xEE
    return slots


def _device_decode(lib, slots, side, sampling, *, lead=0, tail=0):
    """uint8 [n, side, side, 3] from host slots [n, stride]; the slots sit ``lead`` bytes into a poisoned device buffer with
    ``tail`` poisoned bytes behind them, rgb between two guards in a poisoned buffer of its own."""
    from atlaspatch_amd import _lib
    n, stride = slots.shape
    assert lead % 16 == 0
    src = torch.full((lead + n * stride + tail,), 0x77, dtype=torch.uint8, device="cuda")
    src[lead:lead + n * stride] = torch.from_numpy(slots.reshape(-1))
    out_bytes = n * side * side * 3
    dst = torch.full((GUARD + out_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert (src.data_ptr() + lead) % 16 == 0 and (dst.data_ptr() + GUARD) % 16 == 0
    _lib.check(lib.ap_jpeg_decode_tiles(src.data_ptr() + lead, n, side, sampling, dst.data_ptr() + GUARD,
                                        _lib.current_stream_ptr()), "ap_jpeg_decode_tiles")
    got = dst.cpu().numpy()
    assert (got[:GUARD] == POISON).all() and (got[GUARD + out_bytes:] == POISON).all(), "wrote outside rgb"
    back = src.cpu().numpy()
    assert (back[:lead] == 0x77).all() and (back[lead + n * stride:] == 0x77).all()
    assert np.array_equal(back[lead:lead + n * stride], slots.reshape(-1)), "the slots were modified"
    return got[GUARD:GUARD + out_bytes].reshape(n, side, side, 3)


def _compare(got, streams, labels):
    for i, (stream, label) in enumerate(zip(streams, labels)):
        want = js.pillow_rgb(stream)
        if not np.array_equal(got[i], want):
            bad = np.argwhere(got[i] != want)
            raise AssertionError(f"tile {i} ({label}): {len(bad)} bytes differ, first at {bad[0].tolist()}: "
                                 f"{int(got[i][tuple(bad[0])])} != {int(want[tuple(bad[0])])}")


@pytest.mark.parametrize("sampling", js.SAMPLINGS)
@pytest.mark.parametrize("side", js.SIDES)
def test_device_decode_equals_pillow(lib, tmp_path, side, sampling):
    """Side 8: one block, a ragged band; 24: a partial MCU and a ragged last band; 25: odd, the crop after upsampling; 40: two
    and a half bands, the chroma halo crosses band borders; 16: exactly one band."""
    cases = js.matrix(side, sampling)
    streams = [s for _, s in cases]
    slots = _host_slots(lib, js.write_files(tmp_path, streams), side, sampling)
    assert len(cases) == 15
    _compare(_device_decode(lib, slots, side, sampling), streams, [l for l, _ in cases])


@pytest.mark.parametrize("side", (1, 3, 4, 5, 12, 32, 48))
def test_device_decode_of_tiny_tiles_and_whole_group_rows(lib, tmp_path, side):
    """Chroma planes at most two samples wide are replicated, not interpolated (sides up to 4); 5 and 12 sit just above.
    32 and 48 are multiples of 16, two and three bands: the output stage whose 16-pixel groups lie in one row each, with the
    chroma halo crossing band borders (16 in the matrix is its one-band case, 256 below its many-band one)."""
    for sampling in js.SAMPLINGS:
        streams = [js.encode(js.pixels(side, c), sampling, 90) for c in js.CONTENTS]
        slots = _host_slots(lib, js.write_files(tmp_path, streams, f"s{sampling}_"), side, sampling)
        _compare(_device_decode(lib, slots, side, sampling), streams, [f"sampling {sampling}"] * 3)


@pytest.mark.parametrize("sampling", js.SAMPLINGS)
def test_device_decode_of_a_tissue_tile(lib, tmp_path, sampling):
    """One 256-pixel synthetic-tissue tile at quality 80, the tile store's setting (16 bands of 64 + 2 x 48 blocks at 4:2:0),
    next to a noise tile and a saturated checkerboard of the same size."""
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, render_region
    spec = SynthSpec(width=12000, height=9000, seed=7)
    tissue = None
    for cx, cy, a, b in spec.ellipses().tolist():          # the first rim tile that holds tissue and background both
        for x0, y0 in ((16 * (cx - a) - 128, 16 * cy - 128), (16 * cx - 128, 16 * (cy - b) - 128)):
            t = render_region(spec, max(0, x0), max(0, y0), 256, 256, 0)
            if tissue is None and 0.2 < (t[..., 0] > 233).mean() < 0.8:
                tissue = t
    assert tissue is not None and tissue.shape == (256, 256, 3)
    board = np.zeros((256, 256, 3), dtype=np.uint8)
    board[::2, ::2] = 255
    board[1::2, 1::2] = (255, 0, 255)
    streams = [js.encode(tissue, sampling, 80), js.encode(js.pixels(256, "noise"), sampling, 80), js.encode(board, sampling, 100),
               js.encode(board, sampling, 1)]
    slots = _host_slots(lib, js.write_files(tmp_path, streams), 256, sampling)
    _compare(_device_decode(lib, slots, 256, sampling), streams, ["tissue", "noise", "board q100", "board q1"])


@pytest.mark.parametrize("n", (1, 3, 65))
def test_batch_sizes_and_slot_pitch(lib, tmp_path, n):
    """n tiles in one call, the slots at slot_bytes pitch inside a larger poisoned buffer (not at its start, not to its end)."""
    for side, sampling in ((40, ref.S420), (25, ref.S422), (24, ref.S444), (8, ref.GRAY)):
        base = js.matrix(side, sampling)
        cases = [base[i % len(base)] for i in range(n)]
        streams = [s for _, s in cases]
        slots = _host_slots(lib, js.write_files(tmp_path, streams, f"b{side}_"), side, sampling)
        assert slots.shape == (n, lib.ap_jpeg_slot_bytes(side, sampling))
        got = _device_decode(lib, slots, side, sampling, lead=4096 + 16, tail=1000)
        _compare(got, streams, [l for l, _ in cases])


def test_argument_refusals_and_empty_batch(lib):
    from atlaspatch_amd import _lib
    stride = lib.ap_jpeg_slot_bytes(16, ref.S420)
    src = torch.zeros(2 * stride + 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((2 * 16 * 16 * 3 + 64,), POISON, dtype=torch.uint8, device="cuda")
    s, d, stream = src.data_ptr(), dst.data_ptr(), _lib.current_stream_ptr()
    call = lib.ap_jpeg_decode_tiles
    assert call(s, 0, 16, ref.S420, d, stream) == 0
    for args in ((None, 1, 16, ref.S420, d), (s, 1, 16, ref.S420, None), (s, 1, 0, ref.S420, d), (s, 1, -16, ref.S420, d),
                 (s, -1, 16, ref.S420, d), (s, 1, 16, 4, d), (s, 1, 16, -1, d), (s + 8, 1, 16, ref.S420, d),
                 (s, 1, 16, ref.S420, d + 4), (s, 1, 4096, ref.S444, d)):
        assert call(*args, stream) == _lib.AP_ERR_INVALID, args
        assert lib.ap_last_error()
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == POISON).all()


# ----------------------------------------------------------------------------- the ring
def _store(tmp_path, name, n_expected=(30, 80)):
    """A ~50-tile slide with its tiles as JPEG files at quality 80 (Pillow's default 4:2:0): (slide path, coords, store)."""
    from PIL import Image
    from atlaspatch_amd.core.wsi.synth_pixels import SynthSpec, analytic_mask, render_region
    from atlaspatch_amd.services.extraction import coords_from_mask
    raw = {"width": 5000, "height": 4000, "seed": 7, "n_ellipses": 3, "mag": 20, "mpp": 0.5, "downsamples": [1, 4, 16],
           "jpeg_tiles": "tiles"}
    folder = tmp_path / name
    store = folder / "tiles"
    store.mkdir(parents=True)
    slide = folder / "j.synth"
    slide.write_text(json.dumps(raw))
    spec = SynthSpec(width=raw["width"], height=raw["height"], seed=raw["seed"], n_ellipses=raw["n_ellipses"])
    coords, _ = coords_from_mask(analytic_mask(spec), level0_wh=(spec.width, spec.height), downsamples=[1.0, 4.0, 16.0],
                                 src_mag=20, tgt_mag=20, patch_size=256, step_size=None, tissue_thresh=0.0)
    assert n_expected[0] <= coords.shape[0] <= n_expected[1], coords.shape
    for x, y in coords[:, :2]:
        Image.fromarray(render_region(spec, int(x), int(y), 256, 256, 0)).save(str(store / f"{x}_{y}_256.jpg"), quality=80)
    return str(slide), spec, coords, store


def _process(slide, out, monkeypatch, device_jpeg, workers=4):
    """(features, tiles the ring decoded on the device, tiles it decoded on the host while the device path was on)"""
    from click.testing import CliRunner
    from atlaspatch_amd.cli import cli
    from atlaspatch_amd.services import tile_ring
    from atlaspatch_amd.utils.h5 import h5
    monkeypatch.setenv("ATLASPATCH_RANDOM_INIT", "0")
    if device_jpeg:
        monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    else:
        monkeypatch.delenv("ATLASPATCH_JPEG_DEVICE", raising=False)
    before = dict(tile_ring.JPEG_TILES)
    res = CliRunner().invoke(cli, ["process", slide, "-o", str(out), "--patch-size", "256", "--target-mag", "20",
                                   "--feature-extractors", "vit_b_16", "--feature-precision", "float16",
                                   "--feature-num-workers", str(workers)], catch_exceptions=False)
    assert res.exit_code == 0 and "failures: 0" in res.output, res.output
    with h5.File(out / "patches" / "j.h5", "r") as f:
        got_coords, feats = f["coords"][:], f["features"]["vit_b_16"][:]
    return got_coords, feats, tile_ring.JPEG_TILES["device"] - before["device"], tile_ring.JPEG_TILES["host"] - before["host"]


def test_ring_with_device_jpeg_decode_gives_the_host_paths_features(tmp_path, monkeypatch):
    slide, spec, coords, store = _store(tmp_path, "regular")
    c0, want, dev0, host0 = _process(slide, tmp_path / "out_host", monkeypatch, False)
    c1, got, dev1, host1 = _process(slide, tmp_path / "out_device", monkeypatch, True)
    n = coords.shape[0]
    assert np.array_equal(c0, coords) and np.array_equal(c1, coords)
    assert (dev0, host0) == (0, 0), "the switch is off: no tile may take the device decoder"
    assert (dev1, host1) == (n, 0), "the switch is on: every tile is decoded by ap_jpeg_decode_tiles"
    assert want.dtype == got.dtype == np.float32 and np.array_equal(got, want)
    assert np.abs(want).max() > 0


def test_ring_with_a_mixed_store_sends_the_odd_chunks_to_the_host(tmp_path, monkeypatch):
    """One progressive tile, one 4:4:4 tile in the 4:2:0 store and one missing tile: their chunks take the host route
    (read_tiles_into refuses the chunk with the missing tile too, which is then rendered tile by tile), every other chunk the device's."""
    from PIL import Image
    slide, spec, coords, store = _store(tmp_path, "mixed")
    n, workers = coords.shape[0], 4
    chunk = -(-n // (4 * workers))                    # TileRing.run's task size for a single batch of n tiles
    assert n <= 64 and chunk >= 2
    odd = [chunk + 1, 4 * chunk, n - 1]              # three different chunks, none of them the first (the probe's)
    assert len({i // chunk for i in odd}) == 3 and 0 not in {i // chunk for i in odd}
    paths = [store / f"{x}_{y}_256.jpg" for x, y in coords[:, :2]]
    Image.open(paths[odd[0]]).save(str(paths[odd[0]]) + ".tmp.jpg", quality=80, progressive=True)
    os.replace(str(paths[odd[0]]) + ".tmp.jpg", paths[odd[0]])
    Image.open(paths[odd[1]]).save(str(paths[odd[1]]) + ".tmp.jpg", quality=80, subsampling=0)
    os.replace(str(paths[odd[1]]) + ".tmp.jpg", paths[odd[1]])
    os.remove(paths[odd[2]])
    host_tiles = sum(min(n, (c + 1) * chunk) - c * chunk for c in {i // chunk for i in odd})
    c0, want, dev0, host0 = _process(slide, tmp_path / "out_host", monkeypatch, False, workers)
    c1, got, dev1, host1 = _process(slide, tmp_path / "out_device", monkeypatch, True, workers)
    assert (dev0, host0) == (0, 0)
    assert (dev1, host1) == (n - host_tiles, host_tiles)
    assert np.array_equal(got, want)
    # the odd tiles were really embedded from other pixels than their neighbours': the rows differ from each other
    assert len({want[i].tobytes() for i in odd}) == 3
