"""The tile ring's host logic without a GPU (services/tile_ring.py, services/tile_routes.py): the batch cuts, the merging of a batch's
chunks into runs, and ``routes_for`` on a tiled-JPEG TIFF, a JPEG `.synth` store and a backend with no device capability."""
import ctypes as C
import json
from types import SimpleNamespace

import numpy as np
import pytest

from tests import tiff_fixture as tf


# ----------------------------------------------------------------------------- batch cuts
@pytest.mark.parametrize("batch", (1, 16, 64, 2048))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 797, 8989))
def test_batch_cuts_tile_the_rows_and_ramp_up(n, batch):
    from atlaspatch_amd.services.tile_ring import batch_cuts
    cuts = batch_cuts(n, batch)
    assert cuts[0][0] == 0 and cuts[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])), "the cuts tile [0, n) in order"
    sizes = [hi - lo for lo, hi in cuts]
    assert min(sizes) >= 1 and max(sizes) <= batch
    assert sizes[0] == min(n, max(1, min(batch, max(64, batch // 8))))
    for i in range(1, len(sizes)):
        full = min(batch, 2 * sizes[i - 1])
        assert sizes[i] == full or (i == len(sizes) - 1 and sizes[i] < full), (i, sizes)


def test_batch_cuts_of_a_long_slide():
    from atlaspatch_amd.services.tile_ring import batch_cuts
    assert [hi - lo for lo, hi in batch_cuts(8989, 2048)] == [256, 512, 1024, 2048, 2048, 2048, 1053]
    assert batch_cuts(0, 2048) == []


# ----------------------------------------------------------------------------- run merging
PIXEL, COEF = SimpleNamespace(merges=True), SimpleNamespace(merges=True)
GRID = SimpleNamespace(merges=False)


@pytest.mark.parametrize("taken,count,chunk,want", (
    ([(PIXEL, True)] * 4, 16, 4, [(0, 16, PIXEL, True)]),
    ([(COEF, True)] * 4, 16, 4, [(0, 16, COEF, True)]),
    ([(PIXEL, True), (COEF, True), (PIXEL, True), (COEF, True)], 16, 4,
     [(0, 4, PIXEL, True), (4, 8, COEF, True), (8, 12, PIXEL, True), (12, 16, COEF, True)]),
    ([(COEF, True), (COEF, True), (PIXEL, True), (PIXEL, True), (PIXEL, True), (COEF, True)], 17, 3,        # a short last chunk
     [(0, 6, COEF, True), (6, 15, PIXEL, True), (15, 17, COEF, True)]),
    ([(GRID, 5), (GRID, 7), (GRID, 0)], 7, 3, [(0, 3, GRID, 5), (3, 6, GRID, 7), (6, 7, GRID, 0)]),          # each keeps its tile count
    ([(PIXEL, True), (GRID, 4), (GRID, 4), (PIXEL, True), (PIXEL, True), (GRID, 9)], 11, 2,
     [(0, 2, PIXEL, True), (2, 4, GRID, 4), (4, 6, GRID, 4), (6, 10, PIXEL, True), (10, 11, GRID, 9)]),
    ([(PIXEL, True)], 1, 1, [(0, 1, PIXEL, True)]),
))
def test_merge_runs_gives_the_maximal_runs(taken, count, chunk, want):
    from atlaspatch_amd.services.tile_ring import merge_runs
    runs = merge_runs(taken, count, chunk)
    assert runs == want
    assert runs[0][0] == 0 and runs[-1][1] == count and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert all(stop - start <= chunk for start, stop, route, _ in runs if route is GRID), "two tile-grid chunks share a run"
    assert all(a[2] is not b[2] or a[2] is GRID for a, b in zip(runs, runs[1:])), "two adjacent runs could have been one"


# ----------------------------------------------------------------------------- the probe
def jpeg_store(folder, full):
    """A JPEG `.synth` store of the 256-px tiles of ``full`` (uint8 [h, w, 3]) on the tile grid, Pillow's quality 80 at 4:2:0:
    (slide path, coords int32 [n, 5], uint8 [n, 256, 256, 3] = Pillow's decode of every stored tile)."""
    from PIL import Image
    height, width = full.shape[:2]
    store = folder / "tiles"
    store.mkdir(parents=True)
    slide = folder / "j.synth"
    slide.write_text(json.dumps({"width": width, "height": height, "seed": 7, "n_ellipses": 3, "mag": 20, "mpp": 0.5,
                                 "downsamples": [1, 4, 16], "jpeg_tiles": "tiles"}))
    coords = np.array([[x, y, 256, 256, 0] for y in range(0, height, 256) for x in range(0, width, 256)], dtype=np.int32)
    tiles = []
    for x, y in coords[:, :2].tolist():
        path = store / f"{x}_{y}_256.jpg"
        Image.fromarray(full[y:y + 256, x:x + 256]).save(str(path), quality=80)
        with Image.open(path) as im:
            tiles.append(np.asarray(im.convert("RGB")))
    return str(slide), coords, np.stack(tiles)


def _grid_coords():
    return np.array([[x, y, 256, 256, 0] for y in range(0, 768, 256) for x in range(0, 1024, 256)], dtype=np.int32)


def _tiff(path, ts):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.core.wsi.tiff_wsi import TiffWSI
    tf.write_tiff(path, [tf.image(1024, 768, 21)], tile=(ts, ts))
    wsi = TiffWSI(str(path))
    wsi._ensure_loaded()
    out = np.zeros((16, 16, 3), dtype=np.uint8)
    if _lib.load().ap_host_tiff_read_patches(wsi._handle, 0, np.zeros((1, 2), dtype=np.int64).ctypes.data, 1, 16, 16,
                                             out.ctypes.data) == _lib.AP_ERR_UNSUPPORTED:
        pytest.skip("no usable libjpeg.so.8 on this host: " + _lib.load().ap_last_error().decode())
    return wsi


@pytest.mark.parametrize("ts,per_row", ((256, 4), (240, 9)))
def test_probe_of_a_tiled_tiff(tmp_path, monkeypatch, ts, per_row):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.services.tile_routes import TileGridRoute, routes_for
    wsi = _tiff(tmp_path / "t.tif", ts)
    monkeypatch.delenv("ATLASPATCH_JPEG_DEVICE", raising=False)
    assert routes_for(wsi, _grid_coords(), (256, 256)) == []
    monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    routes = routes_for(wsi, _grid_coords(), (256, 256))
    assert [type(r) for r in routes] == [TileGridRoute]
    sampling = wsi.levels[0]["sampling"]
    slot = int(_lib.load().ap_jpeg_slot_bytes(ts, sampling))
    assert slot > 0 and routes[0].G ** 2 == per_row and routes[0].pinned_row_bytes == slot * per_row
    assert routes_for(wsi, _grid_coords(), (256, 224)) == [], "device routes are for square reads"
    wsi.cleanup()


def test_probe_of_a_jpeg_store(tmp_path, monkeypatch):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.core.wsi.synth_wsi import SynthWSI
    from atlaspatch_amd.services.tile_routes import CoefficientRoute, routes_for
    slide, coords, _ = jpeg_store(tmp_path, tf.image(1024, 768, 21))
    lib = _lib.load()
    w, h, s = C.c_int(), C.c_int(), C.c_int()
    code = lib.ap_host_jpeg_probe(str(tmp_path / "tiles" / "0_0_256.jpg").encode(), C.byref(w), C.byref(h), C.byref(s))
    if code == _lib.AP_ERR_UNSUPPORTED:
        pytest.skip("no usable libjpeg.so.8 on this host: " + lib.ap_last_error().decode())
    wsi = SynthWSI(slide)
    monkeypatch.delenv("ATLASPATCH_JPEG_DEVICE", raising=False)
    assert routes_for(wsi, coords, (256, 256)) == []
    monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    routes = routes_for(wsi, coords, (256, 256))
    assert [type(r) for r in routes] == [CoefficientRoute]
    assert code == _lib.AP_OK and routes[0].sampling == s.value
    assert routes[0].pinned_row_bytes == int(lib.ap_jpeg_slot_bytes(256, s.value)) > 0


def test_probe_of_a_backend_without_device_capabilities(monkeypatch):
    from atlaspatch_amd.services.tile_routes import routes_for
    monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    plain = SimpleNamespace(extract=lambda *a, **k: None, read_tiles_into=lambda rows, ptr, side: False)
    assert routes_for(plain, _grid_coords(), (256, 256)) == []
