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


# ----------------------------------------------------------------------------- the tile sources, without a ring or a device
POISON = 0xA5


def _poisoned(*shape):
    import torch
    t = torch.full(shape, POISON, dtype=torch.uint8)
    assert t.data_ptr() % 16 == 0
    return t


def _sources(monkeypatch, wsi, coords):
    """(the stream source, the coefficient source, tile slots per row) of the routes ``wsi`` offers under both switches."""
    from atlaspatch_amd.services import tile_routes as tr
    monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    monkeypatch.setenv("ATLASPATCH_JPEG_ENTROPY_DEVICE", "1")
    stream, coef = tr.routes_for(wsi, coords, (256, 256))
    assert (type(stream.source), type(coef.source)) == (tr.StreamTiles, tr.CoefficientTiles) and stream.per_row == coef.per_row
    assert (stream.source.merges, coef.source.merges) == (False, True)
    return stream.source, coef.source, stream.per_row


def _check_fills(stream, coef, per_row, rows_held, start, items, share, direct_coefficients, direct_streams):
    """``fill`` of both sources for a chunk that starts at coords row ``start`` of a slot of ``rows_held`` rows, on poisoned CPU buffers
    the test owns: what lands where, against the C entry called directly into fresh buffers, and nothing outside the chunk's share."""
    import torch
    m, first, tiles, bound = len(items), start * per_row, rows_held * per_row, stream.bound
    assert m <= share and first + share <= tiles
    # coefficient slots: tile slot start * per_row onwards
    buf = SimpleNamespace(host=[_poisoned(tiles, coef.slot_bytes)])
    want = _poisoned(m, coef.slot_bytes)
    assert direct_coefficients(want.data_ptr()) == 0
    assert coef.fill(buf, 0, first, items, share) is True
    assert torch.equal(buf.host[0][first:first + m], want) and not (want == POISON).all()
    assert (buf.host[0][:first] == POISON).all() and (buf.host[0][first + m:] == POISON).all()
    # descriptors: tile slot start * per_row onwards; the arena share: byte start * per_row * bound onwards, share * bound long
    buf = SimpleNamespace(desc_host=[_poisoned(tiles, stream.header)], arena_host=[_poisoned(tiles * bound)])
    descs, arena, used = _poisoned(m, stream.header), _poisoned(share * bound), C.c_size_t()
    assert direct_streams(descs.data_ptr(), arena.data_ptr(), share * bound, C.byref(used)) == 0 and 0 < used.value <= share * bound
    assert stream.fill(buf, 0, first, items, share) == used.value
    assert torch.equal(buf.desc_host[0][first:first + m], descs) and not (descs == POISON).all()
    assert torch.equal(buf.arena_host[0][first * bound:(first + share) * bound], arena) and not (arena[:used.value] == POISON).all()
    assert (buf.desc_host[0][:first] == POISON).all() and (buf.desc_host[0][first + m:] == POISON).all()
    assert (buf.arena_host[0][:first * bound] == POISON).all() and (buf.arena_host[0][(first + share) * bound:] == POISON).all()


def _store_or_skip(tmp_path, width):
    from atlaspatch_amd import _lib
    from atlaspatch_amd.core.wsi.synth_wsi import SynthWSI
    slide, coords, _ = jpeg_store(tmp_path, tf.image(width, 256, 21))
    lib, w, h, s = _lib.load(), C.c_int(), C.c_int(), C.c_int()
    if lib.ap_host_jpeg_probe(str(tmp_path / "tiles" / "0_0_256.jpg").encode(), C.byref(w), C.byref(h), C.byref(s)) == _lib.AP_ERR_UNSUPPORTED:
        pytest.skip("no usable libjpeg.so.8 on this host: " + lib.ap_last_error().decode())
    return lib, SynthWSI(slide), coords


def test_the_sources_fill_a_store_chunk_at_its_tile_slot(tmp_path, monkeypatch):
    """A 4-tile JPEG store, one tile per row; the chunk starts at row 3 of an 8-row slot."""
    lib, wsi, coords = _store_or_skip(tmp_path, 1024)
    stream, coef, per_row = _sources(monkeypatch, wsi, coords)
    assert per_row == 1 and len(coords) == 4
    paths = [str(tmp_path / "tiles" / f"{x}_{y}_256.jpg").encode() for x, y in coords[:, :2].tolist()]
    arr = (C.c_char_p * 4)(*paths)
    _check_fills(stream, coef, 1, 8, 3, coords.tolist(), 4,
                 lambda slots: lib.ap_host_jpeg_coefficients(slots, arr, 4, 256, coef.sampling),
                 lambda descs, arena, cap, used: lib.ap_host_jpeg_streams(descs, arena, cap, used, arr, 4, 256, stream.sampling))


def test_the_sources_fill_a_tile_grid_chunk_at_its_tile_slot(tmp_path, monkeypatch):
    """The ts = 240 TIFF: 9 tile slots per row; a chunk of three rows starts at row 2 of a 5-row slot."""
    from atlaspatch_amd import _lib
    wsi = _tiff(tmp_path / "t.tif", 240)
    stream, coef, per_row = _sources(monkeypatch, wsi, _grid_coords())
    assert per_row == 9
    rows = _grid_coords()[[1, 6, 11]].tolist()
    geometry = wsi.tile_gather_geometry(rows, 256)
    ids, _ = wsi.tile_gather_plan(rows, geometry, 256)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    lib, m = _lib.load(), int(ids.shape[0])
    assert 9 < m <= 27, "the chunk's distinct tiles reach past its first row's slots"
    _check_fills(stream, coef, 9, 5, 2, ids, 27,
                 lambda slots: lib.ap_host_tiff_tile_coefficients(wsi._handle, 0, ids.ctypes.data, m, slots),
                 lambda descs, arena, cap, used: lib.ap_host_tiff_tile_streams(wsi._handle, 0, ids.ctypes.data, m, descs, arena, cap, used))
    wsi.cleanup()


def test_a_chunk_the_stager_refuses_fills_to_none(tmp_path, monkeypatch):
    """The third of four tiles is progressive: both sources refuse the chunk (None).  As at the C entries, the tiles in front of the
    refused one are staged, its own slot / descriptor and those behind it keep the poison, and nothing outside the share is touched."""
    from PIL import Image
    lib, wsi, coords = _store_or_skip(tmp_path, 1024)
    stream, coef, _ = _sources(monkeypatch, wsi, coords)
    bad = tmp_path / "tiles" / "512_0_256.jpg"
    with Image.open(bad) as im:
        im.convert("RGB").save(str(bad), quality=80, progressive=True)
    bound, first = stream.bound, 3
    buf = SimpleNamespace(host=[_poisoned(8, coef.slot_bytes)], desc_host=[_poisoned(8, stream.header)], arena_host=[_poisoned(8 * bound)])
    assert coef.fill(buf, 0, first, coords.tolist(), 4) is None and b"progressive" in lib.ap_last_error()
    assert stream.fill(buf, 0, first, coords.tolist(), 4) is None and b"progressive" in lib.ap_last_error()
    for held in (buf.host[0], buf.desc_host[0]):
        assert not (held[first] == POISON).all() and not (held[first + 1] == POISON).all()
        assert (held[:first] == POISON).all() and (held[first + 2:] == POISON).all()
    assert (buf.arena_host[0][:first * bound] == POISON).all() and (buf.arena_host[0][(first + 4) * bound:] == POISON).all()
    # inside the share: byte for byte what the C entry leaves behind a refusal at the same capacity -- the two tiles in front staged,
    # *arena_used standing behind them (not 0, not the whole share) -- while the source's answer is None
    import torch
    arr = (C.c_char_p * 4)(*[str(tmp_path / "tiles" / f"{x}_{y}_256.jpg").encode() for x, y in coords[:, :2].tolist()])
    descs, arena, used = _poisoned(4, stream.header), _poisoned(4 * bound), C.c_size_t()
    assert lib.ap_host_jpeg_streams(descs.data_ptr(), arena.data_ptr(), 4 * bound, C.byref(used), arr, 4, 256, stream.sampling) != 0
    assert 0 < used.value < 4 * bound and used.value % 16 == 0
    assert torch.equal(buf.desc_host[0][first:first + 4], descs) and torch.equal(buf.arena_host[0][first * bound:(first + 4) * bound], arena)
    assert not (arena[:used.value] == POISON).all()


def _unprepared(route, rows_held):
    """``route`` with the pinned half of its buffer set made here from poisoned CPU tensors, as ``prepare`` would on a ring."""
    tiles, source = rows_held * route.per_row, route.source
    held = dict(host=[_poisoned(tiles, route.slot_bytes)]) if not source.flags else \
        dict(desc_host=[_poisoned(tiles, source.header)], arena_host=[_poisoned(tiles * source.bound)])
    route.buf = SimpleNamespace(**held)
    route.plan_np = [np.full((rows_held, 4 + route.per_row), -9, dtype=np.int32)]
    return route.buf


def test_the_routes_hand_their_sources_the_row_index_in_tile_slots(tmp_path, monkeypatch):
    """``fill`` of the routes themselves: a store route's chunk at row 3 lands at tile slot 3, a tile-grid route's chunk at row 2 at
    tile slot 2 * 9 with its plan in rows 2 .. 4, and each equals its source's ``fill`` at that slot."""
    import torch
    from atlaspatch_amd.services import tile_routes as tr
    lib, store, coords = _store_or_skip(tmp_path / "s", 1024)
    wsi = _tiff(tmp_path / "t.tif", 240)
    monkeypatch.setenv("ATLASPATCH_JPEG_DEVICE", "1")
    monkeypatch.setenv("ATLASPATCH_JPEG_ENTROPY_DEVICE", "1")
    grid_rows = _grid_coords()[[1, 6, 11]].tolist()
    for routes, rows, start in ((tr.routes_for(store, coords, (256, 256)), coords.tolist(), 3),
                                (tr.routes_for(wsi, _grid_coords(), (256, 256)), grid_rows, 2)):
        for route in routes:
            per_row, source = route.per_row, route.source
            buf = _unprepared(route, 8)
            token, plan = route.fill(0, start, rows), route.plan_np[0]
            items, staged = (rows, token) if per_row == 1 else (wsi.tile_gather_plan(rows, route.geometry, 256)[0], token[1])
            want = _unprepared(route, 8)
            assert source.fill(want, 0, start * per_row, items, len(rows) * per_row) == staged and staged is not None
            for name, got in vars(buf).items():
                assert torch.equal(got[0], getattr(want, name)[0]) and not (got[0] == POISON).all(), (type(route), name)
            if per_row > 1:
                assert token[0] == len(items) and (plan[:start] == -9).all() and (plan[start + 3:] == -9).all()
                assert np.array_equal(plan[start:start + 3], wsi.tile_gather_plan(rows, route.geometry, 256)[1])
            first = start * per_row
            head = buf.host[0] if not source.flags else buf.desc_host[0]
            assert (head[:first] == POISON).all() and not (head[first] == POISON).all()
    wsi.cleanup()
